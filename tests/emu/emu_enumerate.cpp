// tests/emu/emu_enumerate.cpp -- whole batches through the emulated device code (emu_harness.cpp: serial enumerate functions, descriptors,
// lane-per-item code, scan formulation) as a program for AddressSanitizer and UBSan (CPU only).  TEST INFRASTRUCTURE ONLY.
// emu_enumerate_asan IN OUT: IN holds an index and hand-built batches (tests/emu_enumerate_lib.py writes it).  Every sequence, every index
// array and every batch array is copied into a heap block of its exact size, so a load of the device code that leaves its array -- a read
// segment that leaves its contig makes rev_pos negative -- ends the program.  Every batch is lifted twice: light items through the
// lane-per-item code (lane_max_w as the engine's default) and everything through the scan formulation.  OUT receives both results.
#include "emu_harness.cpp"

#include "emu_batch_file.hpp"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    Reader rd;
    if (!rd.load(argv[1])) return 2;
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    FileIndex fi;
    if (!fi.load(rd)) return 3;
    const uint32_t n_cases = rd.u32();
    for (uint32_t cs = 0; cs < n_cases; ++cs) {
        plo_batch_in in;
        uint32_t stages, lane_max_w;
        if (!load_batch(rd, in, stages, lane_max_w)) return 3;
        for (int mode = 0; mode < 2; ++mode) {
            plo_batch_out out;
            memset(&out, 0, sizeof(out));
            unsigned long long counters[24];
            const int rc = emu_liftover_batch(&fi.ix, &in, stages, 768, 256, 256, 1 << 16, 0, 0, 2048, mode == 0 ? (int)lane_max_w : -1, 3072, 0, 0, 0, &out, counters);
            put_result(o, rc, out, (uint32_t)counters[23]);
            emu_free_last();
        }
        rd.release();
    }
    if (rd.at != rd.all.size()) return 3;
    fi.release();
    fclose(o);
    return 0;
}
