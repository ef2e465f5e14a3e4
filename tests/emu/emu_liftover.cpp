// tests/emu/emu_liftover.cpp -- the catalogue of tests/liftover_cases.py through the emulated liftover stage (emu_harness.cpp) as a program
// for AddressSanitizer and UBSan (CPU only).  TEST INFRASTRUCTURE ONLY.
// emu_liftover_asan IN OUT: IN holds an index and hand-built batches (tests/emu_enumerate_lib.py's format).  Every index array, the batch
// CIGAR and every other batch array is copied into a heap block of its exact size; the packed block maps (ix.kv) are a vector cut to its
// size and the program is compiled with the vector annotations, so a cursor's look-ahead that reads the entry behind the last map's last key
// -- the map-end cases of family S are there for it -- ends the program.  Every batch is lifted four times: lane_tile with 32-bit and with
// 16-bit regions (light items by the engine's default weight), the window route (every item heavy, groups of 64), and the streaming kernel
// (one team; all stages only: a batch with another stage set stops after the window route).  OUT receives every result with the route's
// retry count.
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
        uint32_t stages, heavy_max_w;  // (heavy_max_w: the weight limit of the heavy routes)
        if (!load_batch(rd, in, stages, heavy_max_w)) return 3;
        const int n_modes = (stages & PLO_STAGES_ALL) == PLO_STAGES_ALL ? 4 : 3;
        for (int mode = 0; mode < n_modes; ++mode) {
            plo_batch_out out;
            memset(&out, 0, sizeof(out));
            unsigned long long counters[24];
            setenv("PLO_EMU_H16", mode == 1 ? "1" : "0", 1);
            const int max_w = mode < 2 ? 192 : (int)heavy_max_w;
            const int per = mode < 2 ? 0 : (mode == 3 ? 1024 : 64);
            const int rc = emu_liftover_batch(&fi.ix, &in, stages, 768, 256, 256, 1 << 16, 0, 0, 2048, max_w, 3072, per, 0, mode == 3 ? 1 : 0, &out, counters);
            put_result(o, rc, out, (uint32_t)counters[CNT_NRETRY]);
            emu_free_last();
        }
        rd.release();
    }
    if (rd.at != rd.all.size()) return 3;
    fi.release();
    fclose(o);
    return 0;
}
