// tests/emu/emu_finish.cpp -- record finishing and SA text (finish_core.hpp) as a program for AddressSanitizer and UBSan (CPU only).
// TEST INFRASTRUCTURE ONLY.  emu_finish_asan IN OUT: IN holds hand-built batches (tests/emu_finish_lib.py writes it); every input array of a
// batch is copied into a heap block of its exact size -- bases and qualities into a block of `shift` + their bytes, used from `shift` on,
// so their last byte is the block's last -- every output is a heap block of its exact size (emu_finish.hpp), and the batch is finished
// at each thread count.  OUT receives every result for the test to compare.
#include <plo_wave.hpp>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "emu_finish.hpp"

namespace {
struct Reader {
    std::vector<uint8_t> all;
    size_t at = 0;
    bool ok = true;
    void get(void *dst, size_t n) {
        if (at + n > all.size()) {
            ok = false;
            memset(dst, 0, n);
            return;
        }
        memcpy(dst, all.data() + at, n);
        at += n;
    }
    uint32_t u32() {
        uint32_t v;
        get(&v, 4);
        return v;
    }
    uint64_t u64() {
        uint64_t v;
        get(&v, 8);
        return v;
    }
    // `count` values of `size` bytes in a heap block of exactly that many bytes, `lead` unused bytes in front
    uint8_t *block(uint64_t count, size_t size, uint32_t lead = 0) {
        uint8_t *p = (uint8_t *)malloc(lead + count * size);
        if (count) get(p + lead, count * size);
        return p;
    }
};
void put(FILE *o, const void *p, size_t n) {
    if (n) fwrite(p, 1, n, o);
}
void put32(FILE *o, uint32_t v) { fwrite(&v, 4, 1, o); }
void put64(FILE *o, uint64_t v) { fwrite(&v, 8, 1, o); }
}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    Reader rd;
    uint8_t buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof(buf), f)) > 0) rd.all.insert(rd.all.end(), buf, buf + k);
    fclose(f);
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    if (rd.u32() != 0x314e4946u) return 3;  // "FIN1"
    const uint32_t n_cases = rd.u32();
    for (uint32_t cs = 0; cs < n_cases; ++cs) {
        uint32_t n_threads = rd.u32(), threads[8];
        if (n_threads > 8) return 3;
        for (uint32_t t = 0; t < n_threads; ++t) threads[t] = rd.u32();
        const uint32_t fmt = rd.u32(), nr = rd.u32(), ns = rd.u32(), n = rd.u32(), n_chroms = rd.u32(), shift = rd.u32(), one_buffer = rd.u32(), do_sa = rd.u32();
        const uint64_t n_cigar = rd.u64(), seq_bytes = rd.u64(), qual_bytes = rd.u64(), names_bytes = rd.u64();
        if (!rd.ok || shift > 3) return 3;
        plo_batch_in in;
        memset(&in, 0, sizeof(in));
        plo_finish_in fin;
        memset(&fin, 0, sizeof(fin));
        plo_batch_out lift;
        memset(&lift, 0, sizeof(lift));
        std::vector<void *> blocks;
        auto keep = [&](uint8_t *p) {
            blocks.push_back(p);
            return p;
        };
        in.n_reads = nr;
        in.n_segs = ns;
        in.seq_fmt = (int32_t)fmt;
        in.read_seq_len = (uint32_t *)keep(rd.block(nr, 4));
        in.read_seq_off = (uint64_t *)keep(rd.block(nr, 8));
        fin.read_flags = (uint16_t *)keep(rd.block(nr, 2));
        fin.read_qual_off = (uint64_t *)keep(rd.block(nr, 8));
        in.seg_read = (uint32_t *)keep(rd.block(ns, 4));
        in.seq = keep(rd.block(seq_bytes, 1, shift)) + shift;
        in.seq_bytes = seq_bytes;
        fin.qual = one_buffer ? in.seq : keep(rd.block(qual_bytes, 1, shift)) + shift;
        fin.qual_bytes = qual_bytes;
        lift.n_items = n;
        lift.item_seg = (uint32_t *)keep(rd.block(n, 4));
        lift.item_status = keep(rd.block(n, 1));
        lift.item_need_flipped = keep(rd.block(n, 1));
        lift.item_mapq = keep(rd.block(n, 1));
        lift.item_chrom_index = (uint32_t *)keep(rd.block(n, 4));
        lift.item_ref_pos = (int64_t *)keep(rd.block(n, 8));
        lift.item_cigar_off = (uint64_t *)keep(rd.block(n, 8));
        lift.item_cigar_len = (uint32_t *)keep(rd.block(n, 4));
        lift.cigar = (uint32_t *)keep(rd.block(n_cigar, 4));
        lift.n_cigar = n_cigar;
        uint32_t *name_off = (uint32_t *)keep(rd.block((uint64_t)n_chroms + 1, 4));
        uint8_t *names = keep(rd.block(names_bytes, 1));
        if (!rd.ok) return 3;
        for (uint32_t t = 0; t < n_threads; ++t) {
            FinOut fo;
            plo_finish_out out;
            memset(&out, 0, sizeof(out));
            const int n_fault = emu_finish_run(&in, &fin, &lift, (int)threads[t], &fo, &out);
            put32(o, (uint32_t)n_fault);
            put(o, out.item_flag, (size_t)n * 2);
            put(o, out.item_bin, (size_t)n * 2);
            put(o, out.item_ref_end, (size_t)n * 8);
            put(o, out.item_is_primary, n);
            put(o, out.item_seq_off, (size_t)n * 8);
            put(o, out.item_qual_off, (size_t)n * 8);
            put(o, out.read_n_lifted, (size_t)nr * 4);
            put(o, out.read_primary_item, (size_t)nr * 4);
            put(o, out.read_unmapped_flag, (size_t)nr * 2);
            put(o, out.read_seq_off, (size_t)nr * 8);
            put(o, out.read_qual_off, (size_t)nr * 8);
            put64(o, out.rev_seq_bytes);
            put64(o, out.rev_qual_bytes);
            put(o, out.rev_seq, out.rev_seq_bytes);
            put(o, out.rev_qual, out.rev_qual_bytes);
            if (do_sa && t == 0) {
                // item_read, flags and records per read as the finishing left them, each in a block of its exact size
                uint32_t *iread = (uint32_t *)malloc((size_t)n * 4), *nl = (uint32_t *)malloc((size_t)nr * 4);
                uint16_t *fl = (uint16_t *)malloc((size_t)n * 2);
                if (n) memcpy(iread, fo.iread.data(), (size_t)n * 4);
                if (n) memcpy(fl, out.item_flag, (size_t)n * 2);
                if (nr) memcpy(nl, out.read_n_lifted, (size_t)nr * 4);
                uint32_t *off = nullptr;
                uint8_t *text = nullptr;
                if (emu_sa_segments(&lift, fl, iread, nl, name_off, names, &off, &text) != 0) return 4;
                put(o, off, ((size_t)n + 1) * 4);
                put(o, text, off[n]);
                emu_sa_free(off, text);
                free(iread);
                free(nl);
                free(fl);
            }
        }
        for (void *p : blocks) free(p);
    }
    if (rd.at != rd.all.size()) return 3;
    fclose(o);
    return 0;
}
