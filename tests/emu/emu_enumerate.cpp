// tests/emu/emu_enumerate.cpp -- whole batches through the emulated device code (emu_harness.cpp: serial enumerate functions, descriptors,
// lane-per-item code, scan formulation) as a program for AddressSanitizer and UBSan (CPU only).  TEST INFRASTRUCTURE ONLY.
// emu_enumerate_asan IN OUT: IN holds an index and hand-built batches (tests/emu_enumerate_lib.py writes it).  Every sequence, every index
// array and every batch array is copied into a heap block of its exact size, so a load of the device code that leaves its array -- a read
// segment that leaves its contig makes rev_pos negative -- ends the program.  Every batch is lifted twice: light items through the
// lane-per-item code (lane_max_w as the engine's default) and everything through the scan formulation.  OUT receives both results.
#include "emu_harness.cpp"

#include <stdio.h>
#include <stdlib.h>

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
    std::vector<void *> blocks;
    // `count` values of `size` bytes in a heap block of exactly that many bytes
    template <class T>
    T *block(uint64_t count) {
        T *p = (T *)malloc(count * sizeof(T));
        if (count) get(p, count * sizeof(T));
        blocks.push_back(p);
        return p;
    }
    void release() {
        for (void *p : blocks) free(p);
        blocks.clear();
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
    if (rd.u32() != 0x314d4e45u) return 3;  // "ENM1"
    // ---- the index ----
    Reader ixr;  // (owns the index blocks for the whole run)
    plo_index_desc ix;
    memset(&ix, 0, sizeof(ix));
    ix.n_contigs = rd.u32();
    ix.n_segments = rd.u32();
    ix.n_chroms = rd.u32();
    const uint32_t n_seg_cigar = rd.u32();
    if (!rd.ok) return 3;
    ix.contig_len = rd.block<int64_t>(ix.n_contigs);
    ix.contig_seg_off = rd.block<uint32_t>((uint64_t)ix.n_contigs + 1);
    ix.seg_chrom_index = rd.block<uint32_t>(ix.n_segments);
    ix.seg_pos = rd.block<int64_t>(ix.n_segments);
    ix.seg_is_fwd_strand = rd.block<uint8_t>(ix.n_segments);
    ix.seg_mapq = rd.block<uint8_t>(ix.n_segments);
    ix.seg_seq_order_start = rd.block<int64_t>(ix.n_segments);
    ix.seg_seq_order_end = rd.block<int64_t>(ix.n_segments);
    ix.seg_cigar_off = rd.block<uint32_t>((uint64_t)ix.n_segments + 1);
    ix.seg_cigar = rd.block<uint32_t>(n_seg_cigar);
    int64_t *chrom_len = rd.block<int64_t>(ix.n_chroms);
    ix.chrom_len = chrom_len;
    const uint8_t **chrom_seq = (const uint8_t **)malloc(sizeof(void *) * (ix.n_chroms ? ix.n_chroms : 1));
    const uint8_t **rev_seq = (const uint8_t **)malloc(sizeof(void *) * (ix.n_contigs ? ix.n_contigs : 1));
    for (uint32_t c = 0; c < ix.n_chroms; ++c) chrom_seq[c] = rd.block<uint8_t>((uint64_t)chrom_len[c]);
    for (uint32_t c = 0; c < ix.n_contigs; ++c) rev_seq[c] = rd.u32() ? rd.block<uint8_t>((uint64_t)ix.contig_len[c]) : nullptr;
    ix.chrom_seq = chrom_seq;
    ix.rev_contig_seq = rev_seq;
    ix.seq_mem = PLO_MEM_HOST;
    ixr.blocks.swap(rd.blocks);
    if (!rd.ok) return 3;
    // ---- the batches ----
    const uint32_t n_cases = rd.u32();
    for (uint32_t cs = 0; cs < n_cases; ++cs) {
        plo_batch_in in;
        memset(&in, 0, sizeof(in));
        const uint32_t stages = rd.u32(), lane_max_w = rd.u32();
        in.seq_fmt = (int32_t)rd.u32();
        in.n_reads = rd.u32();
        in.n_segs = rd.u32();
        const uint32_t n_cigar = rd.u32(), has_list = rd.u32(), n_list = rd.u32();
        in.seq_bytes = rd.u64();
        if (!rd.ok) return 3;
        in.read_is_reverse = rd.block<uint8_t>(in.n_reads);
        in.read_seq_len = rd.block<uint32_t>(in.n_reads);
        in.read_seq_off = rd.block<uint64_t>(in.n_reads);
        in.seq = rd.block<uint8_t>(in.seq_bytes);
        in.seg_read = rd.block<uint32_t>(in.n_segs);
        in.seg_contig = rd.block<uint32_t>(in.n_segs);
        in.seg_pos = rd.block<int64_t>(in.n_segs);
        in.seg_is_fwd_strand = rd.block<uint8_t>(in.n_segs);
        in.seg_cigar_off = rd.block<uint32_t>((uint64_t)in.n_segs + 1);
        in.cigar = rd.block<uint32_t>(n_cigar);
        if (has_list) {  // the caller's item list (k_item_desc's branch)
            in.n_items = n_list;
            in.item_seg = rd.block<uint32_t>(n_list);
            in.item_cseg = rd.block<uint32_t>(n_list);
        }
        if (!rd.ok) return 3;
        for (int mode = 0; mode < 2; ++mode) {
            plo_batch_out out;
            memset(&out, 0, sizeof(out));
            unsigned long long counters[24];
            const int rc = emu_liftover_batch(&ix, &in, stages, 768, 256, 256, 1 << 16, 0, 0, 2048, mode == 0 ? (int)lane_max_w : -1, 3072, 0, 0, 0, &out, counters);
            const uint32_t n = out.n_items;
            put32(o, (uint32_t)rc);
            put32(o, n);
            put32(o, (uint32_t)counters[23]);
            put(o, out.item_seg, (size_t)n * 4);
            put(o, out.item_cseg, (size_t)n * 4);
            put(o, out.item_status, n);
            put(o, out.item_need_flipped, n);
            put(o, out.item_mapq, n);
            put(o, out.item_chrom_index, (size_t)n * 4);
            put(o, out.item_ref_pos, (size_t)n * 8);
            put(o, out.item_cigar_len, (size_t)n * 4);
            uint64_t total = 0;
            for (uint32_t i = 0; i < n; ++i) total += out.item_cigar_len[i];
            put64(o, total);
            for (uint32_t i = 0; i < n; ++i) put(o, out.cigar + out.item_cigar_off[i], (size_t)out.item_cigar_len[i] * 4);
            emu_free_last();
        }
        rd.release();
    }
    if (rd.at != rd.all.size()) return 3;
    ixr.release();
    free(chrom_seq);
    free(rev_seq);
    fclose(o);
    return 0;
}
