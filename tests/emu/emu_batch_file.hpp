// tests/emu/emu_batch_file.hpp -- the file format of the sanitizer programs that lift whole batches (emu_enumerate.cpp, emu_liftover.cpp): an
// index and hand-built batches as tests/emu_enumerate_lib.py writes them, every array copied into a heap block of its exact size, and the
// results as that module reads them back.  TEST INFRASTRUCTURE ONLY.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/portello_liftover.h"  // plo_index_desc, plo_batch_in, plo_batch_out

namespace {
struct Reader {
    std::vector<uint8_t> all;
    size_t at = 0;
    bool ok = true;
    bool load(const char *path) {
        FILE *f = fopen(path, "rb");
        if (!f) return false;
        uint8_t buf[65536];
        size_t k;
        while ((k = fread(buf, 1, sizeof(buf), f)) > 0) all.insert(all.end(), buf, buf + k);
        fclose(f);
        return true;
    }
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

// the index ("ENM1" header first); its blocks move from `rd` to `keep`, which owns them for the whole run
struct FileIndex {
    plo_index_desc ix;
    Reader keep;
    const uint8_t **chrom_seq = nullptr, **rev_seq = nullptr;
    bool load(Reader &rd) {
        if (rd.u32() != 0x314d4e45u) return false;  // "ENM1"
        memset(&ix, 0, sizeof(ix));
        ix.n_contigs = rd.u32();
        ix.n_segments = rd.u32();
        ix.n_chroms = rd.u32();
        const uint32_t n_seg_cigar = rd.u32();
        if (!rd.ok) return false;
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
        chrom_seq = (const uint8_t **)malloc(sizeof(void *) * (ix.n_chroms ? ix.n_chroms : 1));
        rev_seq = (const uint8_t **)malloc(sizeof(void *) * (ix.n_contigs ? ix.n_contigs : 1));
        for (uint32_t c = 0; c < ix.n_chroms; ++c) chrom_seq[c] = rd.block<uint8_t>((uint64_t)chrom_len[c]);
        for (uint32_t c = 0; c < ix.n_contigs; ++c) rev_seq[c] = rd.u32() ? rd.block<uint8_t>((uint64_t)ix.contig_len[c]) : nullptr;
        ix.chrom_seq = chrom_seq;
        ix.rev_contig_seq = rev_seq;
        ix.seq_mem = PLO_MEM_HOST;
        keep.blocks.swap(rd.blocks);
        return rd.ok;
    }
    void release() {
        keep.release();
        free(chrom_seq);
        free(rev_seq);
    }
};

// one batch; its blocks stay with `rd` until rd.release()
bool load_batch(Reader &rd, plo_batch_in &in, uint32_t &stages, uint32_t &lane_max_w) {
    memset(&in, 0, sizeof(in));
    stages = rd.u32();
    lane_max_w = rd.u32();
    in.seq_fmt = (int32_t)rd.u32();
    in.n_reads = rd.u32();
    in.n_segs = rd.u32();
    const uint32_t n_cigar = rd.u32(), has_list = rd.u32(), n_list = rd.u32();
    in.seq_bytes = rd.u64();
    if (!rd.ok) return false;
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
    return rd.ok;
}

// one result: the return code, the item count, `extra` (a count of the caller's), then the items
void put_result(FILE *o, int rc, const plo_batch_out &out, uint32_t extra) {
    const uint32_t n = out.n_items;
    put32(o, (uint32_t)rc);
    put32(o, n);
    put32(o, extra);
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
}
}  // namespace
