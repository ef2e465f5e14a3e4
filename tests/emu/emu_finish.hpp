// tests/emu/emu_finish.hpp -- record finishing and SA text (finish_core.hpp) executed on the host: what k_finish_items / k_finish_reads /
// k_finish_offsets / k_revcomp and k_sa_len / k_sa_emit do on the GPU, with plain loops standing in for the threads.  Shared by the
// emulator library (emu_harness.cpp) and the sanitizer program (emu_finish.cpp).  TEST INFRASTRUCTURE ONLY.  Include behind plo_wave.hpp.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../portello_amd/csrc/finish_core.hpp"

namespace {
// the outputs of one finished batch.  The reversed bases and qualities are heap blocks of exactly rev_seq_bytes / rev_qual_bytes
// (16-byte aligned, as the device's are), so a store behind a slot's last unit is a store behind the block.
struct FinOut {
    std::vector<uint16_t> flag, bin, uflag;
    std::vector<int64_t> rend;
    std::vector<uint8_t> prim;
    std::vector<uint64_t> isoff, iqoff, rsoff, rqoff;
    std::vector<uint32_t> iread, nl, pitem, su, qu, soff, qoff, fflag, frank, flist;
    uint8_t *rseq = nullptr, *rqual = nullptr;
    FinOut() {}
    FinOut(const FinOut &) = delete;
    FinOut &operator=(const FinOut &) = delete;
    ~FinOut() {
        free(rseq);
        free(rqual);
    }
};
inline uint8_t *emu_fin_block16(uint64_t bytes) { return (uint8_t *)aligned_alloc(16, bytes ? (size_t)bytes : 16); }

// -> the number of items that ended LEN_MISMATCH / PANIC / NEED_BASES (plo_finish_batch_dev refuses the batch when it is not 0; the
// emulation goes on, so that the counting itself can be tested)
inline int emu_finish_run(const plo_batch_in *in, const plo_finish_in *fin, const plo_batch_out *lift, int nthreads, FinOut *o, plo_finish_out *out) {
    plo::DevBatch bt;
    memset(&bt, 0, sizeof(bt));
    bt.read_seq_len = in->read_seq_len;
    bt.read_seq_off = in->read_seq_off;
    bt.seq = in->seq;
    bt.seq_fmt = in->seq_fmt;
    bt.seq_bytes = in->seq_bytes;
    bt.seg_read = in->seg_read;
    bt.n_reads = in->n_reads;
    bt.n_segs = in->n_segs;
    plo::DevWork wk;
    memset(&wk, 0, sizeof(wk));
    uint32_t n = lift->n_items, nr = in->n_reads, ne = n + nr;
    wk.n_items = n;
    wk.item_seg = (uint32_t *)lift->item_seg;
    wk.status = (uint8_t *)lift->item_status;
    wk.flip = (uint8_t *)lift->item_need_flipped;
    wk.mapq = (uint8_t *)lift->item_mapq;
    wk.pos = (int64_t *)lift->item_ref_pos;
    wk.cig_off = (uint64_t *)lift->item_cigar_off;
    wk.cig_len = (uint32_t *)lift->item_cigar_len;
    wk.out_cigar = (uint32_t *)lift->cigar;
    size_t a = n ? n : 1, b = nr ? nr : 1, e = ne ? ne : 1;
    o->flag.assign(a, 0); o->bin.assign(a, 0); o->rend.assign(a, 0); o->prim.assign(a, 0); o->isoff.assign(a, 0); o->iqoff.assign(a, 0);
    o->iread.assign(a, 0); o->nl.assign(b, 0); o->pitem.assign(b, 0); o->uflag.assign(b, 0); o->rsoff.assign(b, 0); o->rqoff.assign(b, 0);
    o->su.assign(e, 0); o->qu.assign(e, 0); o->soff.assign(e + 1, 0); o->qoff.assign(e + 1, 0); o->fflag.assign(e, 0);
    o->frank.assign(e + 1, 0); o->flist.assign(e, 0);
    plo::DevFinish f;
    memset(&f, 0, sizeof(f));
    unsigned n_fault = 0;
    f.n_fault = &n_fault;
    f.read_flags = fin->read_flags; f.qual = fin->qual; f.read_qual_off = fin->read_qual_off; f.qual_bytes = fin->qual_bytes;
    f.seq_bytes = in->seq_bytes;
    f.item_flag = o->flag.data(); f.item_bin = o->bin.data(); f.item_ref_end = o->rend.data(); f.item_is_primary = o->prim.data();
    f.item_seq_off = o->isoff.data(); f.item_qual_off = o->iqoff.data(); f.item_read = o->iread.data();
    f.read_n_lifted = o->nl.data(); f.read_primary_item = o->pitem.data(); f.read_unmapped_flag = o->uflag.data();
    f.read_seq_off = o->rsoff.data(); f.read_qual_off_out = o->rqoff.data();
    f.su = o->su.data(); f.qu = o->qu.data(); f.soff = o->soff.data(); f.qoff = o->qoff.data();
    f.fflag = o->fflag.data(); f.frank = o->frank.data(); f.flist = o->flist.data();
    for (uint32_t i = 0; i < n; ++i) plo::finish_item(bt, wk, f, i);
    for (uint32_t r = 0; r < nr; ++r) plo::finish_read(bt, wk, f, r);
    for (uint32_t k = 0; k < ne; ++k) {
        o->soff[k + 1] = o->soff[k] + o->su[k];
        o->qoff[k + 1] = o->qoff[k] + o->qu[k];
        o->frank[k + 1] = o->frank[k] + o->fflag[k];
    }
    for (uint32_t k = 0; k < ne; ++k) {
        uint64_t so = o->su[k] ? (uint64_t)o->soff[k] * 16u : PLO_NO_FLIP, qo = o->qu[k] ? (uint64_t)o->qoff[k] * 16u : PLO_NO_FLIP;
        if (o->su[k]) o->flist[o->frank[k]] = k;
        if (k < n) { o->isoff[k] = so; o->iqoff[k] = qo; } else { o->rsoff[k - n] = so; o->rqoff[k - n] = qo; }
    }
    const uint64_t sb = (uint64_t)o->soff[ne] * 16u, qb = (uint64_t)o->qoff[ne] * 16u;
    free(o->rseq);
    free(o->rqual);
    uint8_t *rs = o->rseq = emu_fin_block16(sb);
    uint8_t *rq = o->rqual = emu_fin_block16(qb);
    memset(rs, 0xEE, sb ? sb : 16);
    memset(rq, 0xEE, qb ? qb : 16);
    f.rev_seq = rs;
    f.rev_qual = rq;
    for (uint32_t k = 0; k < o->frank[ne]; ++k) {
        uint32_t en = o->flist[k];
        uint32_t read = en < n ? o->iread[en] : en - n;
        for (int t = 0; t < nthreads; ++t)
            plo::revcomp_record(bt, f, read, rs + (uint64_t)o->soff[en] * 16u, rq + (uint64_t)o->qoff[en] * 16u, t, nthreads);
    }
    out->item_flag = f.item_flag; out->item_bin = f.item_bin; out->item_ref_end = f.item_ref_end; out->item_is_primary = f.item_is_primary;
    out->item_seq_off = f.item_seq_off; out->item_qual_off = f.item_qual_off; out->read_n_lifted = f.read_n_lifted;
    out->read_primary_item = f.read_primary_item; out->read_unmapped_flag = f.read_unmapped_flag; out->read_seq_off = f.read_seq_off;
    out->read_qual_off = f.read_qual_off_out; out->rev_seq = rs; out->rev_qual = rq;
    out->rev_seq_bytes = sb; out->rev_qual_bytes = qb;
    out->n_items = n; out->n_reads = ne - n;
    return (int)n_fault;
}
FinOut *g_fin = nullptr;
}  // namespace

// the results stay alive until the next call
extern "C" int emu_finish_batch(const plo_batch_in *in, const plo_finish_in *fin, const plo_batch_out *lift, int nthreads, plo_finish_out *out) {
    delete g_fin;
    g_fin = new FinOut();
    return emu_finish_run(in, fin, lift, nthreads, g_fin, out);
}

// SA tag segments: finish_core.hpp's sa_item_len / sa_item_emit executed on the host.  `lift` and the finish arrays are host
// copies; off ([n_items + 1]) and text (exactly off[n_items] bytes) are malloc'ed and released by emu_sa_free.
extern "C" int emu_sa_segments(const plo_batch_out *lift, const uint16_t *item_flag, const uint32_t *item_read, const uint32_t *read_n_lifted,
                               const uint32_t *chrom_name_off, const uint8_t *chrom_names, uint32_t **off_out, uint8_t **text_out) {
    plo::DevWork wk;
    memset(&wk, 0, sizeof(wk));
    wk.n_items = lift->n_items;
    wk.status = (uint8_t *)lift->item_status;
    wk.flip = (uint8_t *)lift->item_need_flipped;
    wk.chrom = (uint32_t *)lift->item_chrom_index;
    wk.pos = (int64_t *)lift->item_ref_pos;
    wk.mapq = (uint8_t *)lift->item_mapq;
    wk.cig_off = (uint64_t *)lift->item_cigar_off;
    wk.cig_len = (uint32_t *)lift->item_cigar_len;
    wk.out_cigar = (uint32_t *)lift->cigar;
    uint32_t n = lift->n_items;
    std::vector<uint32_t> len(n + 1, 0);
    uint32_t *off = (uint32_t *)malloc(((size_t)n + 1) * 4);
    plo::DevSa sa;
    sa.chrom_name_off = chrom_name_off;
    sa.chrom_names = chrom_names;
    sa.item_flag = item_flag;
    sa.item_read = item_read;
    sa.read_n_lifted = read_n_lifted;
    sa.len = len.data();
    sa.off = off;
    sa.text = nullptr;
    for (uint32_t i = 0; i < n; ++i) len[i] = plo::sa_item_len(wk, sa, i);
    off[0] = 0;
    for (uint32_t i = 0; i < n; ++i) off[i + 1] = off[i] + len[i];
    uint8_t *text = (uint8_t *)malloc(off[n] ? off[n] : 1);
    sa.text = text;
    for (uint32_t i = 0; i < n; ++i) plo::sa_item_emit(wk, sa, i);
    *off_out = off;
    *text_out = text;
    return 0;
}
extern "C" void emu_sa_free(uint32_t *off, uint8_t *text) {
    free(off);
    free(text);
}
