// aln_walk.hpp -- the walk of a lifted item's output CIGAR against the reference, shared by nm_core.hpp, md_core.hpp and eqx_core.hpp.
//   a wave per item (aln_items: persistent waves, items by ticket).  aln_open reads what the item is made of: its bases, its room on the
//   chromosome, its CIGAR.  aln_step takes the ops 64 per step, one per lane; their read and reference advances are scanned across the wave,
//   and the bounds check of the step comes out of the same scans, before a base of the step is touched: nothing outside
//   [seq, seq + (l_seq + 1) / 2) or the chromosome is read by a caller that stops where `ok` is false.
//   An op is cut into PIECES at the 16-byte lines of the reference's ADDRESSES (aln_lines of them; aln_span: the bytes of piece j).  The
//   caller says how many pieces each op of the step has, scans the counts and deals the pieces to the lanes 64 per trip; a lane finds the
//   op of its piece by a search over that scan (aln_find_op: six shuffles).  64 matches of a few bases are one trip, a match of 15 kb is
//   fifteen.  What a piece is worth, and what is carried across trips and steps, is the caller's.
#pragma once
#include <plo_wave.hpp>
#include <stdint.h>

#include "records_core.hpp"

namespace plo {

constexpr int NM_NO_ITEM = 0x7fffffff;  // err_item when no item was refused

// the context's finishing result and the index: the base of DevNm, DevMd and DevEqx, so their first 40 bytes and `d.item_seq_off` as before
struct AlnSrc {
    const uint64_t *item_seq_off;  // PLO_NO_FLIP: the record keeps the source's bases
    const uint8_t *rev_seq;
    const uint8_t *const *chrom_seq;
    const int *chrom_len;
    uint32_t n_chroms;
};

// is item i LIFTED?  Only such an item has bases, a place on a chromosome and a CIGAR to open
PLO_DEV bool aln_lifted(const DevWork &wk, uint32_t i) { return wk.status[i] == PLO_ITEM_LIFTED; }

// (uniform) the view of a LIFTED item
struct AlnItem {
    bool ok;                      // false: it has no chromosome or no place on it; the caller refuses it and walks nothing
    const uint8_t *seq;           // the record's 4-bit bases, [seq_lo, seq_hi) their addresses
    uintptr_t seq_lo, seq_hi;
    unsigned long long lseq, ref_room;  // its bases; the bytes of the chromosome from its position on
    uintptr_t ref0;               // the address of the first of them
    const uint32_t *cg;
    uint32_t n;
};

PLO_DEV AlnItem aln_open(const DevBatch &bt, const DevWork &wk, const AlnSrc &d, uint32_t i) {
    AlnItem it;
    const uint32_t read = bt.seg_read[wk.item_seg[i]];
    it.lseq = bt.read_seq_len[read];
    const uint64_t so = d.item_seq_off[i];
    it.seq = so != PLO_NO_FLIP ? d.rev_seq + so : bt.seq + bt.read_seq_off[read];
    it.seq_lo = (uintptr_t)it.seq;
    it.seq_hi = it.seq_lo + (uintptr_t)((it.lseq + 1) / 2);
    const uint32_t chrom = wk.chrom[i];
    const long long pos = wk.pos[i];
    const long long clen = chrom < d.n_chroms ? (long long)d.chrom_len[chrom] : -1;
    const uint8_t *ref = chrom < d.n_chroms ? d.chrom_seq[chrom] : nullptr;
    it.ok = !(pos < 0 || pos > clen || (!ref && clen > 0));
    it.ref_room = (unsigned long long)(clen - pos);
    it.ref0 = (uintptr_t)ref + (uintptr_t)pos;
    it.n = wk.cig_len[i];
    it.cg = wk.out_cigar + wk.cig_off[i];
    return it;
}

// the lane's op of a step: ops [k, k + 64) of the item, rd_done / rf_done (uniform) consumed by the steps before
struct AlnStep {
    bool ok;                            // (uniform) false: the step's ops leave the read or the chromosome: none of their bases may be touched
    bool has, is_cmp;                   // the lane has an op; it is M, = or X
    uint32_t c, t, len;                 // the op, its code and length (0 without an op)
    unsigned long long rd;              // the read position of its first base
    uintptr_t fa;                       // the address of its first reference byte
    unsigned long long rd_end, rf_end;  // (uniform) consumed behind the step
};

// the step of the lane's op word c (has: the lane has one): the scans, the bounds check, the op's first read base and reference byte
PLO_DEV AlnStep aln_step_op(const AlnItem &it, bool has, uint32_t c, unsigned long long rd_done, unsigned long long rf_done) {
    AlnStep s;
    s.has = has;
    s.c = s.has ? c : 0u;
    s.t = s.c & 15u;
    s.len = s.c >> 4;
    s.is_cmp = s.has && (s.t == 0 || s.t == 7 || s.t == 8);
    const unsigned long long rd_adv = s.has && ((0x193u >> s.t) & 1u) ? s.len : 0u;  // M I S = X
    const unsigned long long rf_adv = s.has && ((0x18Du >> s.t) & 1u) ? s.len : 0u;  // M D N = X
    const unsigned long long rd_inc = wave_scan_incl_u64(rd_adv), rf_inc = wave_scan_incl_u64(rf_adv);
    s.rd_end = rd_done + wv::shfl(rd_inc, 63);
    s.rf_end = rf_done + wv::shfl(rf_inc, 63);
    s.ok = !(s.rd_end > it.lseq || s.rf_end > it.ref_room);
    s.rd = rd_done + rd_inc - rd_adv;
    s.fa = it.ref0 + (uintptr_t)(rf_done + rf_inc - rf_adv);
    return s;
}

PLO_DEV AlnStep aln_step(const AlnItem &it, uint32_t k, unsigned long long rd_done, unsigned long long rf_done) {
    const bool has = k + (uint32_t)wv::lane() < it.n;
    return aln_step_op(it, has, has ? it.cg[k + wv::lane()] : 0u, rd_done, rf_done);
}

// A RECORD's view (pileup_core.hpp): l_seq bases at seq, ref0 the address of the reference byte at its position, ref_room the chromosome's
// bytes from there on, n ops at cig.  A record lies at any byte address, so its ops are no aligned words: `cg` keeps the address only, and
// the walk of such a view takes its steps with aln_step_bytes, never with aln_step.
PLO_DEV AlnItem aln_open_record(const uint8_t *seq, unsigned long long lseq, uintptr_t ref0, unsigned long long ref_room, const uint8_t *cig, uint32_t n) {
    AlnItem it;
    it.ok = true;
    it.seq = seq;
    it.seq_lo = (uintptr_t)seq;
    it.seq_hi = it.seq_lo + (uintptr_t)((lseq + 1) / 2);
    it.lseq = lseq;
    it.ref_room = ref_room;
    it.ref0 = ref0;
    it.cg = (const uint32_t *)(const void *)cig;
    it.n = n;
    return it;
}
// aln_step for a view opened by aln_open_record: the op is read a byte at a time
PLO_DEV AlnStep aln_step_bytes(const AlnItem &it, uint32_t k, unsigned long long rd_done, unsigned long long rf_done) {
    const bool has = k + (uint32_t)wv::lane() < it.n;
    return aln_step_op(it, has, has ? rec_rd32((const uint8_t *)(const void *)it.cg + 4ull * (k + (uint32_t)wv::lane())) : 0u, rd_done, rf_done);
}

// the 16-byte lines that reference bytes [fa, fa + len) lie on, len > 0
PLO_DEV uint32_t aln_lines(uintptr_t fa, uint32_t len) { return (uint32_t)(((fa + len + 15) >> 4) - (fa >> 4)); }

// the bytes [s, e) of them on line j (piece j of the op)
struct AlnSpan { uintptr_t s, e; };
PLO_DEV AlnSpan aln_span(uintptr_t fa, uint32_t len, uint32_t j) {
    uintptr_t s = (fa & ~(uintptr_t)15) + 16u * (uintptr_t)j, e = s + 16;
    if (s < fa) s = fa;
    if (e > fa + len) e = fa + len;
    return AlnSpan{s, e};
}

// the op of piece p of a step: np the lane's own op's pieces, p_inc their inclusive scan.  A p behind the last piece finds some lane.
struct AlnOp {
    int lane;                  // the op's lane: the first with p_inc > p
    uint32_t np, first;        // its pieces, and the number of the first of them
    uint32_t c, t, len;        // the op, its code and length
    uintptr_t fa;              // and where it starts: AlnStep's fa and rd
    unsigned long long rd;
};
PLO_DEV AlnOp aln_find_op(const AlnStep &st, uint32_t np, uint32_t p_inc, uint32_t p) {
    AlnOp o;
    int l = 0;
    for (int s = 32; s; s >>= 1)
        if (wv::shfl(p_inc, l + s - 1) <= p) l += s;
    l &= 63;
    o.lane = l;
    o.np = wv::shfl(np, l);
    o.first = wv::shfl(p_inc, l) - o.np;
    o.c = wv::shfl(st.c, l);
    o.t = o.c & 15u;
    o.len = o.c >> 4;
    o.fa = (uintptr_t)wv::shfl((unsigned long long)st.fa, l);
    o.rd = wv::shfl(st.rd, l);
    return o;
}

// item i is refused: the batch's lowest refused item, and nothing for the item itself
template <class T>
PLO_DEV void aln_refuse(int *err_item, T *item_out, uint32_t i) {
    if (wv::lane() == 0) {
        wv::atomic_min(err_item, (int)i);
        item_out[i] = 0;
    }
}

// persistent waves: items by ticket
template <class F>
PLO_DEV void aln_items(uint32_t n_items, unsigned *ticket, F item) {
    for (;;) {
        unsigned i = 0;
        if (wv::lane() == 0) i = wv::atomic_add_global(ticket, 1u);
        i = wv::bcast_first(i);
        if (i >= n_items) break;
        item(i);
    }
}

}  // namespace plo
