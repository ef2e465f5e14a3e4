// eqx_core.hpp -- the CIGARs of the lifted records with '=' and 'X' in place of 'M', written on the device (plo_eqx_dev).  The lift maps every
// compared op to M; pbmm2 writes = / X, and so do the callers and phasers behind it.  The rule: walk the item's output CIGAR.  An op with
// code M, = or X and length L is COMPARED: its L base pairs are classified by nm_core.hpp's pair rule (c1 the read's 4-bit code, c2 the
// reference byte's code in "=ACMGRSVTWYHKDBN", any other byte 15; a match iff c1 == 0, or c1 == c2 and c1 != 15) and the op is replaced by
// its maximal runs, '=' for matching and 'X' for mismatching pairs, in order.  Runs do not cross op boundaries (5M5= gives two runs at
// least), so no output op is longer than the op it came from; a compared op of length 0 yields nothing.  Every other op (I, D, N, S, H, P,
// codes 9-15) is copied as it stands, in its place.  Reference length, read length, pos, bin and the reference end do not change; the bases
// under X plus the I and D lengths are the item's NM, the X positions the mismatch letters of its MD text that do not stand behind '^'.
//   the walk is aln_walk.hpp's; the pieces are the 16-byte lines of the compared ops, and every other op is one piece, so the output order
//   is the piece order.  A compared piece yields a 16-bit mismatch mask (nm_piece_t<true>).  A lane writes the runs its piece CLOSES: the
//   run that enters the piece when its first base is of the other kind, a run for every change of kind inside it, and the run open at its
//   end when it is its op's last piece.  Of the run that enters it a lane needs the kind (the last base of the piece in front: one shuffle,
//   or the uniform carry for lane 0) and the length: md_seg_scan, where a piece of one kind that continues the entering run passes the
//   length on plus its bases and any other piece restarts the sum with its trailing run.  An op's first piece always starts a run and its
//   last piece always closes one, so nothing is open at the end of a step or of the item; the carry lives in uniform registers across the
//   trips of a step.
//   count and emit are one function (eqx_item<WRITE>): the count pass stores the item's op count (it needs no lengths), the 64-bit scan
//   of records_core.hpp makes item_eqx_off, the emit pass writes the ops as 4-byte stores at item_eqx_off[i] plus a wave scan of the lanes'
//   counts.  No LDS, no scratch.
// The same functions run under the CPU emulator (tests/emu/emu_eqx.cpp).
#pragma once
#include <plo_wave.hpp>
#include <stdint.h>

#include "md_core.hpp"

namespace plo {

struct DevEqx : AlnSrc {
    // count pass
    unsigned long long *item_len;  // [n_items] ops of the item's = / X CIGAR (0: not LIFTED, or refused)
    int *err_item;                 // [1] the lowest item whose CIGAR leaves the chromosome or the read (NM_NO_ITEM: none)
    // emit pass
    const unsigned long long *item_eqx_off;  // [n_items + 1] exclusive scan of item_len
    uint32_t *eqx_ops;
    unsigned *ticket;  // [1] next item (one word per pass)
};

constexpr uint32_t EQX_EQ = 7, EQX_X = 8;  // BAM_CEQUAL, BAM_CDIFF

// the item's slot: nothing is stored outside [out, out + room)
struct EqxSlot {
    uint32_t *out;
    unsigned long long room;
};
PLO_DEV void eqx_put(const EqxSlot &o, unsigned long long at, uint32_t op) {
    if (at < o.room) o.out[at] = op;
}

// the = / X CIGAR of item i by one wave.  WRITE false: its op count -> item_len[i]; true: its ops -> eqx_ops + item_eqx_off[i]
template <bool WRITE>
PLO_DEV void eqx_item(const DevBatch &bt, const DevWork &wk, const DevEqx &d, uint32_t i) {
    const int lane = wv::lane();
    if (!aln_lifted(wk, i)) {  // (wave-uniform, as every branch around a wave primitive below)
        if (!WRITE && lane == 0) d.item_len[i] = 0;
        return;
    }
    const AlnItem it = aln_open(bt, wk, d, i);
    if (!it.ok) {
        if (!WRITE) aln_refuse(d.err_item, d.item_len, i);
        return;
    }
    EqxSlot o = {nullptr, 0};
    if (WRITE) {
        o.out = d.eqx_ops + d.item_eqx_off[i];
        o.room = d.item_eqx_off[i + 1] - d.item_eqx_off[i];
    }
    unsigned long long rd_done = 0, rf_done = 0;  // (uniform) consumed by the steps so far
    unsigned long long done = 0;                  // (uniform) ops written so far
    for (uint32_t k = 0; k < it.n; k += 64) {
        const AlnStep st = aln_step(it, k, rd_done, rf_done);
        if (!st.ok) {
            if (!WRITE) aln_refuse(d.err_item, d.item_len, i);
            return;
        }
        // a compared op: its 16-byte lines (none when it is empty); any other op: one piece, itself
        const uint32_t np = !st.has ? 0u : !st.is_cmp ? 1u : st.len ? aln_lines(st.fa, st.len) : 0u;
        const uint32_t p_inc = (uint32_t)wv::scan_add((int)np);
        const uint32_t n_pieces = (uint32_t)wv::bcast_last((int)p_inc);
        uint32_t run_c = 0, kind_c = 0;  // (uniform) the run open behind the last trip's piece 63: its length and kind
        for (uint32_t p0 = 0; p0 < n_pieces; p0 += 64) {
            const uint32_t p = p0 + (uint32_t)lane;
            const AlnOp op = aln_find_op(st, np, p_inc, p);
            const bool act = p < n_pieces, cmp = act && (op.t == 0 || op.t == 7 || op.t == 8);
            const uint32_t j = p - op.first;
            const bool first = j == 0, last = j + 1 == op.np;
            // the piece's bases and their kinds (bit k: base k mismatches)
            uint32_t nb = 0, mask = 0;
            if (cmp) {
                const AlnSpan sp = aln_span(op.fa, op.len, j);
                nb = (uint32_t)(sp.e - sp.s);
                mask = nm_piece_t<true>(it.seq, it.seq_lo, it.seq_hi, op.fa, op.len, op.rd, j);
            }
            const uint32_t k_first = mask & 1u, k_last = cmp ? (mask >> (nb - 1)) & 1u : 0u;
            uint32_t k_in = wv::shfl(k_last, (lane - 1) & 63);  // the kind of the run that enters the piece
            if (lane == 0) k_in = kind_c;
            kind_c = wv::shfl(k_last, 63);
            const uint32_t chg = cmp ? (mask ^ (mask >> 1)) & ((1u << (nb - 1)) - 1u) : 0u;  // bit k: bases k and k + 1 differ in kind
            const bool closes_in = cmp && !first && k_first != k_in;
            const uint32_t n_out = !act ? 0u : !cmp ? 1u : (closes_in ? 1u : 0u) + (uint32_t)__builtin_popcount(chg) + (last ? 1u : 0u);
            const uint32_t o_inc = (uint32_t)wv::scan_add((int)n_out);
            if (WRITE) {
                // the length of the run that enters every lane's piece
                const bool ev = !cmp || first || closes_in || chg != 0;
                const uint32_t trail = !cmp ? 0u : chg ? nb - 1u - (31u - (uint32_t)wv::clz32(chg)) : nb;
                const unsigned long long incl = md_seg_scan(ev ? (1ull << 32) | trail : (unsigned long long)nb);
                unsigned long long excl = wv::shfl(incl, (lane - 1) & 63);
                if (lane == 0) excl = 0;
                const uint32_t run_in = (excl >> 32) ? (uint32_t)excl : run_c + (uint32_t)excl;
                const unsigned long long end = wv::shfl(incl, 63);
                run_c = (end >> 32) ? (uint32_t)end : run_c + (uint32_t)end;
                unsigned long long at = done + o_inc - n_out;
                if (act && !cmp) {
                    eqx_put(o, at, op.c);
                } else if (cmp) {
                    uint32_t run = first ? 0u : run_in, kind = first ? k_first : k_in, from = 0, m = chg;
                    if (closes_in) {
                        eqx_put(o, at++, (run << 4) | (EQX_EQ + kind));
                        run = 0;
                        kind = k_first;
                    }
                    while (m) {
                        const uint32_t b = (uint32_t)wv::ctz32(m) + 1u;
                        m &= m - 1;
                        eqx_put(o, at++, ((run + b - from) << 4) | (EQX_EQ + kind));
                        run = 0;
                        kind ^= 1u;
                        from = b;
                    }
                    if (last) eqx_put(o, at, ((run + nb - from) << 4) | (EQX_EQ + kind));
                }
            }
            done += (uint32_t)wv::bcast_last((int)o_inc);
        }
        rd_done = st.rd_end;
        rf_done = st.rf_end;
    }
    if (!WRITE && lane == 0) d.item_len[i] = done;
}

template <bool WRITE>
PLO_DEV void eqx_items(const DevBatch &bt, const DevWork &wk, const DevEqx &d) {
    aln_items(wk.n_items, d.ticket, [&](uint32_t i) { eqx_item<WRITE>(bt, wk, d, i); });
}

}  // namespace plo
