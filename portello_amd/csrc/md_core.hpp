// md_core.hpp -- MD:Z of the lifted records written on the device (plo_md_dev): the text samtools calmd writes (bam_md.c,
// bam_fillmd1_core), restated.  A counter u of matched bases starts at 0.  M / = / X go base by base, and the match / mismatch decision of
// a pair is nm_core.hpp's (c1 == 0, or the reference byte is "=ACMGRSVTWYHKDBN"[c1] and c1 != 15): a match does ++u; a mismatch writes u in
// decimal (also 0), then the reference letter, and sets u = 0.  A D of length > 0 writes u (also 0), '^', its reference letters, u = 0.
// I, S, N, H, P write nothing and keep u (I and S advance the read, N the reference).  At the end u is written: the text of a LIFTED item
// is never empty.  Ops of length 0 are skipped: calmd would write an empty '^' for 0D, the lift never emits one.
// The reference letter is the chrom_seq byte: A..Z as it is, a..z upper-cased (calmd's toupper), any other byte 'N' -- the text stays
// inside [0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)* whatever the index holds.
//   the walk is aln_walk.hpp's; the pieces are the 16-byte lines of the M / = / X and of the D ops.
//   A compared piece yields a 16-bit mismatch mask (nm_piece_t<true>): its events.  The matches in
//   front of its first event and behind its last are its leading and trailing count; a D's first piece is an event with both counts 0
//   (it carries u and '^'), every D piece copies its letters.  A segmented scan over the lanes (a set flag cuts the sum) hands every lane
//   the u its first event closes, a second scan over the lanes' byte counts their offsets; u and the bytes written are carried, uniform,
//   across trips and steps, and the run open at the item's end is closed by the last number.
//   count and emit are one function (md_item<WRITE>): the count pass stores the item's length, the 64-bit scan of records_core.hpp makes
//   item_md_off, the emit pass writes the bytes -- with byte stores: a piece without an event writes nothing, and most pieces have none.
// The same functions run under the CPU emulator (tests/emu/emu_md.cpp).
#pragma once
#include <plo_wave.hpp>
#include <stdint.h>

#include "nm_core.hpp"

namespace plo {

struct DevMd : AlnSrc {
    // count pass
    unsigned long long *item_len;  // [n_items] bytes of the item's text (0: not LIFTED, or refused)
    int *err_item;                 // [1] the lowest item whose CIGAR leaves the chromosome or the read (NM_NO_ITEM: none)
    // emit pass
    const unsigned long long *item_md_off;  // [n_items + 1] exclusive scan of item_len
    uint8_t *md_text;
    unsigned *ticket;  // [1] next item (one word per pass)
};

PLO_DEV uint32_t md_digits(uint32_t v) {
    return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u : v < 10000000u ? 7u : v < 100000000u ? 8u : v < 1000000000u ? 9u : 10u;
}
PLO_DEV uint8_t md_letter(unsigned b) { return b - 'A' < 26u ? (uint8_t)b : b - 'a' < 26u ? (uint8_t)(b - 32u) : (uint8_t)'N'; }

// the item's slot: nothing is stored outside [out, out + room)
struct MdSlot {
    uint8_t *out;
    unsigned long long room;
};
PLO_DEV void md_put(const MdSlot &o, unsigned long long at, uint8_t b) {
    if (at < o.room) o.out[at] = b;
}
PLO_DEV unsigned long long md_put_dec(const MdSlot &o, unsigned long long at, uint32_t v) {
    const uint32_t n = md_digits(v);
    for (uint32_t k = n; k > 0; --k) {
        md_put(o, at + k - 1, (uint8_t)('0' + v % 10u));
        v /= 10u;
    }
    return at + n;
}

// the events of a compared piece: `mask` over its bases, u_in matches open in front of it, rf its reference bytes.  -> bytes; WRITE stores them at `at`
template <bool WRITE>
PLO_DEV uint32_t md_events(uint32_t mask, uint32_t u_in, const uint8_t *rf, const MdSlot &o, unsigned long long at) {
    uint32_t nb = 0, uu = u_in;
    int last = -1;
    while (mask) {
        const int k = wv::ctz32(mask);
        mask &= mask - 1;
        uu += (uint32_t)(k - last - 1);
        if (WRITE) {
            at = md_put_dec(o, at, uu);
            md_put(o, at++, md_letter(rf[k]));
        } else {
            nb += md_digits(uu) + 1u;
        }
        uu = 0;
        last = k;
    }
    return nb;
}

// inclusive segmented sum across the wave: bit 32 of x is the lane's flag, the low half its value; a lane without a flag adds what the lanes
// in front of it carry (back to the nearest flag, whose value starts the sum) and takes over their flag
PLO_DEV unsigned long long md_seg_scan(unsigned long long x) {
    const int l = wv::lane();
    for (int s = 1; s < 64; s <<= 1) {
        const unsigned long long t = wv::shfl(x, (l - s) & 63);
        if (l >= s && !(x >> 32)) x += t;
    }
    return x;
}

// the text of item i by one wave.  WRITE false: its length -> item_len[i]; true: its bytes -> md_text + item_md_off[i]
template <bool WRITE>
PLO_DEV void md_item(const DevBatch &bt, const DevWork &wk, const DevMd &d, uint32_t i) {
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
    MdSlot o = {nullptr, 0};
    if (WRITE) {
        o.out = d.md_text + d.item_md_off[i];
        o.room = d.item_md_off[i + 1] - d.item_md_off[i];
    }
    unsigned long long rd_done = 0, rf_done = 0;  // (uniform) consumed by the steps so far
    uint32_t u = 0;                               // (uniform) the matches open behind the last event
    unsigned long long done = 0;                  // (uniform) bytes of the text so far
    for (uint32_t k = 0; k < it.n; k += 64) {
        const AlnStep st = aln_step(it, k, rd_done, rf_done);
        if (!st.ok) {
            if (!WRITE) aln_refuse(d.err_item, d.item_len, i);
            return;
        }
        const bool is_del = st.has && st.t == 2;
        const uint32_t np = (st.is_cmp || is_del) && st.len ? aln_lines(st.fa, st.len) : 0u;
        const uint32_t p_inc = (uint32_t)wv::scan_add((int)np);
        const uint32_t n_pieces = (uint32_t)wv::bcast_last((int)p_inc);
        for (uint32_t p0 = 0; p0 < n_pieces; p0 += 64) {
            const uint32_t p = p0 + (uint32_t)lane;
            const AlnOp op = aln_find_op(st, np, p_inc, p);
            const bool o_del = op.t == 2;
            const bool act = p < n_pieces;
            const uint32_t j = p - op.first;
            const AlnSpan sp = aln_span(op.fa, op.len, j);  // the piece's reference bytes
            const uint32_t nb_ref = act ? (uint32_t)(sp.e - sp.s) : 0u;
            const uint8_t *rf = (const uint8_t *)sp.s;
            uint32_t mask = 0;
            if (act && !o_del) mask = nm_piece_t<true>(it.seq, it.seq_lo, it.seq_hi, op.fa, op.len, op.rd, j);
            const bool ev = act && (o_del || mask != 0);
            const uint32_t lead = !act || o_del ? 0u : mask ? (uint32_t)wv::ctz32(mask) : nb_ref;
            const uint32_t trail = mask ? nb_ref - 1u - (31u - (uint32_t)wv::clz32(mask)) : 0u;
            // the u in front of every lane's piece
            const unsigned long long incl = md_seg_scan(ev ? (1ull << 32) | trail : (unsigned long long)lead);
            unsigned long long excl = wv::shfl(incl, (lane - 1) & 63);
            if (lane == 0) excl = 0;
            const uint32_t u_in = (excl >> 32) ? (uint32_t)excl : u + (uint32_t)excl;
            const unsigned long long last = wv::shfl(incl, 63);
            u = (last >> 32) ? (uint32_t)last : u + (uint32_t)last;
            // its bytes, and where they go
            const bool head = act && o_del && j == 0;  // a D's first piece: u and '^'
            uint32_t nb = 0;
            if (act && o_del) nb = (head ? md_digits(u_in) + 1u : 0u) + nb_ref;
            else if (mask) nb = md_events<false>(mask, u_in, rf, o, 0);
            const uint32_t b_inc = (uint32_t)wv::scan_add((int)nb);
            if (WRITE) {
                unsigned long long at = done + b_inc - nb;
                if (act && o_del) {
                    if (head) {
                        at = md_put_dec(o, at, u_in);
                        md_put(o, at++, (uint8_t)'^');
                    }
                    for (uint32_t x = 0; x < nb_ref; ++x) md_put(o, at + x, md_letter(rf[x]));
                } else if (mask) {
                    md_events<true>(mask, u_in, rf, o, at);
                }
            }
            done += (uint32_t)wv::bcast_last((int)b_inc);
        }
        rd_done = st.rd_end;
        rf_done = st.rf_end;
    }
    if (lane == 0) {
        if (WRITE) md_put_dec(o, done, u);
        else d.item_len[i] = done + md_digits(u);
    }
}

template <bool WRITE>
PLO_DEV void md_items(const DevBatch &bt, const DevWork &wk, const DevMd &d) {
    aln_items(wk.n_items, d.ticket, [&](uint32_t i) { md_item<WRITE>(bt, wk, d, i); });
}

}  // namespace plo
