// nm_core.hpp -- NM:i of the lifted records computed on the device (plo_nm_dev): the edit distance of an output record against the
// reference, by the rule of samtools calmd (bam_md.c).  M / = / X compare base by base: with c1 the read's 4-bit code and c2 the
// reference byte's code in "=ACMGRSVTWYHKDBN" (any other byte: 15) the pair matches iff c1 == 0, or c1 == c2 and c1 != 15; every other pair
// adds 1 (N against N is a mismatch, R against R a match, a read '=' matches anything).  I adds its length and advances the read, D adds
// its length and advances the reference, N advances the reference, S the read, H and P do nothing.
// Since the table is one-to-one, "c1 == c2 and c1 != 15" is "the reference byte is table[c1]" for c1 in 1..14: the read's codes are
// turned into the characters they stand for (two v_perm_b32 per four bases) and compared with the reference bytes as they lie.
//   the walk is aln_walk.hpp's; a piece is one 16-byte line of an M / = / X op, and the pair rule on a piece is this file's (nm_piece_t):
//   a whole piece: 16 aligned bytes of the reference, two aligned 8-byte loads of the read's nibbles (realigned by a funnel shift
//   of whole bytes; an odd read position takes the low nibbles first), sixteen bases compared in four dwords.
//   a part piece (head and tail of an op, any op below 16 bases), and a whole one whose 8-byte words would reach outside the read's
//   bases: base by base -- nothing outside [seq, seq + (l_seq + 1) / 2) or the chromosome is read.
// The same functions run under the CPU emulator (tests/emu/emu_nm.cpp).
#pragma once
#include <plo_wave.hpp>
#include <stdint.h>

#include "aln_walk.hpp"

namespace plo {

struct DevNm : AlnSrc {
    // output
    uint32_t *item_nm;              // [n_items]
    unsigned long long *n_cmp;      // [1] bases compared, whole batch
    int *err_item;                  // [1] the lowest item whose CIGAR leaves the chromosome or the read (NM_NO_ITEM: none)
    unsigned *ticket;               // [1] next item
};

// the four bases whose codes are the bytes of `cd` against the four reference bytes `rf`: 0x80 in byte k where pair k mismatches
PLO_DEV uint32_t nm_mismask4(uint32_t cd, uint32_t rf) {
    const uint32_t T0 = 0x4D43413Du, T1 = 0x56535247u, T2 = 0x48595754u, T3 = 0x4E42444Bu;  // "=ACM" "GRSV" "TWYH" "KDBN"
    const uint32_t idx = cd & 0x07070707u;
    const uint32_t lo = wv::perm_bytes(T1, T0, idx), hi = wv::perm_bytes(T3, T2, idx);
    const uint32_t up = ((cd >> 3) & 0x01010101u) * 0xffu;
    const uint32_t x = ((hi & up) | (lo & ~up)) ^ rf;
    const uint32_t differs = (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
    const uint32_t is15 = ((cd + 0x01010101u) & 0x10101010u) << 3;
    const uint32_t not0 = (cd + 0x7f7f7f7fu) & 0x80808080u;
    return (differs | is15) & not0;
}
// their number
PLO_DEV uint32_t nm_mismatch4(uint32_t cd, uint32_t rf) { return (uint32_t)__builtin_popcount(nm_mismask4(cd, rf)); }
// the 0x80 of byte k as bit k (the partial products of the multiplication meet in no bit)
PLO_DEV uint32_t nm_mask_bits(uint32_t m) { return ((m >> 7) * 0x10204080u) >> 28; }

// one pair, the rule as it is stated
PLO_DEV uint32_t nm_mismatch1(unsigned c1, unsigned ch) {
    if (c1 == 0) return 0;
    if (c1 == 15) return 1;
    const unsigned long long TLO = 0x565352474D43413Dull, THI = 0x4E42444B48595754ull;
    return (unsigned)((((c1 & 8u) ? THI : TLO) >> (8u * (c1 & 7u))) & 0xffu) != ch;
}

// piece j of a match op: reference bytes [fa, fa + len) (an address), read bases from rd on; `seq` = the record's 4-bit bases,
// [seq_lo, seq_hi) their addresses.  MASK false: the piece's mismatches (k_nm); true: bit k set where its base k mismatches (md_core.hpp)
template <bool MASK>
PLO_DEV uint32_t nm_piece_t(const uint8_t *seq, uintptr_t seq_lo, uintptr_t seq_hi, uintptr_t fa, uint32_t len, unsigned long long rd, uint32_t j) {
    const AlnSpan sp = aln_span(fa, len, j);
    const uintptr_t s = sp.s, e = sp.e;
    const unsigned long long rp = rd + (unsigned long long)(s - fa);
    if (e - s == 16) {
        const uintptr_t b = seq_lo + (uintptr_t)(rp >> 1), w = b & ~(uintptr_t)7;
        if (w >= seq_lo && w + 16 <= seq_hi) {
            const uint64_t q0 = *(const PLO_GLOBAL uint64_t *)w, q1 = *(const PLO_GLOBAL uint64_t *)(w + 8);
            const uint64_t r0 = *(const PLO_GLOBAL uint64_t *)s, r1 = *(const PLO_GLOBAL uint64_t *)(s + 8);
            const unsigned sh = 8u * (unsigned)(b & 7u);
            const uint64_t w0 = sh ? (q0 >> sh) | (q1 << (64u - sh)) : q0;
            const uint64_t w1 = sh == 56u ? q1 : (q0 >> (sh + 8u)) | (q1 << (56u - sh));  // one byte on
            const uint64_t NIB = 0x0f0f0f0f0f0f0f0full;
            const uint64_t hi0 = (w0 >> 4) & NIB, lo0 = w0 & NIB, hi1 = (w1 >> 4) & NIB;
            // bases 2k and 2k + 1 of the piece are byte k of a and of b
            const bool odd = (rp & 1u) != 0;
            const uint64_t a = odd ? lo0 : hi0, bb = odd ? hi1 : lo0;
            const uint32_t a0 = (uint32_t)a, a1 = (uint32_t)(a >> 32), b0 = (uint32_t)bb, b1 = (uint32_t)(bb >> 32);
            const uint32_t c0 = wv::perm_bytes(a0, b0, 0x01050004u), c1 = wv::perm_bytes(a0, b0, 0x03070206u);
            const uint32_t c2 = wv::perm_bytes(a1, b1, 0x01050004u), c3 = wv::perm_bytes(a1, b1, 0x03070206u);
            if (MASK)
                return nm_mask_bits(nm_mismask4(c0, (uint32_t)r0)) | (nm_mask_bits(nm_mismask4(c1, (uint32_t)(r0 >> 32))) << 4) |
                       (nm_mask_bits(nm_mismask4(c2, (uint32_t)r1)) << 8) | (nm_mask_bits(nm_mismask4(c3, (uint32_t)(r1 >> 32))) << 12);
            return nm_mismatch4(c0, (uint32_t)r0) + nm_mismatch4(c1, (uint32_t)(r0 >> 32)) + nm_mismatch4(c2, (uint32_t)r1) + nm_mismatch4(c3, (uint32_t)(r1 >> 32));
        }
    }
    uint32_t n = 0;
    const uint8_t *rf = (const uint8_t *)s;
    for (uint32_t k = 0; k < (uint32_t)(e - s); ++k) {
        const unsigned long long p = rp + k;
        const unsigned byte = seq[p >> 1];
        const uint32_t m = nm_mismatch1((p & 1u) ? (byte & 15u) : (byte >> 4), rf[k]);
        n += MASK ? m << k : m;
    }
    return n;
}
PLO_DEV uint32_t nm_piece(const uint8_t *seq, uintptr_t seq_lo, uintptr_t seq_hi, uintptr_t fa, uint32_t len, unsigned long long rd, uint32_t j) {
    return nm_piece_t<false>(seq, seq_lo, seq_hi, fa, len, rd, j);
}

// NM of item i by one wave; cmp (per lane) gathers the bases compared
PLO_DEV void nm_item(const DevBatch &bt, const DevWork &wk, const DevNm &d, uint32_t i, unsigned long long &cmp) {
    const int lane = wv::lane();
    if (!aln_lifted(wk, i)) {  // (wave-uniform, as every branch around a wave primitive below)
        if (lane == 0) d.item_nm[i] = 0;
        return;
    }
    const AlnItem it = aln_open(bt, wk, d, i);
    if (!it.ok) return aln_refuse(d.err_item, d.item_nm, i);
    unsigned long long rd_done = 0, rf_done = 0;  // (uniform) consumed by the steps so far
    uint32_t nm = 0;                              // (per lane)
    for (uint32_t k = 0; k < it.n; k += 64) {
        const AlnStep st = aln_step(it, k, rd_done, rf_done);
        if (!st.ok) return aln_refuse(d.err_item, d.item_nm, i);
        if (st.has && (st.t == 1 || st.t == 2)) nm += st.len;
        const uint32_t np = st.is_cmp && st.len ? aln_lines(st.fa, st.len) : 0u;
        const uint32_t p_inc = (uint32_t)wv::scan_add((int)np);
        const uint32_t n_pieces = (uint32_t)wv::bcast_last((int)p_inc);
        if (st.is_cmp) cmp += st.len;
        for (uint32_t p0 = 0; p0 < n_pieces; p0 += 64) {
            const uint32_t p = p0 + (uint32_t)lane;
            const AlnOp o = aln_find_op(st, np, p_inc, p);
            if (p < n_pieces) nm += nm_piece(it.seq, it.seq_lo, it.seq_hi, o.fa, o.len, o.rd, p - o.first);
        }
        rd_done = st.rd_end;
        rf_done = st.rf_end;
    }
    const uint32_t total = (uint32_t)wv::reduce_add((int)nm);
    if (lane == 0) d.item_nm[i] = total;
}

PLO_DEV void nm_items(const DevBatch &bt, const DevWork &wk, const DevNm &d) {
    unsigned long long cmp = 0;
    aln_items(wk.n_items, d.ticket, [&](uint32_t i) { nm_item(bt, wk, d, i, cmp); });
    cmp = wv::shfl(wave_scan_incl_u64(cmp), 63);
    if (wv::lane() == 0 && cmp) wv::atomic_add_global(d.n_cmp, cmp);
}

}  // namespace plo
