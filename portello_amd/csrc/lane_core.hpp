// lane_core.hpp -- the lane-per-item formulation of the liftover pipeline: 64 items per wave, one LANE per item.
//
// lift_core.hpp spreads the ops of a tile over the lanes and recasts the reference's sequential state as wave scans: ~26
// wave-instructions per input op, a dozen passes over the op stream.  HiFi read->contig CIGARs have ~30 ops, and 64 of them fit
// a wave's LDS slice comfortably -- so here every lane walks ITS item sequentially, exactly as the reference's loops do, and the
// wave only cooperates where items meet: LDS allocation (one add-scan), output allocation (one add-scan), loop bounds (ballots).
// What makes that cheap on CDNA4, where a straightforward per-lane transliteration is not (round 1: 36 KB of LDS per wave, i.e.
// 4 waves per CU; a memory round trip per indel cluster in the middle of the walk):
//   * one compact LDS region per item (weight + slack dwords, ~180 B), used IN PLACE by every stage: the liftover reads its
//     input at the region's upper end and writes its output from the bottom -- pieces <= ops + 2 per block crossed, and the
//     gap in front of the input is exactly that allowance; 64 regions ~ 11 KB per wave -> 12-13 waves per CU;
//   * clean_up_cigar_edge_indels + compress_cigar as a STREAMING writer (LaneOut): leading edge and run merging while the ops
//     are produced, the (short) trailing edge fixed in place afterwards -- no extra passes, no second buffer;
//   * the liftover as one FLAT loop over (op x block) pieces with a three-entry cursor into the block map (current block, next
//     block, the one after it in flight), so that a crossing costs no search and no wait;
//   * the left shift's homology probes ISSUED at the end of an indel cluster and CONSUMED at the next one (the emission of a
//     cluster is deferred until then): the HBM round trip runs under the walk of the following ops.
// Items whose region overflows go to the wave-cooperative code of lift_core.hpp (retry list), which remains the general path.  Items
// too heavy for an LDS region: the same code with the region in global memory behind two small LDS windows per lane (lane_tile<SP, WIN>,
// "Heavy items" below) when a batch has many of them, else the wave-cooperative kernels (large-item lists).
//
// All citations are relative to /root/reference.
#pragma once
#include <plo_wave.hpp>
#include <stdint.h>

#include <type_traits>
#ifdef PLO_EMULATOR
#include <stdio.h>
#include <stdlib.h>
#endif

#include "lift_core.hpp"

#ifdef PLO_EMULATOR
#define PLO_MARK(s)
#else
#define PLO_MARK(s) asm volatile("; " s)  // a comment in the ISA listing (tools: hipcc -S), no code
#endif

// PLO_SHIFT_LOCKSTEP: the shift stage's lockstep loop for items whose ops alternate match / lone indel (lane_tile, "LEFT SHIFT,
// clean items"); 0 compiles it out, DevWork::lane_lockstep_off switches it off at run time.
#ifndef PLO_SHIFT_LOCKSTEP
#define PLO_SHIFT_LOCKSTEP 1
#endif

namespace plo {

// (plo_safe_words, enumerate.hpp: where the lanes without a usable probe window point their unconditional loads)


// -------------------------------------------------------------------------------------------------------------------
// Streaming clean_up_cigar_edge_indels + compress_cigar (lib/rust-vc-utils/src/bam_utils/cigar/mod.rs:265-291, 204-228).
// Ops are pushed in order; the writer applies the LEADING edge rule on the fly (before the first alignment match: D -> S(0),
// its length added to the position shift; I -> S), drops zero-length ops and merges equal neighbours (accumulator = last_elem,
// starting as Match(0), :206).  lane_out_finish() flushes the accumulator and applies the TRAILING edge rule to the ops behind
// the last match (they are few), merging again.  Merging before the trailing rule instead of after it gives the same result:
// the rule maps every I of the tail to S and removes every D of the tail, whatever runs they were merged into.
// "The last match op" is tracked as the last match op WRITTEN.  No stage emits a zero-length match op, but the simplify stage
// copies what it is given: a zero-length M / = / X in its input (raw CIGARs, stage subsets without the liftover) would mark an
// edge without being written -- such an item is handed to the wave-cooperative code (`ovf`).
//
// Code shape: the per-lane state is integers and lane_push() is straight-line code (selects, one predicated LDS store).
// Lane-divergent branches around it cost more than the work they skip: every boolean that is live across a divergent join
// becomes a lane mask in scalar registers that the compiler merges with three scalar instructions per join (the first version
// of this file spent more scalar than vector instructions).
// -------------------------------------------------------------------------------------------------------------------
#ifdef PLO_EMULATOR
struct __attribute__((packed, aligned(4))) Ops4 {
    uint32_t x, y, z, w;
};
#else
typedef uint32_t Ops4 __attribute__((ext_vector_type(4), aligned(4)));  // four CIGAR ops: one 16-byte access at any 4-byte address
#endif
struct LaneOut {
    uint32_t *R = nullptr;  // the lane's region
    int no = 0;             // ops written
    uint32_t acc = 0;       // the open run, (len << 4) | type; starts as Match(0)
    int lead_shift = 0;
    bool seen_m = false;
    bool pairs = false;     // two neighbouring I / D ops were written: an indel cluster of more than one op
    bool ovf = false;       // a write would have passed `wlim`
    // H16 (16-bit ops in the region, below): `no` counts HALFWORDS, `extra` those of them that continue an op longer than H16_MAX
    // (counted where they are written, which is rare: the ops written are no - extra)
    uint16_t *H = nullptr;
    int extra = 0;
};
PLO_DEV int wrap_add(int a, int b) { return (int)((unsigned)a + (unsigned)b); }
PLO_DEV bool b_is_match(int t) { return ((0x181u >> t) & 1u) != 0u; }   // M = X
PLO_DEV bool b_is_indel(int t) { return (unsigned)(t - 1) < 2u; }        // I D
PLO_DEV bool b_ref_cons(int t) { return ((0x18Du >> t) & 1u) != 0u; }   // M D N = X
PLO_DEV bool b_read_cons(int t) { return ((0x1B3u >> t) & 1u) != 0u; }  // M I S H = X

// -------------------------------------------------------------------------------------------------------------------
// H16: the light-item kernel's regions hold 16-BIT ops (round 6; VERDICT r4 / r5 asked for the format itself instead of a proxy).
// A halfword is (len << 3) | type with the BAM op codes 0 .. 6 (M I D N S H P) -- after LOAD has merged = / X / M runs into M, which it
// does whenever the liftover runs (batches of other stage sets keep the 32-bit regions), no other code occurs -- and len <= H16_MAX = 8 191.
// A longer op is stored as up to H16_CHUNKS neighbouring halfwords of its type (the first ones full): every stage treats equal
// neighbours as the reference treats their sum -- the shift builder and the simplify stage add up the members of a cluster and the
// match bases between clusters op by op, the liftover cuts ops into pieces anyway and its writer merges what comes of neighbouring
// pieces -- and the output copy sums them up again.  Beyond H16_CHUNKS halfwords (65 528 bases in one op: no HiFi read's clip) the item takes the retry list.
// In registers ops stay (len << 4) | type.  What it buys: a region of ~90 bytes instead of ~175, i.e. twice the items, or four times
// the staged block-map entries and wider sort windows, in the same LDS slice.
// -------------------------------------------------------------------------------------------------------------------
constexpr int H16_MAX = 8191, H16_CHUNKS = 8;
constexpr int H16_ALLOW = 4;  // halfwords a region has for the extra chunks of its long ops (more: the writer's / LOAD's overflow check -> retry list)
PLO_DEV uint32_t h16_dec(uint32_t h) { return ((h >> 3) << 4) | (h & 7u); }
PLO_DEV uint32_t h16_enc(int t, uint32_t len) { return (len << 3) | (uint32_t)t; }

// the open run `o.acc` goes out for the lanes `flush` (H16: in chunks); `wlim`: first index that must not be written
template <int ST, bool H16>
PLO_DEV void lane_flush(LaneOut &o, bool flush, int wlim) {
    const int at = (int)(o.acc & 15u);
    if constexpr (!H16) {
        const bool ok = o.no < wlim;
        if (flush & ok) o.R[o.no * ST] = o.acc;
        o.ovf = o.ovf | (flush & !ok);
        o.no += flush ? 1 : 0;
    } else {
        static_assert(ST == 1, "H16 regions are lane-contiguous");
        const uint32_t len = o.acc >> 4;
        const bool ok = o.no < wlim;
        if (flush & ok) o.H[o.no] = (uint16_t)h16_enc(at, len < (uint32_t)H16_MAX ? len : (uint32_t)H16_MAX);
        o.ovf = o.ovf | (flush & !ok);
        o.no += flush ? 1 : 0;
        const bool big = flush & (len > (uint32_t)H16_MAX);
        if (wv::ballot(big) != 0ull) {  // (three runs in a thousand)
            uint32_t rest = big ? len - (uint32_t)H16_MAX : 0u;
#pragma unroll
            for (int c = 1; c < H16_CHUNKS; ++c) {
                const bool more = rest > 0u;
                const uint32_t part = rest < (uint32_t)H16_MAX ? rest : (uint32_t)H16_MAX;
                const bool okc = o.no < wlim;
                if (more & okc) o.H[o.no] = (uint16_t)h16_enc(at, part);
                o.ovf = o.ovf | (more & !okc);
                o.no += more ? 1 : 0;
                o.extra += more ? 1 : 0;
                rest -= part;
            }
            o.ovf = o.ovf | (rest > 0u);
        }
    }
}
// Flags are `bool`s combined with & | ^ (no short-circuit: the code must stay one basic block).
// `wlim`: first index that must not be written (the reader's position when the region is used in place).  PAD: the stream may
// hold Pad ops (absent from compress_cigar's summing pattern, :210-212: a Pad following a Pad adds nothing).
// ST: distance of neighbouring ops in o.R (1; 64: the write window of a heavy item, whose writer stops for good at the first op
// that does not fit -- its window indices mean nothing from there).
template <bool PAD = true, int ST = 1, bool H16 = false>
PLO_DEV void lane_push(LaneOut &o, bool on, int t, int L, int wlim) {
    if constexpr (ST != 1) on = on & !o.ovf;
    const bool lead = on & !o.seen_m;
    const bool drop_d = lead & (t == OP_D);
    o.lead_shift += drop_d ? L : 0;
    t = (lead & (t == OP_I)) ? (int)OP_S : t;
    o.seen_m = o.seen_m | (on & b_is_match(t));
    const bool live = on & !drop_d & (L > 0);
    const int at = (int)(o.acc & 15u);
    const bool same = live & (t == at);
    const bool flush = live & !same & (o.acc >= 16u);
    o.pairs = o.pairs | (flush & b_is_indel(at) & b_is_indel(t));
    lane_flush<ST, H16>(o, flush, wlim);
    const uint32_t add = (PAD && t == OP_P) ? 0u : ((uint32_t)L << 4);
    o.acc = same ? o.acc + add : (live ? mk_op(t, L) : o.acc);
}
// wave-uniform call (the loops are bounded by ballots); `on`: lanes that own a writer
template <bool H16 = false>
PLO_DEV void lane_out_finish(LaneOut &o, bool on, int wlim) {
    lane_flush<1, H16>(o, on & (o.acc >= 16u), wlim);
    // trailing edge: the ops behind the last alignment match (if none was written, everything went through the leading rule
    // already).  They are few.
    const bool fix0 = on & !o.ovf & o.seen_m;
    if constexpr (H16) {
        // found by walking back from the end (the chunks of a long match are matches); the tail then goes through a second writer from
        // there (edge rule: I -> S, D dropped; merging and chunking as everywhere): it shrinks or keeps the tail, so it never passes
        // the position it reads at
        int lm = o.no - 1;
        {
            bool look = fix0 & (lm >= 0);
            while (wv::ballot(look) != 0ull) {
                const uint32_t c = o.H[look ? lm : 0];
                const bool hit = look & b_is_match((int)(c & 7u));
                look = look & !hit & (lm > 0);
                lm -= (look) ? 1 : 0;
            }
        }
        const bool fix = fix0 & (lm + 1 < o.no);
        LaneOut o2;
        o2.H = o.H;
        o2.no = lm + 1;
        o2.seen_m = true;
        int i = lm + 1, cont = 0, prev_t = -1;  // cont: halfwords of the old tail that continue an op
        while (wv::ballot(fix & (i < o.no)) != 0ull) {
            const bool act = fix & (i < o.no);
            const uint32_t c = h16_dec(o.H[act ? i : 0]);
            int t = op_type(c);
            const int L = op_len(c);
            i += act ? 1 : 0;
            cont += (act & (t == prev_t)) ? 1 : 0;
            prev_t = act ? t : prev_t;
            const bool keep = act & (t != OP_D);  // a trailing D becomes S(0), which compress_cigar drops
            t = (t == OP_I) ? (int)OP_S : t;
            lane_push<true, 1, true>(o2, keep, t, L, i);
        }
        lane_flush<1, true>(o2, fix & (o2.acc >= 16u), o.no);
        o.no = fix ? o2.no : o.no;
        o.extra = fix ? o.extra - cont + o2.extra : o.extra;
    } else {
        // found by walking back from the end
        int lm = o.no - 1;
        {
            bool look = fix0 & (lm >= 0);
            while (wv::ballot(look) != 0ull) {
                const uint32_t c = o.R[look ? lm : 0];
                const bool hit = look & b_is_match(op_type(c));
                look = look & !hit & (lm > 0);
                lm -= (look) ? 1 : 0;
                // (a lane leaves the loop on its last match, or at index 0 without one -- which seen_m rules out)
            }
        }
        const bool fix = fix0 & (lm + 1 < o.no);
        int i = lm + 1, w = lm + 1;
        uint32_t run = 0;  // open run of the rewritten tail (0: none)
        while (wv::ballot(fix & (i < o.no)) != 0ull) {
            const bool act = fix & (i < o.no);
            const uint32_t c = o.R[act ? i : 0];
            int t = op_type(c);
            const int L = op_len(c);
            i += act ? 1 : 0;
            const bool keep = act & (t != OP_D);  // a trailing D becomes S(0), which compress_cigar drops
            t = (t == OP_I) ? (int)OP_S : t;
            const bool same = keep & (run >= 16u) & (t == (int)(run & 15u));
            const bool flush = keep & !same & (run >= 16u);
            if (flush) o.R[w] = run;
            w += flush ? 1 : 0;
            const uint32_t add = (t == OP_P) ? 0u : ((uint32_t)L << 4);
            run = same ? run + add : (keep ? mk_op(t, L) : run);
        }
        {
            const bool flush = fix & (run >= 16u);
            if (flush) o.R[w] = run;
            w += flush ? 1 : 0;
            o.no = fix ? w : o.no;
        }
    }
}

// -------------------------------------------------------------------------------------------------------------------
// xor_window16 (lift_core.hpp) in two halves for the dense sequence formats: the loads now, the decode later.
// -------------------------------------------------------------------------------------------------------------------
// (the words stay in the shape they are loaded in -- a 16-byte vector and a fifth word per side -- until xw16_decode: loop-carried
// registers of another shape would be filled by copies from the load's destination, i.e. behind a wait for the load)
struct XW16 {
    Ops4 r4, q4;
    uint32_t r1, q1;
    int rsh, qsh, jmin;
};
// Straight-line: every lane loads (lanes without a usable window from the start of `safe`, which must be readable for 20 bytes),
// and nothing looks at the loaded words before xw16_decode -- a select on them would put the wait for the round trip right here.
// Returns whether the lane's window is usable.
// Sparse bases (PLO_SEQ_BAM4_SPARSE): the granule look-up (sparse_locate, lift_core.hpp) comes first -- the header pair(s) of the
// window's granules, three words of the read's own header line, which its earlier probes have brought into the caches -- and the
// window's loads follow at the granule's place; `miss`: a granule of the window is absent (the item ends PLO_ITEM_NEED_BASES).
PLO_DEV bool xw16_issue(bool on, const uint8_t *ref, int ref_len, int r0, const ReadSeq &rd, int q0, const uint8_t *safe, XW16 &w, bool &miss) {
    bool ok = on & (r0 >= 0) & (q0 >= 0) & (q0 <= rd.len - 16);
    const int rsh = (int)(((unsigned)(uintptr_t)ref + (unsigned)r0) & 3u);
    ok = ok & (r0 - rsh >= 0) & (r0 - rsh <= ref_len - 20);
    const int jmin = rd.flip ? rd.len - q0 - 16 : q0;
    const bool bam4 = rd.fmt != PLO_SEQ_ASCII;
    int b0 = bam4 ? (jmin >> 1) : jmin;
    miss = false;
    if (rd.fmt == PLO_SEQ_BAM4_SPARSE) {
        const int j0 = ok ? jmin : 0, j1 = ok ? jmin + 15 : 0;
        const int g0 = j0 >> 5, g1 = j1 >> 5;
        const PLO_GLOBAL uint32_t *hdr = (const PLO_GLOBAL uint32_t *)(ok ? rd.p : safe);
        const uint32_t m0 = hdr[2 * (g0 >> 5)], rk0 = hdr[2 * (g0 >> 5) + 1], m1 = hdr[2 * (g1 >> 5)];
        const bool present = (((m0 >> (g0 & 31)) & (m1 >> (g1 & 31))) & 1u) != 0u;
        const unsigned rank = rk0 + (unsigned)__builtin_popcount(m0 & ((1u << (g0 & 31)) - 1u));
        const long long off = (long long)rd.data + (long long)rank * 16 + ((j0 >> 1) & 15);
        const bool bad = !present | (rank > 0x3ffffffu) | (off + (g1 - g0) * 16 + 20 > (long long)rd.hi);
        miss = ok & bad;
        ok = ok & !bad;
        b0 = (int)off;
    }
    const int qsh = (int)(((unsigned)(uintptr_t)rd.p + (unsigned)b0) & 3u);
    ok = ok & (b0 - qsh >= rd.lo) & (b0 - qsh + 20 <= rd.hi);  // five words, whatever the format needs
#ifdef PLO_EXP_PROBE_NOMEM  // timing experiment (tools/): every probe reads the same 32 bytes -- what do the probes' HBM round trips cost?  (results are wrong)
    const PLO_GLOBAL uint32_t *pr = (const PLO_GLOBAL uint32_t *)safe;
    const PLO_GLOBAL uint32_t *pq = (const PLO_GLOBAL uint32_t *)safe;
#else
    const PLO_GLOBAL uint32_t *pr = (const PLO_GLOBAL uint32_t *)(ok ? ref + (r0 - rsh) : safe);
    const PLO_GLOBAL uint32_t *pq = (const PLO_GLOBAL uint32_t *)(ok ? rd.p + (b0 - qsh) : safe);
#endif
    w.r4 = *(const PLO_GLOBAL Ops4 *)pr;
    w.r1 = pr[4];
    w.q4 = *(const PLO_GLOBAL Ops4 *)pq;
    w.q1 = pq[4];
    w.rsh = rsh;
    w.qsh = qsh;
    w.jmin = jmin;
    return ok;
}
PLO_DEV void xw16_decode(const ReadSeq &rd, const XW16 &wx, unsigned X[4]) {
    struct {
        unsigned wr[5], wq[5];
        int rsh, qsh, jmin;
    } w = {{wx.r4.x, wx.r4.y, wx.r4.z, wx.r4.w, wx.r1}, {wx.q4.x, wx.q4.y, wx.q4.z, wx.q4.w, wx.q1}, wx.rsh, wx.qsh, wx.jmin};
    const bool bam4 = rd.fmt != PLO_SEQ_ASCII;
    unsigned D[4];
    if (bam4) {
        unsigned S[5];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            unsigned Q = wv::align_bytes(w.wq[q + 1], w.wq[q], (unsigned)w.qsh);
            unsigned H = (Q >> 4) & 0x0f0f0f0fu, L = Q & 0x0f0f0f0fu;
            S[2 * q] = wv::perm_bytes(L, H, 0x05010400u);
            if (2 * q + 1 < 5) S[2 * q + 1] = wv::perm_bytes(L, H, 0x07030602u);
        }
        const unsigned par = (unsigned)(w.jmin & 1);
        const unsigned long long lo = rd.flip ? 0x4e4e4e434e47544eull : 0x565352474d43413dull;
        const unsigned long long hi = rd.flip ? 0x4e4e4e4e4e4e4e41ull : 0x4e42444b48595754ull;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            unsigned T = wv::align_bytes(S[v + 1], S[v], par);
            unsigned idx = T & 0x07070707u;
            unsigned dl = wv::perm_bytes((unsigned)(lo >> 32), (unsigned)lo, idx);
            unsigned dh = wv::perm_bytes((unsigned)(hi >> 32), (unsigned)hi, idx);
            unsigned mk = ((T >> 3) & 0x01010101u) * 0xffu;
            D[v] = (dh & mk) | (dl & ~mk);
        }
    } else {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            D[v] = wv::align_bytes(w.wq[v + 1], w.wq[v], (unsigned)w.qsh);
            if (rd.flip) D[v] = comp4(D[v]);
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        unsigned R = wv::align_bytes(w.wr[u + 1], w.wr[u], (unsigned)w.rsh);
        unsigned B = rd.flip ? wv::perm_bytes(0u, D[3 - u], 0x00010203u) : D[u];
        X[u] = R ^ B;
    }
}

// The left breakend homology of one indel cluster (left_homology, lift_core.hpp), split in three: lane_probe_arm() does the
// index checks of indel_breakend_homology.rs:32-39 when the cluster ends; lane_probe_load() sends the loads of the first 16-base
// window -- at the top of the lane's NEXT round, so that the loads and their use (lane_probe_finish, at that round's event) lie in
// one loop iteration with the scan between them: loads in flight across the loop's back edge are waited for right there (the
// compiler copies loop-carried values at the back edge), which is what the first version of this stage did without meaning to;
// lane_probe_finish() turns the words into the match run and continues window by window (synchronously) in the rare case that
// all 16 bases agree.
struct LaneProbe {
    XW16 w;
    int re = 0, qe = 0, maxk = 0;
    bool async_ok = false;
    bool miss = false;  // sparse bases: the window's granule is absent
};
// Wave-uniform call that overwrites the probe parameters of EVERY lane (none is pending when it is made: an event resolves the
// lane's pending cluster first).  `on`: the lanes whose cluster ends; sets their `panic` where the reference's slice index would.
PLO_DEV void lane_probe_arm(LaneProbe &p, bool on, int ref_len, int rs, int del, const ReadSeq &rd, int qs, int ins, int bound, bool &panic) {
    const int re = rs + del, qe = qs + ins;
    const int max_left = wv::imin(rs, qs);  // max_left_offset (:32)
    int maxk = wv::imin(max_left, bound);
    const bool bad = (max_left > 0) & ((re - 1 >= ref_len) | (qe - 1 >= rd.len));  // slice-index panic (:38-39)
    panic = panic | (on & bad);
    maxk = (bad | !on) ? 0 : maxk;
    p.re = re;
    p.qe = qe;
    p.maxk = maxk;
}
// wave-uniform call; `on`: the lanes with an armed cluster
PLO_DEV void lane_probe_load(LaneProbe &p, bool on, const uint8_t *ref, int ref_len, const ReadSeq &rd, const uint8_t *safe) {
    p.async_ok = xw16_issue(on & (p.maxk > 0), ref, ref_len, p.re - 16, rd, p.qe - 16, safe, p.w, p.miss);
}
PLO_DEV int match_run_back_from(const uint8_t *ref, int ref_len, int re, ReadSeq &rd, int qe, int maxk, int k, int &probes) {
    while (k < maxk) {
        unsigned X[4];
        if (!xor_window16(ref, ref_len, re - k - 16, rd, qe - k - 16, X)) break;
        int n = wv::imin(16, maxk - k);
        int m = wv::imin(zero_bytes_from_top(X), n);
        probes += wv::imin(m + 1, n);
        k += m;
        if (m < n) return k;
    }
    while (k < maxk) {
        int n = wv::imin(8, maxk - k);
        int a[8], b[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            int jj = j < n ? j : 0;
            a[j] = ((const PLO_GLOBAL uint8_t *)ref)[re - 1 - k - jj];
            b[j] = read_base(rd, qe - 1 - k - jj);
        }
        int adv = n;
#pragma unroll
        for (int j = 7; j >= 0; --j)
            if (j < n && a[j] != b[j]) adv = j;
        probes += wv::imin(adv + 1, n);
        k += adv;
        if (adv < n) break;
    }
    return k;
}
PLO_DEV int top_zero_bytes(const unsigned X[4]) {  // zero_bytes_from_top without branches
    const unsigned long long hi = ((unsigned long long)X[3] << 32) | X[2], lo = ((unsigned long long)X[1] << 32) | X[0];
    const int zh = hi ? (__builtin_clzll(hi) >> 3) : 8, zl = lo ? (__builtin_clzll(lo) >> 3) : 8;
    return hi ? zh : 8 + zl;
}
// wave-uniform call; `on`: the lanes whose pending cluster is resolved now
PLO_DEV int lane_probe_finish(const LaneProbe &p, bool on, const uint8_t *ref, int ref_len, ReadSeq &rd, int &probes) {
    unsigned X[4];
    xw16_decode(rd, p.w, X);  // (registers only: harmless where nothing was loaded)
    const int n = wv::imin(16, p.maxk);
    const int m = wv::imin(top_zero_bytes(X), n);
    rd.miss = rd.miss | (on & p.miss);  // absent bases: no homology is reported, the item is lifted again from the complete read
    const bool live = on & (p.maxk > 0) & !p.miss;
    const bool fast = live & p.async_ok;
    int h = fast ? m : 0;
    probes += fast ? wv::imin(m + 1, n) : 0;
    // the window lay outside a buffer (first / last bases of a sequence), the batch is sparse, or all 16 bases agree and the
    // match run allows more: window by window from there
    const bool more = live & ((!p.async_ok) | ((m == n) & (n < p.maxk)));
    if (wv::ballot(more) != 0ull) {
        if (more) h = match_run_back_from(ref, ref_len, p.re, rd, p.qe, p.maxk, h, probes);
    }
    return h;
}

// -------------------------------------------------------------------------------------------------------------------
// Heavy items (k_lift_lanes_g): the lane's region lies in wave-private GLOBAL memory, and the stages reach it through two small
// LDS windows per lane -- every stage reads its input front to back and writes its output front to back, so a read window
// [rbase, rbase + LANE_RW) and a write window [wbase, wbase + LANE_WW) of region indices are all it needs.  The windows of all
// lanes are refilled / flushed together (16 bytes per global access and lane) whenever some lane runs out: every LANE_RW
// iterations at most.  (Reaching into the global region op by op instead -- the first version of that kernel -- makes every access
// an L2 round trip on the loop's dependence chain: 15.9 ms against 13.1 ms of the workgroup-per-item kernel on the stress workload.)
// Window element j of lane l is word j * 64 + l of the wave's LDS: whatever positions the lanes are at, lane l uses bank l.  The
// windows are lane-private: no barrier between a lane's writes and its reads.
// (Measured and dropped: a third window of eight block-map entries per lane for the liftover's cursor, so that a block crossing reads
// LDS instead of global memory -- 9.98 ms either way on the stress workload; and k_chunk_sort over the heavy classes when their groups
// outnumber the resident waves -- 16.3 ms either way at 250 k reads.)
// -------------------------------------------------------------------------------------------------------------------
constexpr int LANE_RW = 20, LANE_WW = 28;  // dwords per lane; LANE_RW a multiple of 4
constexpr int LANE_WIN_DWORDS = LANE_RW + LANE_WW;
constexpr int LANE_WIN_MARGIN = 8;            // most ops a lane writes between two looks at the write window's fill
constexpr int LANE_REGION_PAD = LANE_RW + 4;  // behind a region: a refill at its last op reads LANE_RW dwords
struct LaneWin {
    uint32_t *G = nullptr;                  // index 0 of the lane's region (global memory)
    uint32_t *rw = nullptr, *ww = nullptr;  // element 0 of the lane's windows (LDS; element j at [j * 64])
    int rbase = 0, wbase = 0;               // region index of element 0
};
PLO_DEV void win_fill(LaneWin &w, bool on, int idx) {
    if (on) {
        w.rbase = idx;
        Ops4 v[LANE_RW / 4];
#pragma unroll
        for (int q = 0; q < LANE_RW / 4; ++q) v[q] = *(const PLO_GLOBAL Ops4 *)(w.G + idx + 4 * q);
#pragma unroll
        for (int q = 0; q < LANE_RW / 4; ++q) {
            w.rw[(4 * q) * 64] = v[q].x;
            w.rw[(4 * q + 1) * 64] = v[q].y;
            w.rw[(4 * q + 2) * 64] = v[q].z;
            w.rw[(4 * q + 3) * 64] = v[q].w;
        }
    }
}
// the same from the batch's input CIGAR `src` (n_in ops), walked backwards for reverse-mapped contig segments: window element j =
// op idx + j in walking order.  Heavy items whose first stage can read the input as it is skip the LOAD pass.
PLO_DEV void win_fill_input(LaneWin &w, bool on, int idx, const uint32_t *src, int n_in, bool rev, int lo_ok, int hi_ok) {
    // [lo_ok, hi_ok): indices relative to `src` that lie inside the batch's CIGAR buffer (a quad that reaches past the item's ends reads its
    // neighbours' ops, masked below; only one that would leave the buffer takes the op-by-op loads).  All LANE_RW / 4 loads are in flight
    // together: inside lane-divergent branches every one of them was waited for on its own (five round trips per refill).
    uint32_t a[LANE_RW];
    const uint32_t *qa[LANE_RW / 4];
    bool edge = false;
#pragma unroll
    for (int q = 0; q < LANE_RW / 4; ++q) {
        const int kq = idx + 4 * q;
        const bool want = on & (kq < n_in);
        const int gi = rev ? n_in - 4 - kq : kq;
        const bool inside = (gi >= lo_ok) & (gi + 4 <= hi_ok);
        edge = edge | (want & !inside);
        qa[q] = (want & inside) ? src + gi : (const uint32_t *)plo_safe_words;
    }
    if (wv::ballot(edge) == 0ull) {
        Ops4 v[LANE_RW / 4];
#pragma unroll
        for (int q = 0; q < LANE_RW / 4; ++q) v[q] = *(const PLO_GLOBAL Ops4 *)qa[q];
#pragma unroll
        for (int q = 0; q < LANE_RW / 4; ++q) {
            a[4 * q] = rev ? v[q].w : v[q].x;
            a[4 * q + 1] = rev ? v[q].z : v[q].y;
            a[4 * q + 2] = rev ? v[q].y : v[q].z;
            a[4 * q + 3] = rev ? v[q].x : v[q].w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < LANE_RW; ++j) {
            a[j] = 0u;
            if (on && idx + j < n_in) a[j] = src[rev ? n_in - 1 - idx - j : idx + j];
        }
    }
    if (on) {
        w.rbase = idx;
#pragma unroll
        for (int j = 0; j < LANE_RW; ++j) w.rw[j * 64] = (idx + j < n_in) ? a[j] : 0u;
    }
}
// region indices [wbase, end) are in the window: out with them
PLO_DEV void win_flush(LaneWin &w, bool on, int end) {
    if (on) {
        const int cnt = end - w.wbase;
        uint32_t *const dst = w.G + w.wbase;
#pragma unroll
        for (int q = 0; q < LANE_WW / 4; ++q) {
            Ops4 v;
            v.x = w.ww[(4 * q) * 64];
            v.y = w.ww[(4 * q + 1) * 64];
            v.z = w.ww[(4 * q + 2) * 64];
            v.w = w.ww[(4 * q + 3) * 64];
            if (4 * q + 3 < cnt) *(PLO_GLOBAL Ops4 *)(dst + 4 * q) = v;
        }
        const int n4 = cnt & ~3;
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (n4 + j < cnt) dst[n4 + j] = w.ww[(n4 + j) * 64];
        w.wbase = end;
    }
}

// -------------------------------------------------------------------------------------------------------------------
// One group of up to 64 items, lane t <-> item t.  `lds`: the wave's slice of capw dwords, shared out among the items by their
// weights (light items) -- or, WIN, one region of fixed_stride dwords per lane in wave-private global scratch, reached through LDS
// windows (heavy items, k_lift_lanes_g).
// (Measured and dropped: the group's CIGAR span copied into LDS with coalesced loads and picked apart there, results gathered in
// LDS and stored coalesced -- 37 % slower than every lane reading / writing its own 16 bytes: the extra LDS round trips cost more
// than the scattered requests.)
// -------------------------------------------------------------------------------------------------------------------
// The block-map entries a group's liftover cursors read, staged in LDS: the items of a group are neighbours on a contig, their
// windows into the block map overlap almost entirely, and the union -- a dozen entries or two -- goes into LANE_KVS entries of the
// wave's LDS with one coalesced load per group.  The cursor then reads LDS (one ds_read_b64 per crossing, asked for at the top of
// the iteration and used at its end) instead of global memory: the first version requested the entry after next from global memory at
// every crossing and, because the value was carried across the loop's back edge, waited for it at the end of the same iteration --
// an L2 round trip in every iteration of every group.  Items whose window lies outside the staged range keep the global loads.
constexpr int LANE_KVS = 128;                  // staged entries per wave
constexpr int LANE_KVS_DWORDS = 2 * LANE_KVS;  // behind the wave's slice (lds + capw) / windows (lds + 64 * LANE_WIN_DWORDS)
// The light-item kernel takes the number of staged entries from the launch (DevWork::lane_kvs, a multiple of 64 up to LANE_KVS_MAX): groups
// of a sort window wider than 128 reads are every n-th read of a longer stretch of the contig, and their union of block-map entries grows
// with the window (wgs30x, 4.8-fold coverage per haplotype: ~0.15 entries per kb, 64 neighbouring reads span 200 kb, 512 span 1.6 Mb).
constexpr int LANE_KVS_MAX = 512;
#ifdef PLO_EMULATOR
// Test visibility (tests/emu/, emulator builds only -- no device code sees this): how the liftover loops of lane_tile and of the streaming
// kernel (lane_stream.hpp) were entered and where their block-map entries came from, summed until the harness clears them.
struct EmuKvStats {
    unsigned long long all_lds;     // lane_tile rounds that ran the all-staged copy of the liftover loop
    unsigned long long mixed;       // ... the copy with the global fallback
    unsigned long long global_kv;   // block-map entries lane_tile's cursors fetched from global memory (per lane)
    unsigned long long s_restage;   // streaming kernel: stagings of the team's entries
    unsigned long long s_mid;       // ... of them while another lane was in the middle of an item
    unsigned long long s_flip_on;   // ... lanes in the middle of an item whose kv_lds went from false to true
    unsigned long long s_flip_off;  // ... and from true to false
    unsigned long long s_global_kv; // streaming kernel: entries fetched from global memory (per lane)
};
inline EmuKvStats g_emu_kv = {0, 0, 0, 0, 0, 0, 0, 0};
constexpr unsigned EMU_LIFT_TRIPS = 1u << 18;  // trips of one group's liftover loop before the emulator gives up (an item of 2^16 ops and keys)
#endif
// NOSHIFT: an instantiation for groups of the class without the shift stage (forward-mapped contig segments), compiled without that
// stage's code and state -- lanes that would need it are handed to the retry list (the class order keeps them away).
// STATS: the launch counts its algorithmic bytes (SURVEY.md 8(d)'s B_item per item: plo_timing::algo_bytes) and the lanes at work per
// loop trip (plo_timing::lane_utilisation).  The production instantiation of the light-item kernel is compiled WITHOUT them (the trip
// counters sat in the two hot loops: an s_bcnt1 and two 64-bit adds per trip); a context asks for the counting kernel with
// PLO_LANE_STATS=1 (bench.py's statistics pass, tools/, the tests of plo_timing).
// H16: 16-bit ops in the regions (above); only without WIN, and only for stage sets with the liftover (the caller's business).
template <bool SP, bool WIN = false, bool NOSHIFT = false, bool STATS = true, bool H16 = false>
PLO_DEV void lane_tile(const DevIndex &ix, const DevBatch &bt, const DevWork &wk, uint32_t stages, uint32_t item_begin, int nit,
                       uint32_t *lds, int capw, int fixed_stride, WaveCtx &ctx, const uint32_t *list, bool have_g, uint32_t g_pre,
                       uint32_t *greg = nullptr, uint32_t *kvs = nullptr, int kvs_n = LANE_KVS) {
    // WIN (heavy items): `lds` = 64 x LANE_WIN_DWORDS dwords of LDS for the lanes' windows, `greg` = 64 regions of fixed_stride dwords
    // in global memory; else: `lds` = the wave's slice of capw dwords, the regions themselves.
    static_assert(!(H16 && WIN), "16-bit ops: LDS regions only");
    const int lane = wv::lane();
    const bool has = lane < nit;
    const uint32_t g = have_g ? g_pre : (has ? list[item_begin + (uint32_t)lane] : 0u);
#ifdef PLO_PHASE_TIMING
    long long tlast = wv::clock();
#define PLO_LT(k)                     \
    {                                 \
        long long now_ = wv::clock(); \
        ctx.tph[k] += now_ - tlast;   \
        tlast = now_;                 \
    }
#define PLO_LC(k, v) ctx.tph[k] += (v);  // loop trip counts (statistics of the timing build)
#else
#define PLO_LT(k)
#define PLO_LC(k, v)
#endif

    // ---- descriptors (build_item_desc, enumerate.hpp) ----
    int n_in = 0, n_m = 0, in_off = 0, pos1 = 0, kv0 = 0, kv1 = 0, W0 = 0, W1 = 0, seq_len = 0, shift_ref_len = 0;
    bool len_bad = false, rev = false, do_shift = false, flip = false;
    unsigned long long seq_off = 0, shift_ref = 0;
    if (has) {
        in_off = (int)wk.d.in_off[g];
        n_in = (int)wk.d.n_in[g];
        n_m = (int)wk.d.n_m[g];
        W0 = (int)wk.d.w0[g];
        W1 = (int)wk.d.w1[g];
        kv0 = (int)wk.d.kv0[g];
        kv1 = (int)wk.d.kv1[g];
        const uint32_t fl = wk.d.flags[g];
        pos1 = wk.d.pos1[g];
        seq_len = (int)wk.d.seq_len[g];
        const uint32_t read_len_in = wk.d.read_len[g];
        len_bad = read_len_in == 0xffffffffu || (uint32_t)seq_len != read_len_in;  // LENGTH CHECK, see lift_tile
        seq_off = wk.d.seq_off[g];
        shift_ref = wk.d.shift_ref[g];
        shift_ref_len = wk.d.shift_ref_len[g];
        rev = (fl & ITF_REV) != 0;
        flip = (fl & ITF_FLIP) != 0;
        const bool contig_fwd = (fl & ITF_CONTIG_FWD) != 0;
        do_shift = (stages & PLO_STAGE_LSHIFT) && (!(stages & PLO_STAGE_STRAND) || !contig_fwd);
    }
    const bool need_shift = do_shift;
    if constexpr (NOSHIFT) do_shift = false;
    // The item's region (enumerate.hpp lane_region_dwords): its ops as LOAD stores them -- match runs merged when the next stage
    // merges them anyway -- behind a gap for what the liftover may add.
    const bool merges = do_shift || (stages & PLO_STAGE_LIFTOVER);
    const int n_ld = merges ? n_m : n_in;
    const int gap = has ? lane_region_gap(W0, W1) : 0;
    // (H16: in halfwords, with room for the extra chunks of long ops; the slice is shared out in dwords)
    const int W = n_ld + gap + LANE_SLACK + (H16 ? H16_ALLOW : 0);  // dwords (H16: halfwords)
    const int W_dw = H16 ? (W + 1) >> 1 : W;

    // ---- block-map entries of the group -> LDS (loads now; the stores follow the LOAD pass, whose round trip covers this one) ----
    int kvs_base = 0, kvs_cnt = 0;
    bool kv_lds = false, kvs_store = false;
    constexpr int KVS_Q = H16 ? LANE_KVS_MAX / 64 : LANE_KVS / 64;  // loads per lane that stage the entries (32-bit regions: LANE_KVS entries at most)
    if constexpr (!H16) kvs_n = kvs_n < LANE_KVS ? kvs_n : LANE_KVS;
    KV kvs_e[KVS_Q];
#pragma unroll
    for (int q = 0; q < KVS_Q; ++q) kvs_e[q] = {0, 0};
    if (kvs != nullptr && (stages & PLO_STAGE_LIFTOVER)) {
        // the cursor of an item reads the entries [W0, min(kv1, W1 + 2)): its window and the look-ahead behind it
        const int need_hi = wv::imin(kv1, W1 + 2);
        kvs_base = -wv::reduce_max(has ? -W0 : -IMAX);
        const int top = wv::reduce_max(has ? need_hi : 0);
        const int cnt = wv::imax(0, wv::imin(top - kvs_base, kvs_n));
        kv_lds = has & (need_hi <= kvs_base + cnt);
        kvs_cnt = cnt;
#pragma unroll
        for (int q = 0; q < KVS_Q; ++q)
            if (64 * q < kvs_n && lane + 64 * q < cnt) kvs_e[q] = ix.kv[kvs_base + lane + 64 * q];
        kvs_store = true;
    }

    // items no region can hold (the class order keeps them away; tiny test capacities do not): the wave-cooperative path
    bool pending = has;
    {
        const bool defer = has && (W_dw > (WIN ? fixed_stride - LANE_REGION_PAD : capw) || (NOSHIFT && need_shift));
        const unsigned long long dm = wv::ballot(defer);
        if (dm != 0ull) {
            int slot = 0;
            if (lane == 0) slot = (int)wv::atomic_add_global(&wk.counters[CNT_NRETRY], (unsigned long long)__builtin_popcountll(dm));
            slot = wv::bcast_first(slot);
            if (defer) {
                wk.retry_list[slot + __builtin_popcountll(dm & ((1ull << lane) - 1ull))] = g;
                wk.status[g] = (uint8_t)ITEM_NEED_BIG;
                pending = false;
            }
        }
    }

    // ---- rounds: the longest prefix of the pending items whose regions fit the slice (nearly always all of them) ----
    while (wv::ballot(pending) != 0ull) {
        const int wv_ = pending ? W_dw : 0;
        const int incl = WIN ? 0 : wv::scan_add(wv_);
        const bool act0 = pending && (WIN || incl <= capw);
        pending = pending && !act0;
        // R: where the stages read / write their ops by region index -- the region itself, or (WIN) re-pointed at a window
        uint32_t *R = WIN ? nullptr : lds + (act0 ? incl - wv_ : 0);
        uint16_t *const R16 = (uint16_t *)R;  // (H16: the same region, indexed in halfwords)
        LaneWin win;
        if constexpr (WIN) {
            // (lanes without an item point at the wave's first region: the writer's clean-up reads o.R[0] unconditionally, and with fewer
            // than 64 items per wave the regions of the lanes beyond them lie outside the wave's -- for the last wave, outside the buffer's --
            // scratch; found by tests/test_fuzz_parity.py::test_fuzz_hip_heavy_lane_kernel[5] as a GPU memory fault)
            win.G = greg + (size_t)(has ? lane : 0) * (size_t)fixed_stride;
            win.rw = lds + lane;
            win.ww = lds + LANE_RW * 64 + lane;
        }
        wv::sync();  // the previous round's regions are dead

        int status = PLO_ITEM_LIFTED;
        bool alive = act0;
        bool shift_on = act0 && do_shift;
        if (shift_on && shift_ref == 0ull) {  // rev_contig_seq.unwrap() on None (src/read_alignment_scanner.rs:174)
            status = PLO_ITEM_PANIC;
            alive = false;
            shift_on = false;
        }
        bool ovf = false, panic = false;
        unsigned algo = 0;
        int cur_off = 0, n = 0;  // the item's current CIGAR: R[cur_off .. cur_off + n)
        int nops = 0;            // H16: its ops (n counts halfwords; an op longer than H16_MAX has several)
        constexpr int ST = WIN ? 64 : 1;
        // the op at R[cur_off + k] (lanes without one: some readable word)
        auto rd_at = [&](int k, bool ok) -> uint32_t {
            if constexpr (WIN) return win.rw[ok ? (cur_off + k - win.rbase) * 64 : 0];
            else if constexpr (H16) return h16_dec(R16[cur_off + (ok ? k : 0)]);
            else return R[cur_off + (ok ? k : 0)];
        };
        // WIN, stages with the liftover: the first stage of an item -- the shift or the liftover, which take =, X and M ops alike --
        // reads the batch's input through the window; `ext`: the lane's current CIGAR is still that input (cur_off = 0)
        const bool direct = WIN && (stages & PLO_STAGE_LIFTOVER) != 0u;
        const int n_cig_all = WIN ? (int)bt.seg_cigar_off[bt.n_segs] : 0;  // ops in the batch's CIGAR buffer
        bool ext = false;
        auto rd_fill = [&](bool on, int idx) {
            if constexpr (WIN) {
                if (direct) {
                    if (wv::ballot(on & ext) != 0ull) win_fill_input(win, on & ext, idx, bt.cigar + in_off, n_in, rev, -in_off, n_cig_all - in_off);
                    if (wv::ballot(on & !ext) != 0ull) win_fill(win, on & !ext, idx);
                } else {
                    win_fill(win, on, idx);
                }
            }
        };
        // WIN: before rd_at -- the read windows of the stage's lanes move up to their positions when one of them has left its window
        auto rd_need = [&](int k, bool ok, bool stage_on) {
            if constexpr (WIN) {
                if (wv::ballot(ok & (cur_off + k - win.rbase >= LANE_RW)) != 0ull) rd_fill(stage_on, cur_off + k);
            }
        };
        // a stage's writer, from region index `base`
        auto wr_open = [&](LaneOut &o, int base) {
            if constexpr (WIN) {
                win.wbase = base;
                o.R = win.ww;
            } else if constexpr (H16) {
                o.H = R16 + base;
            } else {
                o.R = R + base;
            }
        };
        // WIN: before a round of at most LANE_WIN_MARGIN pushes
        auto wr_room = [&](LaneOut &o, bool on, int base) {
            if constexpr (WIN) {
                if (wv::ballot(on & !o.ovf & (base + o.no - win.wbase > LANE_WW - LANE_WIN_MARGIN)) != 0ull) {
                    win_flush(win, on & !o.ovf, base + o.no);
                    o.R = win.ww - o.no * 64;
                }
            }
        };
        // clean_up_cigar_edge_indels' trailing edge + compress: WIN, on the region itself (walks back)
        auto wr_finish = [&](LaneOut &o, bool on, int base, int wlim) {
            if constexpr (WIN) {
                win_flush(win, on & !o.ovf, base + o.no);
                o.R = win.G + base;
            }
            lane_out_finish<H16>(o, on, wlim);
        };
        int pos = pos1;
        ReadSeq rd = item_read_seq<SP>(bt, seq_off, seq_len, flip ? 1 : 0);
        PLO_LT(0)

        // ---- LOAD: input ops -> LDS, reversed for reverse-mapped contig segments (:167) --------------------------------------
        // Items of the shift stage: at the region's upper end (the shift writes from `gap` upwards behind its own reading
        // position).  The others: at `gap`, where the liftover expects its input.  Neighbouring alignment-match ops (= X M) are
        // merged into one M on the way when the next stage treats the three alike and merges what comes of them anyway: the
        // shift builder (add_match: match_run += len, emitted as M, cigar_indel_shifter.rs:150-153,136) and the liftover (:102-109
        // turn every match piece into M, compress_cigar :220 merges the pieces of neighbouring ops).  Same result, a third fewer
        // ops to walk -- and the ops of a shifted item then alternate match / cluster, which is what keeps its scans short.
        if (direct) {
            n = act0 ? n_in : 0;
            ext = act0;
        } else {
            const bool ld = act0;
            const bool merge = ld & merges;
            const int inb = shift_on ? W - n_ld - (H16 ? H16_ALLOW : 0) : gap;
            const int nmax = wv::reduce_max(ld ? n_in : 0);
            const int n_cig = (int)bt.seg_cigar_off[bt.n_segs];  // ops in the batch's CIGAR buffer (wave-uniform)
            uint32_t run = 0;
            bool has_run = false;
            int w = 0;
            if constexpr (WIN) win.wbase = inb;
            bool ld_ovf = false;  // H16: more chunks than the region allows
            auto put = [&](bool on, uint32_t v) {
                if constexpr (WIN) {
                    if (on) win.ww[(inb + w - win.wbase) * 64] = v;
                } else if constexpr (H16) {
                    // (chunks: the first here, the others -- three runs in a thousand -- behind a wave-uniform test; `w` moves in put_more)
                    // (a lone = or X is an M to the stages that follow, like the runs merged above: the format has codes 0 .. 6)
                    const uint32_t len = v >> 4;
                    const int vt = b_is_match((int)(v & 15u)) ? (int)OP_M : (int)(v & 15u);
                    const bool ok = inb + w < W;
                    if (on & ok) R16[inb + w] = (uint16_t)h16_enc(vt, len < (uint32_t)H16_MAX ? len : (uint32_t)H16_MAX);
                    ld_ovf = ld_ovf | (on & !ok);
                } else {
                    if (on) R[inb + w] = v;
                }
            };
            auto put_more = [&](bool on, uint32_t v) {  // H16: the chunks after the first
                if constexpr (H16) {
                    const uint32_t len = v >> 4;
                    const bool big = on & (len > (uint32_t)H16_MAX);
                    if (wv::ballot(big) != 0ull) {
                        uint32_t rest = big ? len - (uint32_t)H16_MAX : 0u;
#pragma unroll
                        for (int c = 1; c < H16_CHUNKS; ++c) {
                            const bool more = rest > 0u;
                            const uint32_t part = rest < (uint32_t)H16_MAX ? rest : (uint32_t)H16_MAX;
                            const bool ok = inb + w < W;
                            if (more & ok) R16[inb + w] = (uint16_t)h16_enc(b_is_match((int)(v & 15u)) ? (int)OP_M : (int)(v & 15u), part);
                            ld_ovf = ld_ovf | (more & !ok);
                            w += more ? 1 : 0;
                            rest -= part;
                        }
                        ld_ovf = ld_ovf | (rest > 0u);
                    }
                }
            };
            // LB ops per round trip: LB / 4 loads of 16 bytes per lane (every lane reads its own CIGAR), ALL of them in flight together.
            // The loads are unconditional (lanes without a quad read plo_safe_words): a load inside a lane-divergent branch is waited
            // for at the branch's end, one round trip per load -- the first version of this pass did that twice per eight ops.  A quad
            // that reaches past its item (the item's last one) is read whole, the neighbour's ops masked below; only a quad that would
            // leave the batch's buffer (first / last ops of the batch) sends the wave through the op-by-op loads.
            constexpr int LB = 16;
            for (int k0 = 0; k0 < nmax; k0 += LB) {
                PLO_LC(10, 1)
                if constexpr (WIN) {
                    if (wv::ballot(ld & (inb + w - win.wbase > LANE_WW - (LB + 1))) != 0ull) win_flush(win, ld, inb + w);
                }
                uint32_t r[LB];
                const uint32_t *qa[LB / 4];
                bool edge = false;
#pragma unroll
                for (int q = 0; q < LB / 4; ++q) {
                    const int kq = k0 + 4 * q;
                    const bool want = ld & (kq < n_in);
                    const int gi = in_off + (rev ? n_in - 4 - kq : kq);  // the ops kq .. kq+3 in walking order are four neighbours in memory
                    const bool inside = (gi >= 0) & (gi <= n_cig - 4);
                    edge = edge | (want & !inside);
                    qa[q] = (want & inside) ? bt.cigar + gi : (const uint32_t *)plo_safe_words;
                }
                if (wv::ballot(edge) == 0ull) {
                    Ops4 v[LB / 4];
#pragma unroll
                    for (int q = 0; q < LB / 4; ++q) v[q] = *(const PLO_GLOBAL Ops4 *)qa[q];
#pragma unroll
                    for (int q = 0; q < LB / 4; ++q) {
                        r[4 * q] = rev ? v[q].w : v[q].x;
                        r[4 * q + 1] = rev ? v[q].z : v[q].y;
                        r[4 * q + 2] = rev ? v[q].y : v[q].z;
                        r[4 * q + 3] = rev ? v[q].x : v[q].w;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < LB; ++j) {
                        r[j] = 0u;
                        if (ld && k0 + j < n_in) r[j] = bt.cigar[in_off + (rev ? (n_in - 1 - k0 - j) : k0 + j)];
                    }
                }
#pragma unroll
                for (int j = 0; j < LB; ++j) {
                    const bool have = ld & (k0 + j < n_in);
                    const uint32_t c = r[j];
                    const bool join = merge & have & has_run & b_is_match(op_type(c)) & b_is_match(op_type(run));
                    const bool flush = have & has_run & !join;
                    put(flush, run);
                    w += flush ? 1 : 0;
                    put_more(flush, run);
                    run = join ? ((run & ~15u) + (c & ~15u)) | (uint32_t)OP_M : (have ? c : run);
                    has_run = has_run | have;
                }
            }
            put(ld & has_run, run);
            w += (ld & has_run) ? 1 : 0;
            put_more(ld & has_run, run);
            if constexpr (WIN) win_flush(win, ld, inb + w);
            n = ld ? w : 0;
            cur_off = ld ? inb : 0;
            if constexpr (H16) ovf = ovf | (ld & ld_ovf);
        }
        if (kvs_store) {  // (wave-uniform; once per group)
#pragma unroll
            for (int q = 0; q < KVS_Q; ++q)
                if (64 * q < kvs_n) {  // (wave-uniform)
                    kvs[2 * (lane + 64 * q)] = (uint32_t)kvs_e[q].key;
                    kvs[2 * (lane + 64 * q) + 1] = (uint32_t)kvs_e[q].val;
                }
            kvs_store = false;
        }
        wv::sync();

        PLO_LT(1)
        // ---- LEFT SHIFT (left_shift_indels.rs:17-39 + cigar_indel_shifter.rs:10-165) -------------------------------------------
        // EVENT-ALIGNED walk: a round = every lane scans its ops (cheap) up to its next event -- the end of an indel cluster, an
        // op that flushes the builder's match run (:155-165), or the end of the CIGAR -- and then all lanes run the event code
        // together, so that the expensive part (probe decode, emission) executes with most lanes active instead of with the
        // fifth that sits on a cluster end at any given op index.
        // The emission of a cluster (M I D, :132-147) needs its homology; the probe is sent when the cluster ends and the cluster
        // stays `pend`ing -- match bases that follow collect in `msince` -- until the lane's next event: its probe's HBM round trip
        // runs under the scan in between.
        // CLEAN items (on HiFi data all but a few in a thousand), in LOCKSTEP: iteration j is every lane's j-th cluster, at the
        // known index 2j + 1 behind the lane's first match.  M(a0) X1 M(a1) .. Xn M(an) becomes M(a0 - s1) X1 M(s1 + a1 - s2) .. Xn M(sn + an)
        // with s_j = min(s_{j-1} + a_{j-1}, h_j): the builder's arithmetic (`match` = shift carried + bases since, :132, :150-153) without
        // its scan, its cluster state and its writer -- the ops stay where they are, only the matches' lengths change.  The probe's
        // addresses come from the input walk alone, so the window of cluster j + 1 is asked for before cluster j is resolved (two probes,
        // alternating: nothing in flight changes registers at the back edge); only the clamp needs the carry.
        // A lane whose shift EMPTIES a match (the builder skips that op; its neighbours meet, the leading edge rule may apply) finishes the
        // arithmetic all the same and then streams its region through the writer, which is the builder's push sequence exactly.
        constexpr bool LOCK = PLO_SHIFT_LOCKSTEP && !WIN && !H16 && !SP && !NOSHIFT;
        if constexpr (LOCK) {
            // Which lanes are clean: (S|H)* M (X M)* (S|H)* over the stored ops, X one I or one D, every length > 0, no two equal
            // neighbours (the writer would merge them), hence no N and no P.  Three short loops over the region: the leading clips, the
            // (M, X) pairs -- two ops per trip --, the trailing clips.
            const bool lk = shift_on & (wk.lane_lockstep_off == 0u);
            int n_lead = 0, lead_read = 0, ncl = 0;  // leading clip ops, the read bases they consume; clusters
            bool c_bad = false;
            const int end = cur_off + n;
            if (wv::ballot(lk) != 0ull) {
                {
                    bool go = lk;
                    int pt = -1;
                    while (wv::ballot(go) != 0ull) {
                        const bool have = go & (n_lead < n);
                        const uint32_t c = R[have ? cur_off + n_lead : 0];
                        const int t = op_type(c);
                        const bool clip = have & ((unsigned)(t - (int)OP_S) < 2u);
                        c_bad = c_bad | (clip & ((c < 16u) | (t == pt)));
                        lead_read += clip ? op_len(c) : 0;
                        n_lead += clip ? 1 : 0;
                        pt = t;
                        go = clip;
                    }
                }
                {
                    bool go = lk;
                    while (wv::ballot(go) != 0ull) {
                        const int i0 = cur_off + n_lead + 2 * ncl;
                        const bool h0 = go & (i0 < end), h1 = go & (i0 + 1 < end);
                        const uint32_t c0 = R[h0 ? i0 : 0], c1 = R[h1 ? i0 + 1 : 0];
                        const bool m = h0 & b_is_match(op_type(c0)) & (c0 >= 16u);
                        const bool x = h1 & b_is_indel(op_type(c1)) & (c1 >= 16u);
                        c_bad = c_bad | (go & !m);  // (behind an X, or first of all, a match must stand)
                        go = m & x;                 // (else: the end, a clip, or something the loop below refuses)
                        ncl += go ? 1 : 0;
                    }
                }
                {
                    int k = cur_off + n_lead + 2 * ncl + 1, pt = -1;
                    const bool go = lk & !c_bad;
                    while (wv::ballot(go & (k < end)) != 0ull) {
                        const bool have = go & (k < end);
                        const uint32_t c = R[have ? k : 0];
                        const int t = op_type(c);
                        c_bad = c_bad | (have & (((unsigned)(t - (int)OP_S) >= 2u) | (c < 16u) | (t == pt)));
                        pt = have ? t : pt;
                        k += have ? 1 : 0;
                    }
                }
            }
            const bool lock_on = lk & !c_bad;
            if (wv::ballot(lock_on) != 0ull) {
                const uint8_t *const sref = (const uint8_t *)(uintptr_t)shift_ref;
                const int m0 = lock_on ? cur_off + n_lead : 0;  // the lane's first match
                int ref_head = pos1, read_head = lead_read, carry = 0, probes = 0;
                bool marked = false;
                LaneProbe pa, pb;
                int a_a = 0, a_b = 0;  // the ORIGINAL length of the match in front of the probe's cluster
                // cluster j: heads, panic test and the window's loads
                auto issue = [&](LaneProbe &p, int &a, int j) {
                    const bool on = lock_on & (j < ncl);
                    const uint32_t cm = R[on ? m0 + 2 * j : 0], cx = R[on ? m0 + 2 * j + 1 : 0];
                    const int t = op_type(cx), L = op_len(cx);
                    a = op_len(cm);
                    const int rs = ref_head + a, qs = read_head + a;
                    const int del = t == OP_D ? L : 0, ins = t == OP_I ? L : 0;
                    // (no clamp yet: maxk = min(rs, qs), 0 where the reference panics; the clamp s + a > 0 does not change which lanes load)
                    lane_probe_arm(p, on, shift_ref_len, rs, del, rd, qs, ins, IMAX, panic);
                    lane_probe_load(p, on, sref, shift_ref_len, rd, (const uint8_t *)plo_safe_words);
                    ref_head = on ? rs + del : ref_head;
                    read_head = on ? qs + ins : read_head;
                };
                auto resolve = [&](LaneProbe &p, int a, int j) {
                    const bool on = lock_on & (j < ncl);
                    const int bound = carry + a;
                    p.maxk = wv::imin(p.maxk, bound);
                    int h = lane_probe_finish(p, on, sref, shift_ref_len, rd, probes);
                    h = rd.miss ? 0 : h;
                    const int sh = wv::imin(bound, h);  // actual_shift_len (:132)
                    if (on) R[m0 + 2 * j] = mk_op(OP_M, bound - sh);
                    marked = marked | (on & (bound == sh));
                    carry = on ? sh : carry;
                };
                PLO_MARK("LOCKSTEP LOOP BEGIN");
                issue(pa, a_a, 0);
                for (int j = 0; wv::ballot(lock_on & (j < ncl)) != 0ull; j += 2) {
                    PLO_LC(8, 2)
                    if constexpr (STATS) {
                        ctx.u_act += (unsigned)__builtin_popcountll(wv::ballot(lock_on & (j < ncl))) + (unsigned)__builtin_popcountll(wv::ballot(lock_on & (j + 1 < ncl)));
                        ctx.u_trips += 2;
                    }
                    issue(pb, a_b, j + 1);
                    resolve(pa, a_a, j);
                    issue(pa, a_a, j + 2);
                    resolve(pb, a_b, j + 1);
                }
                PLO_MARK("LOCKSTEP LOOP END");
                if (lock_on) R[m0 + 2 * ncl] = mk_op(OP_M, op_len(R[m0 + 2 * ncl]) + carry);  // the last match takes the last shift (every match is written, as M: a lone = or X of the input too)
                if constexpr (STATS) algo += lock_on ? 2u * (unsigned)probes : 0u;
                const bool mk = lock_on & marked;
                if (wv::ballot(mk) != 0ull) {  // read at cur_off, written at gap: behind the reader
                    LaneOut o;
                    wr_open(o, gap);
                    const int wl0 = cur_off - gap;
                    const int nmax = wv::reduce_max(mk ? n : 0);
                    for (int k = 0; k < nmax; ++k) {
                        const bool act = mk & (k < n);
                        const uint32_t c = R[cur_off + (act ? k : 0)];
                        lane_push<false, ST, H16>(o, act & (op_len(c) > 0), op_type(c), op_len(c), wl0 + k + 1);
                    }
                    wr_finish(o, mk, gap, wl0 + n);
                    if (mk) {
                        n = o.no;
                        cur_off = gap;
                        pos += o.lead_shift;
                        ovf = ovf | o.ovf;
                    }
                }
                shift_on = shift_on & !lock_on;  // clean lanes keep cur_off, n and pos; the others take the walk below
            }
        }
        if constexpr (!NOSHIFT) if (wv::ballot(shift_on) != 0ull) {
            const uint8_t *const sref = (const uint8_t *)(uintptr_t)shift_ref;
            LaneOut o;
            wr_open(o, gap);
            rd_fill(shift_on, cur_off);
            const int wl0 = cur_off - gap;  // the writer may use what lies below the reader: index < wl0 + ops consumed
            const int wl_ext = W - gap;     // ... or, reading the batch's input, all of the region
            int k = 0;
            bool fin = !shift_on;
            int ref_head = pos1, read_head = 0, match = 0, del = 0, ins = 0, blk_ref = 0, blk_read = 0;
            bool in_blk = false, pend = false;
            int p_match = 0, p_ins = 0, p_del = 0, msince = 0, probes = 0;
            LaneProbe pr;
            PLO_MARK("SHIFT LOOP BEGIN");
            for (unsigned long long bm; (bm = wv::ballot(!fin)) != 0ull;) {
                PLO_LC(8, 1)
                if constexpr (STATS) {
                    ctx.u_act += (unsigned)__builtin_popcountll(bm);
                    ctx.u_trips += 1;
                }
                wr_room(o, shift_on, gap);
                // the probes of the clusters that ended at the lanes' last events go out now: their round trips run under this round's scan
                if (wv::ballot(pend) != 0ull) lane_probe_load(pr, pend, sref, shift_ref_len, rd, (const uint8_t *)plo_safe_words);
                // scan to the next event (not consumed)
                bool stop = fin, ev_other = false, ev_end = false;
                int ev_t = 0, ev_L = 0;
                while (wv::ballot(!stop) != 0ull) {
                    PLO_LC(9, 1)
                    const bool act = !stop;
                    const bool have = k < n;
                    rd_need(k, have & shift_on, shift_on);
                    const uint32_t c = rd_at(k, have & (!WIN | shift_on));
                    const int t = op_type(c), L = op_len(c);
                    const bool indel = have & b_is_indel(t);
                    const bool ism = have & b_is_match(t);
                    const bool other = have & !indel & !ism;
                    const bool atend = !have;
                    const bool ev = act & ((in_blk & (ism | other | atend)) | other | atend);
                    const bool take = act & !ev;
                    const bool memb = take & indel & (L > 0);  // add_del / add_ins (:73-85, len > 0 only)
                    const bool open = memb & !in_blk;
                    blk_ref = open ? ref_head : blk_ref;
                    blk_read = open ? read_head : blk_read;
                    in_blk = in_blk | memb;
                    del += (memb & (t == OP_D)) ? L : 0;
                    ins += (memb & (t == OP_I)) ? L : 0;
                    const bool tm = take & ism;  // add_match (:150-153)
                    msince += (tm & pend) ? L : 0;
                    match += (tm & !pend) ? L : 0;
                    read_head += (take & b_read_cons(t)) ? L : 0;
                    ref_head += (take & b_ref_cons(t)) ? L : 0;
                    k += take ? 1 : 0;
                    ev_t = ev ? t : ev_t;
                    ev_L = ev ? L : ev_L;
                    ev_other = ev ? other : ev_other;
                    ev_end = ev ? atend : ev_end;
                    stop = stop | ev;
                }
                // the event
                const bool evl = !fin;             // lanes with an event
                const bool endc = evl & in_blk;    // end_indel (:101-148)
                const bool flushing = evl & (ev_other | ev_end);
                const int wl = ext ? wl_ext : wl0 + k;
                auto resolve = [&](bool on) {  // end_indel's emission for the pending cluster (:132-147)
                    int h = lane_probe_finish(pr, on, sref, shift_ref_len, rd, probes);
                    h = rd.miss ? 0 : h;
                    const int sh = wv::imin(p_match, h);  // actual_shift_len (:132)
                    lane_push<false, ST, H16>(o, on & (p_match - sh > 0), OP_M, p_match - sh, wl);
                    lane_push<false, ST, H16>(o, on & (p_ins > 0), OP_I, p_ins, wl);
                    lane_push<false, ST, H16>(o, on & (p_del > 0), OP_D, p_del, wl);
                    match = on ? sh + msince : match;
                    msince = on ? 0 : msince;
                    pend = pend & !on;
                };
                // Pass 0: the pending cluster first (every event needs the builder's match run), then this cluster's probe is armed -- the
                // match run is exact there, nothing is pending; its loads go out at the top of the next round.  Pass 1 (rare): a cluster
                // directly in front of a flushing op or of the end has no ops to hide its probe under: loads and resolution at once.  One
                // copy of the resolving code for both (the probe's slow paths are large).
#pragma nounroll
                for (int pass = 0; pass < 2; ++pass) {
                    const bool res = (pass == 0 ? evl : flushing) & pend;
                    if (wv::ballot(res) != 0ull) {
                        if (pass == 1) lane_probe_load(pr, res, sref, shift_ref_len, rd, (const uint8_t *)plo_safe_words);
                        resolve(res);
                    }
                    if (pass == 1) break;
                    if (wv::ballot(endc) != 0ull) {
                        lane_probe_arm(pr, endc, shift_ref_len, blk_ref, del, rd, blk_read, ins, match, panic);
                        p_match = endc ? match : p_match;
                        p_ins = endc ? ins : p_ins;
                        p_del = endc ? del : p_del;
                        ins = endc ? 0 : ins;
                        del = endc ? 0 : del;
                        in_blk = in_blk & !endc;
                        pend = pend | endc;
                    }
                    if (wv::ballot(flushing & pend) == 0ull) break;
                }
                if (wv::ballot(flushing) != 0ull) {  // add_other (:155-165); at the end: get_cigar()'s add_other(None) (:54-60)
                    lane_push<false, ST, H16>(o, flushing & (match > 0), OP_M, match, wl);
                    match = flushing ? 0 : match;
                    const bool oth = flushing & ev_other;
                    lane_push<true, ST, H16>(o, oth, ev_t, ev_L, wl + 1);
                    read_head += (oth & b_read_cons(ev_t)) ? ev_L : 0;
                    ref_head += (oth & b_ref_cons(ev_t)) ? ev_L : 0;
                    k += oth ? 1 : 0;
                    fin = fin | (flushing & ev_end);
                }
            }
            PLO_MARK("SHIFT LOOP END");
            wr_finish(o, shift_on, gap, ext ? wl_ext : wl0 + n);  // :35-38 clean_up_cigar_edge_indels + compress
            if (shift_on) {
                if constexpr (STATS) algo += 2u * (unsigned)probes;
                n = o.no;
                cur_off = gap;
                ext = false;
                pos += o.lead_shift;
                ovf = ovf | o.ovf;
            }
        }
        if (act0 && (panic || rd.miss)) {  // absent bases (sparse batches) come first: what the probes saw then is not the read
            status = rd.miss ? PLO_ITEM_NEED_BASES : PLO_ITEM_PANIC;
            alive = false;
        }
        wv::sync();
        PLO_LT(2)

        // ---- LIFTOVER (src/liftover_read_alignment.rs:35-223) ---------------------------------------------------------------------
        // One iteration = one (op x block) piece (update_ref2_cigar_segment, :35-133) or one copied op, straight-line.  Block
        // cursor: {kb, vb} the block that holds block_pos (bvalid: there is one), {kn, vn} the next entry of the map, {kf, vf}
        // the one after it, requested at the previous crossing.
        bool pairs = true;
        if (stages & PLO_STAGE_LIFTOVER) {
            const bool lo_on = alive && !ovf;
            if constexpr (STATS) {
                if (lo_on) {
                    const int nb = kv1 - kv0;
                    const int lg = nb > 1 ? 32 - __builtin_clz((unsigned)(nb - 1)) : 0;  // ceil(log2(nb))
                    algo += 16u * (unsigned)(W1 - W0) + 8u * (unsigned)lg;
                }
            }
            LaneOut o;
            wr_open(o, 0);
            rd_fill(lo_on, cur_off);
            int k = 0;
            bool in_op = false, ism = false, bvalid = false, has_start = false, has_end = false;
            int t = 0, seg_start = pos, seg_end = 0, block_pos = 0, r2s = 0, r2e = 0;
            int kb = 0, vb = NONE32, kn = IMAX, vn = NONE32, kf = IMAX, vf = NONE32;
            int ni = W0 + 2;  // index of the entry to request at the next crossing
            // entry `idx` of the block map for the lanes `on`: from the staged copy, or (items outside it) from global memory.
            // ALL_LDS: every lane's entries are staged (nearly every group: the items of a group are neighbours on a contig) -- the loop
            // body is then ONE basic block: no `any lane outside` test, no global load, and none of the lane-mask merges the compiler
            // puts at the join of a divergent branch (three scalar instructions per loop-carried flag, profiles/r05_liftover_loop.s).
            auto run = [&](auto all_lds_c) {
                constexpr bool ALL_LDS = decltype(all_lds_c)::value;
                auto kv_fetch = [&](bool on, int idx, int &key, int &val) {
                    if (kvs != nullptr) {
                        // (only what was staged: the cursor's look-ahead may ask for the entry one past the item's own range)
                        // (ALL_LDS: every request lies in [W0, min(kv1, W1 + 2)) -- a crossing needs a key <= block_pos < pos1 + ref_len, so at most
                        // W1 - W0 of them happen and the last one asks for entry W1 + 1 -- which is what kv_lds says is staged)
                        const bool l = ALL_LDS ? on : (on & kv_lds & ((unsigned)(idx - kvs_base) < (unsigned)kvs_cnt));
#ifdef PLO_EMULATOR
                        if (ALL_LDS && on && (unsigned)(idx - kvs_base) >= (unsigned)kvs_cnt) {
                            fprintf(stderr, "lane_tile: block-map entry %d outside the staged range [%d, %d)\n", idx, kvs_base, kvs_base + kvs_cnt);
                            abort();
                        }
#endif
                        const uint32_t *q = kvs + 2 * (l ? idx - kvs_base : 0);
                        const int lk = (int)q[0], lv = (int)q[1];
                        key = l ? lk : key;
                        val = l ? lv : val;
                        on = on & !l;
                    }
                    if constexpr (!ALL_LDS) {
                        const bool gl = on;
                        if (wv::ballot(gl) != 0ull) {
                            if (gl) {
                                const KV e = ix.kv[idx];
                                key = e.key;
                                val = e.val;
#ifdef PLO_EMULATOR
                                g_emu_kv.global_kv += 1;
#endif
                            }
                        }
                    }
                };
                kv_fetch(lo_on & (W0 < kv1), W0, kn, vn);
                kv_fetch(lo_on & (W0 + 1 < kv1), W0 + 1, kf, vf);
                PLO_MARK("LIFTOVER LOOP BEGIN");
#ifdef PLO_EMULATOR
                unsigned emu_trips = 0;
#endif
                for (unsigned long long bm; (bm = wv::ballot(lo_on & ((k < n) | in_op))) != 0ull;) {
                    PLO_LC(7, 1)
#ifdef PLO_EMULATOR
                    // a walk that does not end (tests/emu/: a wrong comparison in this loop) is reported, not waited for: every trip emits or
                    // consumes something, so a group is through long before EMU_LIFT_TRIPS; the harness answers 2 (CNT_ERROR)
                    if (++emu_trips > EMU_LIFT_TRIPS) {
                        if (lane == 0) wv::atomic_add_global(&wk.counters[CNT_ERROR], 1ull);
                        break;
                    }
#endif
                    if constexpr (STATS) {
                        ctx.u_act += (unsigned)__builtin_popcountll(bm);
                        ctx.u_trips += 1;
                    }
                    // the next op, unless one is being cut into pieces
                    const bool fetch = lo_on & !in_op & (k < n);
                    wr_room(o, lo_on, 0);
                    rd_need(k, fetch, lo_on);
                    const uint32_t c = rd_at(k, fetch);
                    k += fetch ? 1 : 0;
                    const int tf = op_type(c), Lf = op_len(c);
                    const bool copy = fetch & (((0x32u >> tf) & 1u) != 0u);  // I S H: :157-160 copied through; Pad (:213) emits nothing
                    const bool start = fetch & b_ref_cons(tf) & (Lf > 0);
                    // (t: what a piece of this op in a mapped block is written as, :102-109 -- D and N as themselves, the matches as M)
                    t = start ? ((unsigned)(tf - (int)OP_D) < 2u ? tf : (int)OP_M) : t;
                    ism = start ? b_is_match(tf) : ism;
                    seg_end = start ? seg_start + Lf : seg_end;
                    block_pos = start ? seg_start : block_pos;
                    in_op = in_op | start;
                    // the piece starts in the next block (get_ref_range walks on, read_to_ref_map.rs:79-84)
                    const bool adv = in_op & (kn <= block_pos);
                    int fk = IMAX, fv = NONE32;
                    kv_fetch(adv & (ni < kv1), ni, fk, fv);  // (used at the end of the iteration)
                    kb = adv ? kn : kb;
                    vb = adv ? vn : vb;
                    bvalid = bvalid | adv;
                    kn = adv ? kf : kn;
                    vn = adv ? vf : vn;
                    ni += adv ? 1 : 0;
                    // (kn <= block_pos still: the shift stage moved the start past another key; the walk goes on next iteration)
                    const bool piece = in_op & (kn > block_pos);
                    const int pend = wv::imin(seg_end, kn);  // :62-67
                    const int plen = pend - block_pos;
                    const bool mapped = bvalid & (vb != NONE32);
                    const bool mp = piece & mapped;
                    const bool set_start = mp & ism & !has_start;  // :84-88
                    r2s = set_start ? wrap_add(vb, block_pos - kb) : r2s;
                    has_start = has_start | set_start;
                    const int d = wrap_add(vb, -r2e);  // :91-96 (wrapping: vb is NONE32 where the piece is not mapped, and then unused)
                    // ONE writer call per trip.  A piece that enters its block behind a jump of the reference (:91-96) takes two trips:
                    // the first emits the deletion D(d) and moves ref2_end_pos up to the block's start, so that the second -- same op,
                    // same block, nothing else has moved -- finds d == 0 and emits the piece itself.  (The jump is live in about one
                    // trip in twenty; the second writer call it used to have cost every trip a quarter of its vector instructions.)
                    const bool e0 = mp & has_end & (d > 0) & has_start;
                    has_end = has_end | mp;
                    const bool go = piece & !e0;  // the piece is consumed in this trip
                    r2e = mp ? wrap_add(vb, e0 ? 0 : pend - kb) : r2e;  // :98-100
                    // :102-109 mapped piece | :111-115 insertion over an unmapped block | :117-123 soft clip before the first block
                    const bool e1p = go & (mapped ? (ism | has_start) : ism);
                    const int t1p = mapped ? t : (bvalid ? (int)OP_I : (int)OP_S);
                    block_pos = go ? pend : block_pos;
                    const bool done = go & (pend >= seg_end);
                    in_op = in_op & !done;
                    seg_start = done ? seg_end : seg_start;
                    const int wl = ext ? W : cur_off + k;  // ops below R[cur_off + k] have been read
                    lane_push<false, ST, H16>(o, e0 | copy | e1p, e0 ? (int)OP_D : (copy ? tf : t1p), e0 ? d : (copy ? Lf : plen), wl);
                    kf = adv ? fk : kf;  // the entry after next (kv_fetch above)
                    vf = adv ? fv : vf;
                }
            };
#ifdef PLO_EMULATOR
            {
                const bool any_on = wv::ballot(lo_on) != 0ull, any_out = wv::ballot(lo_on & !kv_lds) != 0ull;
                if (lane == 0 && kvs != nullptr && any_on) (any_out ? g_emu_kv.mixed : g_emu_kv.all_lds) += 1;
            }
#endif
            if (kvs != nullptr && wv::ballot(lo_on & !kv_lds) == 0ull) run(std::true_type{});
            else run(std::false_type{});
            PLO_MARK("LIFTOVER LOOP END");
            PLO_LT(3)
            wr_finish(o, lo_on, 0, ext ? W : cur_off + n);  // :219-220
            if (lo_on) {
                ovf = ovf | o.ovf;
                if (!has_start) {  // :218 ref2_start_pos.map(...) on None
                    status = PLO_ITEM_NO_LIFTOVER;
                    alive = false;
                } else {
                    n = o.no;
                    nops = o.no - o.extra;
                    cur_off = 0;
                    ext = false;
                    pos = r2s + o.lead_shift;  // :221
                }
                pairs = o.pairs;
            }
            wv::sync();
        }

        PLO_LT(4)
        // ---- LENGTH CHECK (src/read_alignment_scanner.rs:204-229), decided from the descriptors (see lift_tile) ----
        bool simp = alive && !ovf;
        if ((stages & PLO_STAGE_LENCHECK) && simp && len_bad) {
            status = PLO_ITEM_LEN_MISMATCH;
            simp = false;
        }

        // ---- SIMPLIFY (src/simplify_alignment_indels.rs:5-156), in place ---------------------------------------------------------
        // On a CIGAR the liftover has just cleaned and compressed the function is the identity unless some indel cluster has more
        // than one op (see lift_tile); such items -- most -- take no part.
        if (stages & PLO_STAGE_SIMPLIFY) {
            const bool s_on = simp && (!(stages & PLO_STAGE_LIFTOVER) || pairs);
            if (wv::ballot(s_on) != 0ull) {
                unsigned long long chrom_ref = 0;
                int chrom_ref_len = 0;
                if (s_on) {
                    chrom_ref = wk.d.chrom_ref[g];
                    chrom_ref_len = wk.d.chrom_ref_len[g];
                }
                const uint8_t *const cref = (const uint8_t *)(uintptr_t)chrom_ref;
                LaneOut o;
                wr_open(o, 0);
                rd_fill(s_on, cur_off);
                int ref_head = pos, read_head = 0, del = 0, ins = 0, blk_ref = 0, blk_read = 0, cmp = 0;
                bool in_blk = false, spanic = false, zero_m = false;
                // (Measured and dropped: the event-aligned walk of the shift stage here -- every lane scanning to the end of its next
                // cluster, end_indel for all of them together.  5 % slower on the indel-dense stress workload, 2.6 % on wgs30x: the
                // clusters that need base comparisons are few, and the rest of end_indel is cheaper than the second loop level.)
                const int nmax = wv::reduce_max(s_on ? n : 0);
                for (int k = 0; k <= nmax; ++k) {
                    const bool valid = s_on & (k < n);
                    const bool atend = s_on & (k == n);
                    wr_room(o, s_on, 0);
                    rd_need(k, valid, s_on);
                    const uint32_t c = rd_at(k, valid);
                    const int t = op_type(c), L = op_len(c);
                    const bool indel = valid & b_is_indel(t);
                    const int wl = cur_off + wv::imin(k + 1, n);
                    const bool endc = in_blk & !indel & (valid | atend);
                    if (wv::ballot(endc) != 0ull) {  // CigarBlockInfo::end_indel (:35-111)
                        // :41-44 one kind only (nothing for 0 / 0); :45-48 1 / 1 -> M(1); else the base comparisons
                        const bool single = endc & ((del == 0) | (ins == 0));
                        const bool one_one = endc & (del == 1) & (ins == 1);
                        const bool cplx = endc & !single & !one_one;
                        int pre = one_one ? 1 : 0, post = 0;
                        if (wv::ballot(cplx) != 0ull) {
                            if (cplx) {
                                if (blk_ref < 0 || blk_ref + del - 1 >= chrom_ref_len || blk_read + ins - 1 >= rd.len) {
                                    spanic = true;  // slice index out of bounds: the reference panics (:58-60)
                                    del = 0;
                                    ins = 0;
                                } else {
                                    // :55-68 trailing bases shared by the inserted and the deleted sequence, then :71-85 leading ones
                                    post = match_run_back(cref, chrom_ref_len, blk_ref + del, rd, blk_read + ins, wv::imin(del, ins), cmp);
                                    del -= post;
                                    ins -= post;
                                    pre = match_run_fwd(cref, chrom_ref_len, blk_ref, rd, blk_read, wv::imin(del, ins), cmp);
                                    del -= pre;
                                    ins -= pre;
                                    if (del == 1 && ins == 1) {  // :88-92
                                        del = 0;
                                        ins = 0;
                                        ++post;
                                    }
                                }
                            }
                        }
                        // :101-104 M(pre) I D M(post).  A cluster of one kind (most) emits that one op: the M ops and the second
                        // kind only where some lane has them
                        const bool emit_id = endc & !one_one;
                        const bool both = wv::ballot(endc & !single) != 0ull;
                        if (both) lane_push<false, ST, H16>(o, endc & (pre > 0), OP_M, pre, wl);
                        {
                            const bool first_d = emit_id & (ins == 0);  // (then the one op is the D, if anything)
                            lane_push<false, ST, H16>(o, emit_id & ((first_d ? del : ins) > 0), first_d ? (int)OP_D : (int)OP_I, first_d ? del : ins, wl);
                            if (both) {
                                lane_push<false, ST, H16>(o, emit_id & !first_d & (del > 0), OP_D, del, wl);
                                lane_push<false, ST, H16>(o, endc & (post > 0), OP_M, post, wl);
                            }
                        }
                        del = endc ? 0 : del;
                        ins = endc ? 0 : ins;
                        in_blk = in_blk & !endc;
                    }
                    const bool open = indel & !in_blk;  // _add_indel (:16-22)
                    blk_ref = open ? ref_head : blk_ref;
                    blk_read = open ? read_head : blk_read;
                    in_blk = in_blk | indel;
                    del += (indel & (t == OP_D)) ? L : 0;
                    ins += (indel & (t == OP_I)) ? L : 0;
                    const bool cp = valid & !indel;
                    zero_m = zero_m | (cp & b_is_match(t) & (L == 0));  // an edge mark the writer would not see (LaneOut)
                    lane_push<true, ST, H16>(o, cp, t, L, wl);  // :144-147
                    read_head += (valid & b_read_cons(t)) ? L : 0;
                    ref_head += (valid & b_ref_cons(t)) ? L : 0;
                }
                wr_finish(o, s_on, 0, cur_off + n);  // :153-154
                if (s_on) {
                    if constexpr (STATS) algo += 2u * (unsigned)cmp;
                    ovf = ovf | o.ovf | zero_m;
                    n = o.no;
                    nops = o.no - o.extra;
                    cur_off = 0;
                    pos += o.lead_shift;  // :155
                    if (rd.miss || spanic) {
                        status = rd.miss ? PLO_ITEM_NEED_BASES : PLO_ITEM_PANIC;
                        alive = false;
                    }
                }
                wv::sync();
            }
        }

        PLO_LT(5)
        // ---- OUTPUT ----------------------------------------------------------------------------------------------------------------
        {   // regions that overflowed: the wave-cooperative code takes the item (retry list)
            const bool re = act0 && ovf;
            const unsigned long long om = wv::ballot(re);
            if (om != 0ull) {
                int slot = 0;
                if (lane == 0) slot = (int)wv::atomic_add_global(&wk.counters[CNT_NRETRY], (unsigned long long)__builtin_popcountll(om));
                slot = wv::bcast_first(slot);
                if (re) {
                    wk.retry_list[slot + __builtin_popcountll(om & ((1ull << lane) - 1ull))] = g;
                    wk.status[g] = (uint8_t)ITEM_NEED_BIG;
                }
            }
        }
        const bool done = act0 && !ovf;
        const bool emit_cigar = done && (status == PLO_ITEM_LIFTED || status == PLO_ITEM_LEN_MISMATCH);
        const int oc = emit_cigar ? (H16 ? nops : n) : 0;
        const int inco = wv::scan_add(oc);
        const int oS = inco - oc;
        const int total = wv::bcast_last(inco);
        if ((unsigned long long)total > ctx.slab_left) {  // wave-uniform: reserve a new slab
            const unsigned long long want = (unsigned long long)total > SLAB_OPS ? (unsigned long long)total : SLAB_OPS;
            unsigned long long nb = 0;
            if (lane == 0) nb = wv::atomic_add_global(&wk.counters[CNT_CIGAR], want) + wk.slab_offset;
            ctx.slab_base = wv::bcast_first(nb);
            ctx.slab_left = want;
        }
        const unsigned long long gbase = ctx.slab_base;
        ctx.slab_base += (unsigned long long)total;
        ctx.slab_left -= (unsigned long long)total;
        const bool fits = gbase + (unsigned long long)total <= wk.out_cap;
        if (!fits && lane == 0) wv::atomic_add_global(&wk.counters[CNT_OVERFLOW], 1ull);
        if constexpr (H16) {
            // halfwords -> 32-bit ops.  No op of the group in chunks (three groups in four): four halfwords, one 16-byte store; else
            // equal neighbours -- the writer leaves no others than the chunks of one op -- are summed on the way
            const int nh = (emit_cigar && fits) ? n : 0;
            const int nhmax = wv::reduce_max(nh);
            uint32_t *const dst = wk.out_cigar + gbase + (unsigned long long)oS;
            const uint16_t *const srcp = R16 + cur_off;
            if (wv::ballot(nh != (fits ? oc : 0)) == 0ull) {
                for (int k = 0; k < nhmax; k += 4) {
                    if (k + 3 < nh) {
                        Ops4 v;
                        v.x = h16_dec(srcp[k]);
                        v.y = h16_dec(srcp[k + 1]);
                        v.z = h16_dec(srcp[k + 2]);
                        v.w = h16_dec(srcp[k + 3]);
                        *(PLO_GLOBAL Ops4 *)(dst + k) = v;
                    } else {
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            if (k + j < nh) dst[k + j] = h16_dec(srcp[k + j]);
                    }
                }
            } else {
                uint32_t run = 0;
                int w = 0;
                for (int k = 0; k < nhmax; ++k) {
                    const bool act = k < nh;
                    const uint32_t c = h16_dec(srcp[act ? k : 0]);
                    const bool same = act & (run >= 16u) & (((c ^ run) & 15u) == 0u);
                    const bool fl = act & !same & (run >= 16u);
                    if (fl) dst[w] = run;
                    w += fl ? 1 : 0;
                    run = same ? run + (c & ~15u) : (act ? c : run);
                }
                if ((nh > 0) & (run >= 16u)) dst[w] = run;
            }
        } else {
            const int ocmax = wv::reduce_max(fits ? oc : 0);
            uint32_t *const dst = wk.out_cigar + gbase + (unsigned long long)oS;
            const uint32_t *const srcp = (WIN ? win.G : R) + cur_off;
            for (int k = 0; k < ocmax; k += 4) {  // 16 bytes per store and lane
                if (fits && k + 3 < oc) {
                    Ops4 v;
                    v.x = srcp[k];
                    v.y = srcp[k + 1];
                    v.z = srcp[k + 2];
                    v.w = srcp[k + 3];
                    *(PLO_GLOBAL Ops4 *)(dst + k) = v;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (fits && k + j < oc) dst[k + j] = srcp[k + j];
                }
            }
        }
        if (done) {
            if (status == PLO_ITEM_NEED_BASES) wk.miss_list[wv::atomic_add_global(&wk.counters[CNT_NMISS], 1ull)] = g;  // rare
            wk.status[g] = (uint8_t)status;
            wk.pos[g] = emit_cigar ? (int64_t)pos : (int64_t)-1;
            wk.cig_off[g] = emit_cigar ? gbase + (unsigned long long)oS : 0ull;
            wk.cig_len[g] = (uint32_t)oc;
            if constexpr (STATS) ctx.algo_bytes += algo + 40u + 4u * (unsigned)n_in + 24u + 4u * (unsigned)oc;
            ctx.in_ops += (unsigned)n_in;  // (two adds per group: plo_timing::n_in_ops / n_out_ops are always reported)
            ctx.out_ops += (unsigned)oc;
        }
        PLO_LT(6)
        PLO_LC(11, 1)
    }
#undef PLO_LT
#undef PLO_LC
}

// Persistent wave over the groups of the lane classes: class c (0: no shift stage, 1: shift stage) occupies positions
// [c_begin, c_end) of the class order and is cut into groups of `gs` (64; 32, 16 or 8 when the batch has too few items to give
// every resident wave a group of 64: a group runs as long as its longest item whatever its size, so few items are better
// spread over many waves) from its start, so that groups are strand-homogeneous.
// Group indices: class 0 first.  The item indices of the next group are fetched one group ahead.
// (Measured and dropped: the class order sorted by item weight inside chunks of 4 .. 32 groups, so that a group does not wait for
// its one longest CIGAR -- a quarter fewer loop trips per group, but 5-15 % slower overall: neighbours in the batch share
// descriptor, CIGAR and block-map cache lines, and a group of scattered items gives that up.  k_chunk_sort's windows of 128 items
// are what survived of it.  Also measured and dropped: the groups dealt out by atomic queues, one per XCD, instead of the fixed
// slots below -- 1.30 ms either way on wgs30x, the waves' loads are even enough, and a small batch pays for the atomics.)
// DYNAMIC DEALING (round 6): with wk.lane_ticket set, a wave takes its first wk.lane_static_rounds groups by the fixed slots above and every
// further one from a device-wide ticket counter, one group ahead (the ticket for the next group is asked for before this group is lifted
// and looked at after it).  tools/wave_timeline.py on wgs30x: with fixed slots the 3 072 waves start within half a microsecond and end
// between 800 and 1 380 us -- a quarter of all wave-slots of the launch idle behind waves that drew cheap groups (half the groups have no shift
// stage and take half as long; the last round is a partial one).  The earlier attempt with one queue per XCD (round 4) kept the XCDs' unequal
// shares; one counter for the chip levels them too.
// `base`: class-order position of the first item (0; a launch over one class only starts at that class)
template <bool SP, bool NOSHIFT = false, bool STATS = true, bool H16 = false>
PLO_DEV void lane_tiles_persistent(const DevIndex &ix, const DevBatch &bt, const DevWork &wk, uint32_t stages, uint32_t first, uint32_t stride,
                                   uint32_t n0, uint32_t n1, uint32_t gs, uint32_t *lds, int capw, WaveCtx &ctx, uint32_t base = 0, int kvs_n = LANE_KVS) {
    const uint32_t lane = (uint32_t)wv::lane();
    // groups: cut by LDS budget (k_chunk_sort's list, wk.lane_groups) or fixed: `gs` items each from the start of either class
    const bool listed = wk.lane_groups != nullptr;
    const uint32_t t0 = (n0 + gs - 1u) / gs, t1 = (n1 + gs - 1u) / gs;
    uint32_t n_groups = listed ? wv::bcast_first(*wk.lane_n_groups) : t0 + t1;
    if (listed && n_groups > wk.lane_groups_cap) {  // (k_chunk_sort did not write the groups beyond the list's capacity)
        if (first == 0u && lane == 0u) wv::atomic_add_global(&wk.counters[CNT_ERROR], 1ull);
        n_groups = wk.lane_groups_cap;
    }
    auto group = [&](uint32_t t, uint32_t &lo, uint32_t &hi) {
        if (listed) {
            lo = wk.lane_groups[2 * t];
            hi = lo + wk.lane_groups[2 * t + 1];
        } else {
            // the two classes interleaved (group 0 of the first, group 0 of the second, group 1 of the first, ...; the longer class's rest
            // behind): the groups with the shift stage are the ones whose probes load the memory system, and a kernel that runs all the
            // others first and all of them last has every wave probing at the same time
            bool second;
            uint32_t idx;
            if (wk.lane_tail_rounds) {
                // (round 6) the last groups dealt are groups WITHOUT the shift stage -- half as long as the others: what the waves still have to
                // do when the tickets run out is what the launch waits for (tools/group_log.py: with the longer class's surplus at the end the
                // last 1 800 groups of wgs30x were all of the expensive kind and took 120-160 us each) -- and the classes are mixed in
                // proportion in front of them instead of one to one with the longer one's rest behind
                const uint32_t keep = wk.lane_tail_rounds * stride, tail = t0 < keep ? t0 : keep;
                const uint32_t head0 = t0 - tail, head = head0 + t1;
                if (t >= head) {
                    second = false;
                    idx = head0 + (t - head);
                } else {
                    const uint32_t r0 = (uint32_t)(((unsigned long long)t * t1) / head), r1 = (uint32_t)(((unsigned long long)(t + 1u) * t1) / head);
                    second = r1 > r0;  // (r0 groups of the second class lie in front of t)
                    idx = second ? r0 : t - r0;
                }
            } else {
                const uint32_t m = t0 < t1 ? t0 : t1;
                second = t < 2u * m ? (t & 1u) != 0u : t1 > t0;
                idx = t < 2u * m ? t >> 1 : t - m;
            }
            if (!second) {
                lo = idx * gs;
                hi = lo + gs < n0 ? lo + gs : n0;
            } else {
                lo = n0 + idx * gs;
                hi = lo + gs < n0 + n1 ? lo + gs : n0 + n1;
            }
            lo += base;
            hi += base;
        }
    };
    // round j: wave w takes group j * stride + (w + j) % stride -- the waves rotate through the slots from round to round, so that
    // a wave does not keep drawing the longer (or the shorter) half of every sorted window (k_chunk_sort) when the number of waves
    // is even
    auto slot = [&](uint32_t j) { return j * stride + (first + j) % stride; };
    const bool dyn = wk.lane_ticket != nullptr;
    const uint32_t n_static = dyn ? (wk.lane_static_rounds ? wk.lane_static_rounds : 1u) : 0xffffffffu;  // rounds by fixed slots
    const uint32_t t_base = dyn ? n_static * stride : 0u;  // tickets count from the first group no fixed slot covers
    // One call site of lane_tile (the kernel's code is large: a second copy costs instruction-cache misses and compile time).  Software
    // pipeline: the item indices of the next group are fetched while this one is lifted when its index is known (fixed slots); a
    // ticket is asked for before the group and looked at after it (the atomic's round trip runs under the group's own loads).
    uint32_t t = slot(0), lo = 0, hi = 0, g = 0;
    bool have = t < n_groups;
    if (have) {
        group(t, lo, hi);
        g = lo + lane < hi ? wk.perm[lo + lane] : 0u;
    }
    for (uint32_t j = 0; have; ++j) {
        const bool next_fixed = j + 1u < n_static;
        uint32_t tn = next_fixed ? slot(j + 1u) : 0xffffffffu, lon = 0, hin = 0, gn = 0, ticket = 0;
        if (next_fixed) {
            if (tn < n_groups) {
                group(tn, lon, hin);
                gn = lon + lane < hin ? wk.perm[lon + lane] : 0u;
            }
        } else if (dyn) {
            if (lane == 0u) ticket = wv::atomic_add_global(wk.lane_ticket, 1u);
        }
#ifdef PLO_PHASE_TIMING
        const long long tg0 = wv::realtime(), lt0 = ctx.tph[7], sr0 = ctx.tph[8], sc0 = ctx.tph[9], rd0 = ctx.tph[11];
#endif
        lane_tile<SP, false, NOSHIFT, STATS, H16>(ix, bt, wk, stages, lo, (int)(hi - lo), lds, capw, 0, ctx, wk.perm, true, g, nullptr, lds + capw, kvs_n);
        wv::sync();
#ifdef PLO_PHASE_TIMING
        {
            const long long dt = wv::realtime() - tg0;
            ctx.g_n += 1;
            ctx.g_max = dt > ctx.g_max ? dt : ctx.g_max;
            ctx.g_prev = ctx.g_last;
            ctx.g_last = dt;
            ctx.g_last_begin = tg0;
            // the group's record behind the waves' slots (tools/group_log.py): ticks, trip counts, rounds, where it ran
            if (lane == 0u && t < 49152u) {
                unsigned long long *r = wk.wave_stats + (size_t)8192 * STAT_WORDS + (size_t)t * 4;
                r[0] = (unsigned long long)dt | ((unsigned long long)(tg0 - ctx.t_begin) << 32);
                r[1] = (unsigned long long)(ctx.tph[7] - lt0) | ((unsigned long long)(ctx.tph[8] - sr0) << 32);
                r[2] = (unsigned long long)(ctx.tph[9] - sc0) | ((unsigned long long)(ctx.tph[11] - rd0) << 32);
                r[3] = (unsigned long long)lo | ((unsigned long long)(hi - lo) << 32) | ((unsigned long long)first << 44);
            }
        }
#endif
        if (!next_fixed && dyn) {
            const uint32_t k = wv::bcast_first(ticket);
            tn = k < n_groups ? k + t_base : 0xffffffffu;  // (k < n_groups first: the sum must not wrap)
            if (tn < n_groups) {
                group(tn, lon, hin);
                gn = lon + lane < hin ? wk.perm[lon + lane] : 0u;
            }
        }
        have = tn < n_groups;
        t = tn;
        lo = lon;
        hi = hin;
        g = gn;
    }
}

// Persistent wave over the HEAVY items (classes 2 and 3: positions [lo, mid) and [mid, hi) of the class order), `per` items per
// group (<= 64: few heavy items are spread over more waves, at fewer lanes each, so that they still fill the chip), every lane with
// a region of `stride` dwords in the wave's global scratch `regions` and its windows in `windows` (64 x LANE_WIN_DWORDS dwords of LDS).
template <bool SP>
PLO_DEV void lane_heavy_persistent(const DevIndex &ix, const DevBatch &bt, const DevWork &wk, uint32_t stages, uint32_t first, uint32_t step,
                                   uint32_t lo, uint32_t mid, uint32_t hi, uint32_t per, uint32_t *windows, uint32_t *regions, int stride, WaveCtx &ctx) {
    const uint32_t t0 = (mid - lo + per - 1) / per, t1 = (hi - mid + per - 1) / per;
    for (uint32_t t = first; t < t0 + t1; t += step) {
        const bool c1 = t >= t0;
        const uint32_t b = c1 ? mid + (t - t0) * per : lo + t * per, e = c1 ? hi : mid;
        const uint32_t n = e - b < per ? e - b : per;
        lane_tile<SP, true>(ix, bt, wk, stages, b, (int)n, windows, 0x7fffffff, stride, ctx, wk.perm, false, 0u, regions, windows + 64 * LANE_WIN_DWORDS);
        wv::sync();
    }
}

}  // namespace plo
