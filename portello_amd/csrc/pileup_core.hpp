// pileup_core.hpp -- the allele pileup of the output records on the device (plo_pileup_*): which reference bases carry non-reference evidence.
// The rule is stated in include/portello_liftover.h ("Allele pileup and candidate sites").  In short: a pileup object holds one int32 array
// with PILEUP_CHANNELS = 8 counters per reference base (A C G T N DEL INS CLIP; 32 contiguous, 32-byte aligned bytes), over the whole of
// every chromosome or over at most one region [beg, end) per chromosome.  A counted record (refID >= 0, pos >= 0, FLAG & exclude == 0; depth's
// rule) whose real CIGAR consumes reference is walked from pos: every MISMATCHING pair of an M / = / X op (plo_nm_dev's pair rule, whatever
// the op's own code says) adds 1 to the channel of the read's base at its reference base, a D adds 1 to DEL at its first base, an I to INS
// and an S to CLIP at max(rf - 1, pos).  Only events are counted: the reference-matching count at a base is depth - (A + C + G + T + N).
// An event outside its chromosome's region is dropped.
//   check  (a wave per record): depth's checks and plan word (depth_check_rules), then kind 9 -- bases and qualities leave the record -- and
//          kind 10 -- the real CIGAR's read length differs from l_seq, the read advances summed a lane each.  A record that consumes no
//          reference gets a plan of 0 ops: nothing to add.
//   add    (a wave per record): reads the check's word first -- a refused call adds nothing.  The walk is aln_walk.hpp's over a record's view
//          (aln_open_record, aln_step_bytes: a record lies at any byte address): the ops 64 a step, the lane that owns a D, I or S issues
//          its one add; the M / = / X ops are cut into their 16-byte pieces, dealt 64 a trip, nm_piece_t<true> gives a piece's mismatch bits
//          and the lane issues one int32 atomic add of device scope, without return, per set bit.  The events issued inside the regions are
//          counted per lane, reduced per wave and added with one atomic per wave.
//   sites  tiles of PLO_PILEUP_TILE bases, a wave each: counted per tile, the 64-bit scan of records_core.hpp, emit.  A lane takes a base: its
//          32 bytes as two 16-byte loads, the maximum over the masked channels, the depth from a FINISHED depth object's array.
// The file has two parts, like depth_core.hpp: plain C++ for the rule of one record by one thread (pileup_add_scalar), the layout and the
// site rule, and the wave part.  The same functions run under the CPU emulator (tests/emu/emu_pileup.cpp), there with a small PLO_PILEUP_TILE.
#pragma once
#include <stdint.h>

#include "index_core.hpp"

#ifndef PLO_PILEUP_TILE
#define PLO_PILEUP_TILE 1024
#endif

namespace plo {

constexpr int PILEUP_CHANNELS = 8;
enum { PILEUP_A = 0, PILEUP_C = 1, PILEUP_G = 2, PILEUP_T = 3, PILEUP_N = 4, PILEUP_DEL = 5, PILEUP_INS = 6, PILEUP_CLIP = 7 };
constexpr unsigned long long PILEUP_TILE = PLO_PILEUP_TILE;
static_assert(PLO_PILEUP_TILE >= 1, "a tile holds a base at the least");
// what the lowest offending record broke, behind depth's kinds (1 .. 8)
enum { PILEUP_ERR_SEQ = 9,     // the bases and qualities leave the record
       PILEUP_ERR_LSEQ = 10 };  // a counted record whose real CIGAR's read length differs from l_seq

struct PileupRegion {  // plo_pileup_region
    int32_t ref_id, beg, end;
};
struct PileupSite {  // plo_pileup_site
    int32_t ref_id, pos, depth;
    uint8_t ref_base, pad[3];
    int32_t count[PILEUP_CHANNELS];
};
static_assert(sizeof(PileupSite) == 48, "plo_pileup_site is 48 bytes");

// the pair rule as it is stated: c1 the read's 4-bit code, ch the reference byte
PLO_HD unsigned pileup_ref_code(unsigned ch) {
    const char *t = "=ACMGRSVTWYHKDBN";
    for (unsigned k = 0; k < 16; ++k)
        if ((unsigned)(uint8_t)t[k] == ch) return k;
    return 15;
}
PLO_HD bool pileup_pair_matches(unsigned c1, unsigned ch) {
    const unsigned c2 = pileup_ref_code(ch);
    return c1 == 0 || (c1 == c2 && c1 != 15);
}
// the channel of a mismatching read base
PLO_HD int pileup_channel(unsigned c1) { return c1 == 1 ? PILEUP_A : c1 == 2 ? PILEUP_C : c1 == 4 ? PILEUP_G : c1 == 8 ? PILEUP_T : PILEUP_N; }

// The slots: chromosome r holds the bases [slot_beg[r], slot_end[r]) from base slot_off[r] of the array on; slot_off[n_ref] = the bases of the
// array.  No regions: every chromosome whole.  With regions a chromosome without one holds nothing.  -> 0, or what is refused (`which` names
// the chromosome or the region): 1 a negative length, 2 a region's ref_id outside [0, n_ref), 3 beg < 0, beg > end or end > ref_len,
// 4 a second region on one chromosome
PLO_HD int pileup_layout(uint32_t n_ref, const int32_t *ref_len, uint32_t n_regions, const PileupRegion *regions, int32_t *slot_beg, int32_t *slot_end, uint64_t *slot_off,
                         uint32_t &which) {
    for (uint32_t r = 0; r < n_ref; ++r) {
        if (ref_len[r] < 0) {
            which = r;
            return 1;
        }
        slot_beg[r] = 0;
        slot_end[r] = n_regions ? -1 : ref_len[r];  // (-1: no region yet)
    }
    for (uint32_t k = 0; k < n_regions; ++k) {
        const PileupRegion &g = regions[k];
        which = k;
        if (g.ref_id < 0 || (uint32_t)g.ref_id >= n_ref) return 2;
        if (g.beg < 0 || g.beg > g.end || g.end > ref_len[g.ref_id]) return 3;
        if (slot_end[g.ref_id] >= 0) return 4;
        slot_beg[g.ref_id] = g.beg;
        slot_end[g.ref_id] = g.end;
    }
    unsigned long long at = 0;
    for (uint32_t r = 0; r < n_ref; ++r) {
        if (slot_end[r] < 0) slot_beg[r] = slot_end[r] = 0;
        slot_off[r] = at;
        at += (unsigned long long)(slot_end[r] - slot_beg[r]);
    }
    slot_off[n_ref] = at;
    return 0;
}

// One counted record by one thread: n_cig words at cig from pos on, its 4-bit bases at seq, chrom the chromosome's bytes; slot = the counters
// of base `beg`, events outside [beg, end) are dropped.  -> the adds inside.  The caller has checked the record (its ops stay inside the
// chromosome and its l_seq bases) and that the ops consume reference.
PLO_HD unsigned long long pileup_add_scalar(const uint8_t *cig, unsigned n_cig, const uint8_t *seq, long long pos, const uint8_t *chrom, long long beg, long long end, int32_t *slot) {
    unsigned long long n = 0;
    long long rf = pos, rd = 0;
    auto hit = [&](long long b, int ch) {
        if (b >= beg && b < end) {
            slot[(b - beg) * PILEUP_CHANNELS + ch] += 1;
            ++n;
        }
    };
    for (unsigned k = 0; k < n_cig; ++k) {
        const unsigned op = index_rd32(cig + 4ull * k), t = op & 15u;
        const long long len = (long long)(op >> 4);
        if (!len) continue;
        if (t == 0 || t == 7 || t == 8) {
            for (long long x = 0; x < len; ++x) {
                const unsigned byte = seq[(rd + x) >> 1], c1 = ((rd + x) & 1) ? (byte & 15u) : (byte >> 4);
                if (!pileup_pair_matches(c1, chrom[rf + x])) hit(rf + x, pileup_channel(c1));
            }
            rf += len;
            rd += len;
        } else if (t == 2) {
            hit(rf, PILEUP_DEL);
            rf += len;
        } else if (t == 3) {
            rf += len;
        } else if (t == 1 || t == 4) {
            hit(rf - 1 > pos ? rf - 1 : pos, t == 1 ? PILEUP_INS : PILEUP_CLIP);
            rd += len;
        }
    }
    return n;
}

// what plo_pileup_sites_dev refuses -> 0, or 1 min_count < 1, 2 frac_den == 0 while frac_num != 0, 3 the depth object is open, 4 it has
// another chromosome list
PLO_HD int pileup_sites_refused(int32_t min_count, uint32_t frac_num, uint32_t frac_den, bool has_depth, bool depth_finished, bool same_chroms) {
    if (min_count < 1) return 1;
    if (frac_num != 0 && frac_den == 0) return 2;
    if (has_depth && !depth_finished) return 3;
    if (has_depth && !same_chroms) return 4;
    return 0;
}

// the site rule: m = the maximum over the masked channels; depth < 0: no depth object
PLO_HD bool pileup_is_site(const int32_t *count, uint32_t channel_mask, int32_t min_count, long long depth, uint32_t frac_num, uint32_t frac_den) {
    int32_t m = 0;
    bool any = false;
    for (int ch = 0; ch < PILEUP_CHANNELS; ++ch)
        if ((channel_mask >> ch) & 1u) {
            if (!any || count[ch] > m) m = count[ch];
            any = true;
        }
    if (!any || m < min_count) return false;
    if (depth < 0 || frac_num == 0) return true;
    return (unsigned long long)(uint32_t)m * frac_den >= (unsigned long long)frac_num * (unsigned long long)depth;
}

}  // namespace plo

#ifdef PLO_WAVE
#include "depth_core.hpp"
#include "nm_core.hpp"

namespace plo {

struct DevPileup {
    DevSort s;                        // the input fields only (bytes, n_bytes, n, record_off, n_ref): what sort_check_record reads
    const int32_t *ref_len;           // [n_ref]
    const uint64_t *slot_off;         // [n_ref + 1] first base of every slot, [n_ref] = the bases of the array
    const int32_t *slot_beg, *slot_end;  // [n_ref] the region of every chromosome
    int32_t *arr;                     // [bases][PILEUP_CHANNELS]
    uint32_t exclude_flags;
    const uint8_t *const *chrom_seq;  // [n_ref] the calling context's index
    uint64_t *plan;                   // [n] offset of the real CIGAR from the block_size word << 32 | its ops (0: the record adds nothing)
    int *err;                         // [1] lowest offending record << 4 | what it broke (DEPTH_NO_RECORD: none)
    unsigned *n_counted;              // [1]
    unsigned long long *n_events;     // [1] adds issued inside the regions
};

// ---- check ---------------------------------------------------------------------------------------------------------------------------------
// Record i by one wave -> 1 when it is counted and accepted.  Nothing outside [bytes, bytes + n_bytes) is read (depth_check_rules; the real
// CIGAR's ops lie inside the record once the kinds 6 and 7 are passed).
PLO_DEV unsigned pileup_check_record(const DevPileup &d, uint32_t i) {
    const DepthRec r = depth_check_rules(d.s, d.ref_len, d.exclude_flags, i);
    int kind = r.kind;
    unsigned long long lseq = 0;
    if (!kind) {
        lseq = rec_rd32(r.p + 20);
        if ((unsigned long long)r.at + 4ull * r.nc + (lseq + 1) / 2 + lseq > r.len) kind = PILEUP_ERR_SEQ;
    }
    const uint32_t n_cig = kind ? 0u : r.n_cig;  // (wave-uniform; 0 unless the record is counted)
    unsigned long long part = 0;
#pragma unroll 4
    for (unsigned long long k = (unsigned long long)wv::lane(); k < n_cig; k += PLO_WAVE) {
        const unsigned op = rec_rd32(r.cig + 4ull * k);
        part += ((0x193u >> (op & 15u)) & 1u) ? (unsigned long long)(op >> 4) : 0ull;  // M I S = X
    }
    const unsigned long long rdlen = wv::shfl(wave_scan_incl_u64(part), 63);
    if (!kind && r.counted && rdlen != lseq) kind = PILEUP_ERR_LSEQ;
    if (wv::lane() == 0) {
        if (kind) wv::atomic_min(d.err, (int)((i << 4) | (unsigned)kind));
        else d.plan[i] = ((unsigned long long)(r.cig - r.p) << 32) | (r.rlen ? n_cig : 0u);
    }
    return !kind && r.counted ? 1u : 0u;
}

PLO_DEV void pileup_check_records(const DevPileup &d, uint32_t w, uint32_t nw) {
    unsigned counted = 0;
    for (uint32_t i = w; i < d.s.n; i += nw) counted += pileup_check_record(d, i);
    if (wv::lane() == 0 && counted) wv::atomic_add_global(d.n_counted, counted);
}

// ---- add -----------------------------------------------------------------------------------------------------------------------------------
struct PileupSlot {
    int32_t *base;       // the counters of base `beg`
    long long beg, end;
};
// one event: dropped outside the region, so nothing outside the slot is written whatever b is
PLO_DEV void pileup_hit(const PileupSlot &sl, long long b, int ch, unsigned &ev) {
    if (b >= sl.beg && b < sl.end) {
        wv::atomic_add(sl.base + ((unsigned long long)(b - sl.beg) * PILEUP_CHANNELS + (unsigned)ch), 1);
        ++ev;
    }
}

// Record i of an ACCEPTED call by one wave; ev (per lane) gathers the adds issued.  The check has seen that the ops stay inside the
// chromosome and consume exactly l_seq bases, and that the bases lie inside the record: every step is `ok`, and nothing outside
// [seq, seq + (l_seq + 1) / 2), the record or [chrom_seq[r], chrom_seq[r] + ref_len[r]) is read.
PLO_DEV void pileup_add_record(const DevPileup &d, uint32_t i, unsigned &ev) {
    const unsigned long long plan = d.plan[i];
    const uint32_t n_cig = (uint32_t)plan;
    if (!n_cig) return;  // (wave-uniform, as every branch around a wave primitive below)
    const int lane = wv::lane();
    const uint8_t *p = d.s.bytes + d.s.record_off[i];
    const uint32_t ref = rec_rd32(p + 4);
    const long long pos = (long long)rec_rd32(p + 8);
    const uint8_t *seq = p + 36u + p[12] + 4u * rec_rd16(p + 16);
    const AlnItem it = aln_open_record(seq, rec_rd32(p + 20), (uintptr_t)d.chrom_seq[ref] + (uintptr_t)pos, (unsigned long long)((long long)d.ref_len[ref] - pos), p + (plan >> 32), n_cig);
    PileupSlot sl;
    sl.base = d.arr + d.slot_off[ref] * PILEUP_CHANNELS;
    sl.beg = d.slot_beg[ref];
    sl.end = d.slot_end[ref];
    unsigned long long rd_done = 0, rf_done = 0;  // (uniform) consumed by the steps so far
    for (uint32_t k = 0; k < it.n; k += 64) {
        const AlnStep st = aln_step_bytes(it, k, rd_done, rf_done);
        if (!st.ok) return;
        if (st.has && st.len) {  // the lane that owns a D, I or S: its one add
            const long long rf = pos + (long long)(st.fa - it.ref0);
            if (st.t == 2) pileup_hit(sl, rf, PILEUP_DEL, ev);
            else if (st.t == 1 || st.t == 4) pileup_hit(sl, rf - 1 > pos ? rf - 1 : pos, st.t == 1 ? PILEUP_INS : PILEUP_CLIP, ev);
        }
        const uint32_t np = st.is_cmp && st.len ? aln_lines(st.fa, st.len) : 0u;
        const uint32_t p_inc = (uint32_t)wv::scan_add((int)np);
        const uint32_t n_pieces = (uint32_t)wv::bcast_last((int)p_inc);
        for (uint32_t p0 = 0; p0 < n_pieces; p0 += 64) {
            const uint32_t pc = p0 + (uint32_t)lane;
            const AlnOp o = aln_find_op(st, np, p_inc, pc);
            if (pc < n_pieces) {
                const uint32_t j = pc - o.first;
                uint32_t mask = nm_piece_t<true>(it.seq, it.seq_lo, it.seq_hi, o.fa, o.len, o.rd, j);
                if (mask) {
                    const AlnSpan sp = aln_span(o.fa, o.len, j);
                    const long long b0 = pos + (long long)(sp.s - it.ref0);
                    const unsigned long long r0 = o.rd + (unsigned long long)(sp.s - o.fa);
                    while (mask) {
                        const unsigned x = (unsigned)wv::ctz32(mask);
                        mask &= mask - 1;
                        const unsigned long long rp = r0 + x;
                        const unsigned byte = it.seq[rp >> 1];
                        pileup_hit(sl, b0 + x, pileup_channel((rp & 1u) ? (byte & 15u) : (byte >> 4)), ev);
                    }
                }
            }
        }
        rd_done = st.rd_end;
        rf_done = st.rf_end;
    }
}

PLO_DEV void pileup_add_records(const DevPileup &d, uint32_t w, uint32_t nw) {
    if (*d.err != DEPTH_NO_RECORD) return;  // a refused call: nothing is added
    unsigned long long events = 0;
    for (uint32_t i = w; i < d.s.n; i += nw) {
        unsigned ev = 0;
        pileup_add_record(d, i, ev);
        events += ev;
    }
    events = wv::shfl(wave_scan_incl_u64(events), 63);
    if (wv::lane() == 0 && events) wv::atomic_add_global(d.n_events, events);
}

// ---- sites ---------------------------------------------------------------------------------------------------------------------------------
struct alignas(16) PileupVec4 {  // four counters, moved as one 16-byte access
    int32_t x, y, z, w;
};
struct DevPileupSites {
    const int32_t *arr;
    const uint64_t *slot_off;         // [n_ref + 1]
    const int32_t *slot_beg;          // [n_ref]
    uint32_t n_ref;
    unsigned long long n_bases;
    const int32_t *depth;             // a finished depth object's array, or NULL
    const uint64_t *depth_slot_off;   // its slots
    const uint8_t *const *chrom_seq;
    uint32_t channel_mask;
    int32_t min_count;
    uint32_t frac_num, frac_den;
    unsigned long long *cnt;          // [n_tiles] sites of every tile
    const unsigned long long *start;  // [n_tiles + 1] their exclusive scan
    PileupSite *site;
};
// Tile `tile` of the array's bases by one wave, 64 bases a trip, a lane each.  EMIT false: the tile's sites are counted.  EMIT true: site
// number k (the tile's first + the sites in front of it inside the tile) is written whole by the lane of its base: every field has one writer.
template <bool EMIT>
PLO_DEV void pileup_sites_tile(const DevPileupSites &d, unsigned long long tile) {
    const unsigned long long lo = tile * PILEUP_TILE;
    unsigned long long hi = lo + PILEUP_TILE;
    if (hi > d.n_bases) hi = d.n_bases;
    const unsigned long long below_mask = (1ull << wv::lane()) - 1ull;
    uint32_t r = 0, b = d.n_ref;  // the last slot that begins at or before lo (n_ref >= 1: the array has bases)
    while (b - r > 1) {
        const uint32_t m = r + ((b - r) >> 1);
        if (d.slot_off[m] <= lo) r = m;
        else b = m;
    }
    unsigned long long k = EMIT ? d.start[tile] : 0ull;
    for (unsigned long long e0 = lo; e0 < hi; e0 += PLO_WAVE) {  // (the same trips for every lane)
        const unsigned long long e = e0 + (unsigned)wv::lane();
        bool is_site = false;
        int32_t c[PILEUP_CHANNELS] = {0, 0, 0, 0, 0, 0, 0, 0};
        long long dep = -1;
        unsigned long long pos = 0;
        if (e < hi) {
            while (r + 1 < d.n_ref && d.slot_off[r + 1] <= e) ++r;  // (slots without bases are stepped over)
            pos = (unsigned long long)d.slot_beg[r] + (e - d.slot_off[r]);
            const PileupVec4 *q = (const PileupVec4 *)(d.arr + e * PILEUP_CHANNELS);  // (32-byte aligned: the array is, a base holds 32 bytes)
            const PileupVec4 v0 = q[0], v1 = q[1];
            c[0] = v0.x, c[1] = v0.y, c[2] = v0.z, c[3] = v0.w;
            c[4] = v1.x, c[5] = v1.y, c[6] = v1.z, c[7] = v1.w;
            if (d.depth) dep = (long long)(uint32_t)d.depth[d.depth_slot_off[r] + pos];
            is_site = pileup_is_site(c, d.channel_mask, d.min_count, dep, d.frac_num, d.frac_den);
        }
        const unsigned long long ms = wv::ballot(is_site);
        if (EMIT && is_site) {
            PileupSite s;
            s.ref_id = (int32_t)r;
            s.pos = (int32_t)pos;
            s.depth = (int32_t)dep;
            s.ref_base = d.chrom_seq[r][pos];
            s.pad[0] = s.pad[1] = s.pad[2] = 0;
            for (int ch = 0; ch < PILEUP_CHANNELS; ++ch) s.count[ch] = c[ch];
            d.site[k + (unsigned long long)__builtin_popcountll(ms & below_mask)] = s;
        }
        k += (unsigned long long)__builtin_popcountll(ms);
    }
    if (!EMIT && wv::lane() == 0) d.cnt[tile] = k;
}

}  // namespace plo
#endif
