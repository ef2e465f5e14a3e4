// depth_core.hpp -- the depth of the output records on the device (plo_depth_*): how many counted records cover every reference base.
// The rule is stated in include/portello_liftover.h ("Depth of the records").  In short: a depth object holds one int32 array, chromosome r
// owns ref_len[r] + 1 entries that start at a multiple of DEPTH_SLOT_ALIGN; a counted record (refID >= 0, pos >= 0, FLAG & exclude == 0)
// adds +1 where a covered stretch of its real CIGAR begins and -1 behind it (M, =, X cover; D covers with count_deletions; N consumes
// reference and covers nothing; ops of length 0 are ignored); an inclusive scan over the whole array turns the differences into depths.
// Every slot's differences sum to zero, so ONE scan over the allocation equals a scan per chromosome.
//   check   (a wave per record): what plo_records_sort_dev and the index call check, the aux walk to the first CG of a record in placeholder
//           form (real_cigar of batch_core.hpp), the reference length of a counted record's ops -> the lowest offender << 4 | kind, and a
//           plan word per record (where its real CIGAR stands, how many ops; 0 ops: nothing to add)
//   add     (a wave per record): reads the check's word first -- a refused call adds nothing --, then the ops a lane each, 64 a trip; a wave
//           prefix sum of the reference lengths gives every op its start, two ballots say which ops consume reference and which cover, and a
//           lane emits +1 at its op's start iff the op covers and the nearest reference-consuming op in front of it does not (or there is
//           none), -1 at its op's start iff the op consumes reference without covering and the nearest reference-consuming op in front
//           covers.  That -1 stands exactly behind the last covering op of the stretch (ops that consume nothing do not move the position),
//           so it is the -1 "behind the op whose follower does not cover", decided from the follower's side: only a carry from the front is
//           needed (position, and whether the last reference-consuming op covered), and it crosses the 64-op seam.  A stretch still open at
//           the record's end is closed by lane 0.  One atomic per end of a maximal covered stretch: two a record for an = / X CIGAR.
//   finish  tile sums -> sums of the sums -> one wave scans those -> the tiles of the sums -> the tiles of the array: five launches, none of
//           which waits on another workgroup.  Tiles are PLO_DEPTH_TILE entries, a wave each; all sums are 32-bit and exact modulo 2^32 (a
//           prefix of the differences is a depth, and a depth fits int32 as long as fewer than 2^31 counted records cover one base)
//   windows (a wave per window of w >= 64 bases, a lane per window below that): the uint64 sum of the depths of every window
//   runs    maximal stretches of equal depth inside a chromosome: run starts counted per tile, the 64-bit scan of records_core.hpp, emit
// The file has two parts, like index_core.hpp: plain C++ for the rule of one record by one thread (depth_add_scalar), and the wave part.
// The same functions run under the CPU emulator (tests/emu/emu_depth.cpp), there with a small PLO_DEPTH_TILE.
#pragma once
#include <stdint.h>

#include "index_core.hpp"

#ifndef PLO_DEPTH_TILE
#define PLO_DEPTH_TILE 1024
#endif

namespace plo {

constexpr int DEPTH_NO_RECORD = 0x7fffffff;
constexpr uint32_t DEPTH_MAX_RECORDS = INDEX_MAX_RECORDS;  // record << 4 | kind in one word
constexpr unsigned long long DEPTH_SLOT_ALIGN = 64, DEPTH_TILE = PLO_DEPTH_TILE;
static_assert(PLO_DEPTH_TILE >= 4 && PLO_DEPTH_TILE % 4 == 0, "a lane takes four entries at a time");
// what the lowest offending record broke, behind SORT_ERR_* (1 .. 5)
enum { DEPTH_ERR_CIGAR = 6,  // the in-record CIGAR leaves the record (INDEX_ERR_CIGAR)
       DEPTH_ERR_AUX = 7,    // placeholder form: the aux fields begin behind the record's end, a malformed field stands in front of the first CG, or that CG's array leaves the record
       DEPTH_ERR_END = 8 };  // a counted record ends behind ref_len[refID]

struct alignas(16) DepthVec4 {  // four entries, moved as one 16-byte access
    int32_t x, y, z, w;
};
struct DepthRun {  // plo_depth_run (portello_liftover.h)
    int32_t ref_id, beg, end, depth;
};
static_assert(sizeof(DepthRun) == 16, "plo_depth_run is 16 bytes");

// does a CIGAR word cover its reference bases?  M, =, X (codes 0, 7, 8), D (2) with count_deletions; a length of 0 covers nothing
PLO_HD bool depth_op_covers(unsigned op, bool count_del) {
    const unsigned c = op & 15u;
    return (op >> 4) != 0 && (c == 0 || c == 7 || c == 8 || (c == 2 && count_del));
}
// the entries of chromosome r's slot, and where the next slot may begin
PLO_HD unsigned long long depth_slot_entries(unsigned long long ref_len) { return (ref_len + 1 + DEPTH_SLOT_ALIGN - 1) / DEPTH_SLOT_ALIGN * DEPTH_SLOT_ALIGN; }

// One counted record by one thread, an add per covering op (the array is the same as with an add per stretch): n_cig words at cig, from pos.
// slot has room for the record's end (the caller has checked it against ref_len).
PLO_HD void depth_add_scalar(const uint8_t *cig, unsigned n_cig, long long pos, bool count_del, int32_t *slot) {
    for (unsigned k = 0; k < n_cig; ++k) {
        const unsigned op = index_rd32(cig + 4ull * k);
        const long long len = (long long)index_op_reflen(op);
        if (depth_op_covers(op, count_del)) {
            slot[pos] += 1;
            slot[pos + len] -= 1;
        }
        pos += len;
    }
}

// where the slots begin: slot_off[n_ref + 1], -> the entries of the array
PLO_HD unsigned long long depth_layout(uint32_t n_ref, const int32_t *ref_len, uint64_t *slot_off) {
    unsigned long long at = 0;
    for (uint32_t r = 0; r < n_ref; ++r) {
        slot_off[r] = at;
        at += depth_slot_entries((unsigned long long)(uint32_t)ref_len[r]);
    }
    slot_off[n_ref] = at;
    return at;
}
// the first window of every chromosome for windows of w >= 1 bases: win_first[n_ref + 1], -> the windows in all
PLO_HD unsigned long long depth_win_layout(uint32_t n_ref, const int32_t *ref_len, uint32_t w, uint64_t *win_first) {
    unsigned long long at = 0;
    for (uint32_t r = 0; r < n_ref; ++r) {
        win_first[r] = at;
        at += ((unsigned long long)(uint32_t)ref_len[r] + w - 1) / w;
    }
    win_first[n_ref] = at;
    return at;
}
// the object's two states and what each admits: adds and the finish while it is open, windows and runs once it is finished, reset always
enum { DEPTH_CALL_ADD = 0, DEPTH_CALL_FINISH = 1, DEPTH_CALL_WINDOWS = 2, DEPTH_CALL_RUNS = 3, DEPTH_CALL_RESET = 4 };
PLO_HD bool depth_call_allowed(bool finished, int call) {
    return call == DEPTH_CALL_RESET || (call == DEPTH_CALL_ADD || call == DEPTH_CALL_FINISH ? !finished : finished);
}

}  // namespace plo

#ifdef PLO_WAVE
#include "batch_core.hpp"
#include "sort_core.hpp"

namespace plo {

struct DevDepth {
    DevSort s;                    // the input fields only (bytes, n_bytes, n, record_off, n_ref): what sort_check_record reads
    const int32_t *ref_len;       // [n_ref]
    const uint64_t *slot_off;     // [n_ref + 1] first entry of every slot, [n_ref] = the entries of the array
    int32_t *arr;
    uint32_t exclude_flags;
    int count_del;
    uint64_t *plan;               // [n] offset of the real CIGAR from the block_size word << 32 | its ops (0: the record adds nothing)
    int *err;                     // [1] lowest offending record << 4 | what it broke (DEPTH_NO_RECORD: none)
    unsigned *n_counted;          // [1]
};

// ---- check ---------------------------------------------------------------------------------------------------------------------------------
// what the check learns of record i (all of it wave-uniform); pileup_core.hpp goes on from here
struct DepthRec {
    int kind;                 // 0, or the first of the kinds 1 .. 8 the record breaks
    const uint8_t *p;         // the record (its block_size word)
    unsigned long long len;   // its bytes
    unsigned at, nc;          // the in-record CIGAR: its offset and its ops
    const uint8_t *cig;       // the real CIGAR, n_cig ops (0 unless the record is counted)
    uint32_t n_cig;
    int ref, pos;
    bool counted;
    unsigned long long rlen;  // the reference length of the n_cig ops
};
// Record i by one wave (i wave-uniform).  Nothing outside [bytes, bytes + n_bytes) is read: the fixed fields only behind sort_check_record,
// the in-record ops only behind index_cigar_fits, an aux byte only inside the record (aux_field_len_wave), the ops of CG only behind that
// field's own length check.
PLO_DEV DepthRec depth_check_rules(const DevSort &s, const int32_t *ref_len, uint32_t exclude_flags, uint32_t i) {
    DepthRec r;
    unsigned long long key, len;
    int kind = sort_check_record(s, i, key, len);
    const uint8_t *p = s.bytes + (kind == SORT_ERR_OFFSET ? 0ull : s.record_off[i]);
    unsigned at = 0, nc = 0;
    if (!kind && !index_cigar_fits(p, len, at, nc)) kind = DEPTH_ERR_CIGAR;
    const uint8_t *cig = p + at;
    uint32_t n_cig = nc;
    if (!kind) {
        const uint32_t lseq = rec_rd32(p + 20);
        if (bb_cigar_is_placeholder(cig, n_cig, lseq)) {  // (wave-uniform) aux_find for CG, as batch_plan_read walks
            const unsigned long long aux_off = (unsigned long long)at + 8ull + ((unsigned long long)lseq + 1) / 2 + lseq;
            const uint8_t *e = p + len, *cg = nullptr;
            if (aux_off > len) kind = DEPTH_ERR_AUX;
            const uint8_t *a = kind ? e : p + aux_off;
            while (a < e) {
                const unsigned long long n = aux_field_len_wave(a, e);
                if (!n) {
                    kind = DEPTH_ERR_AUX;
                    break;
                }
                if (a[0] == 'C' && a[1] == 'G') {
                    cg = a;
                    break;
                }
                a += n;
            }
            if (!kind) bb_real_cigar(cg, lseq, cig, n_cig);
        }
    }
    int ref = -1, pos = -1;
    bool counted = false;
    if (!kind) {
        ref = (int)rec_rd32(p + 4);
        pos = (int)rec_rd32(p + 8);
        counted = ref >= 0 && pos >= 0 && (rec_rd16(p + 18) & exclude_flags) == 0;
    }
    if (!counted) n_cig = 0;  // (wave-uniform: the reductions below are reached by every lane either way)
    unsigned long long part = 0;
#pragma unroll 4
    for (unsigned long long k = (unsigned long long)wv::lane(); k < n_cig; k += PLO_WAVE) part += index_op_reflen(rec_rd32(cig + 4ull * k));
    // (below 2^58: fewer than 2^30 ops, the array of CG lies inside a record of less than 2^32 bytes, of less than 2^28 bases each)
    const unsigned long long rlen = wv::shfl(wave_scan_incl_u64(part), 63);
    if (counted && (unsigned long long)pos + rlen > (unsigned long long)(uint32_t)ref_len[ref]) kind = DEPTH_ERR_END;
    r.kind = kind;
    r.p = p;
    r.len = len;
    r.at = at;
    r.nc = nc;
    r.cig = cig;
    r.n_cig = n_cig;
    r.ref = ref;
    r.pos = pos;
    r.counted = counted;
    r.rlen = rlen;
    return r;
}
// -> 1 when record i is counted and accepted; the lowest offender, or the record's plan word
PLO_DEV unsigned depth_check_record(const DevDepth &d, uint32_t i) {
    const DepthRec r = depth_check_rules(d.s, d.ref_len, d.exclude_flags, i);
    if (wv::lane() == 0) {
        if (r.kind) wv::atomic_min(d.err, (int)((i << 4) | (unsigned)r.kind));
        else d.plan[i] = ((unsigned long long)(r.cig - r.p) << 32) | r.n_cig;
    }
    return !r.kind && r.counted ? 1u : 0u;
}

// the records w, w + nw, ... by wave w of nw
PLO_DEV void depth_check_records(const DevDepth &d, uint32_t w, uint32_t nw) {
    unsigned counted = 0;
    for (uint32_t i = w; i < d.s.n; i += nw) counted += depth_check_record(d, i);
    if (wv::lane() == 0 && counted) wv::atomic_add_global(d.n_counted, counted);
}

// ---- add -----------------------------------------------------------------------------------------------------------------------------------
// Record i of an ACCEPTED call by one wave.  Every position written lies in [pos, pos + rlen] <= ref_len[ref]: inside the slot.
PLO_DEV void depth_add_record(const DevDepth &d, uint32_t i) {
    const unsigned long long plan = d.plan[i];
    const uint32_t n_cig = (uint32_t)plan;
    if (!n_cig) return;  // (wave-uniform)
    const uint8_t *p = d.s.bytes + d.s.record_off[i];
    const uint8_t *cig = p + (plan >> 32);
    int32_t *slot = d.arr + d.slot_off[rec_rd32(p + 4)];
    const bool del = d.count_del != 0;
    const int lane = wv::lane();
    const unsigned long long below_mask = (1ull << lane) - 1ull;
    unsigned at = rec_rd32(p + 8);  // the reference position in front of this trip's ops (the check: at + every sum <= ref_len < 2^31)
    bool open = false;              // the nearest reference-consuming op in front of this trip covers
    for (uint32_t k0 = 0; k0 < n_cig; k0 += PLO_WAVE) {
        const uint32_t k = k0 + (uint32_t)lane;
        const unsigned op = k < n_cig ? rec_rd32(cig + 4ull * k) : 0u;
        const unsigned rl = (unsigned)index_op_reflen(op);
        const bool consumes = rl != 0, covers = depth_op_covers(op, del);
        const unsigned incl = (unsigned)wv::scan_add((int)rl);
        const unsigned long long mc = wv::ballot(consumes), mv = wv::ballot(covers);
        const unsigned long long front = mc & below_mask;
        const bool front_covers = front ? ((mv >> (63 - __builtin_clzll(front))) & 1ull) != 0 : open;
        const unsigned start = at + incl - rl;
        if (covers && !front_covers) wv::atomic_add(slot + start, 1);
        if (consumes && !covers && front_covers) wv::atomic_add(slot + start, -1);
        at += (unsigned)wv::bcast_last((int)incl);
        if (mc) open = ((mv >> (63 - __builtin_clzll(mc))) & 1ull) != 0;
    }
    if (open && lane == 0) wv::atomic_add(slot + at, -1);
}

PLO_DEV void depth_add_records(const DevDepth &d, uint32_t w, uint32_t nw) {
    if (*d.err != DEPTH_NO_RECORD) return;  // a refused call: nothing is added
    for (uint32_t i = w; i < d.s.n; i += nw) depth_add_record(d, i);
}

// ---- finish: the inclusive 32-bit scan in three phases ------------------------------------------------------------------------------------------
// four entries of a from e on, zero behind n
PLO_DEV void depth_load4(const int32_t *a, unsigned long long n, unsigned long long e, int32_t v[4]) {
    if (e + 4 <= n) {
        const DepthVec4 *q = (const DepthVec4 *)(a + e);  // (16-byte aligned: the array, the tiles and e are multiples of 4 entries)
        const DepthVec4 t = *q;
        v[0] = t.x;
        v[1] = t.y;
        v[2] = t.z;
        v[3] = t.w;
    } else {
        for (int j = 0; j < 4; ++j) v[j] = e + j < n ? a[e + j] : 0;
    }
}
// sums[tile] = the sum of tile `tile` of a[0, n), by one wave
PLO_DEV void depth_tile_sum(const int32_t *a, unsigned long long n, unsigned long long tile, int32_t *sums) {
    const unsigned long long lo = tile * DEPTH_TILE;
    unsigned long long hi = lo + DEPTH_TILE;
    if (hi > n) hi = n;
    unsigned s = 0;
    for (unsigned long long e = lo + 4ull * (unsigned)wv::lane(); e < hi; e += 4ull * PLO_WAVE) {
        int32_t v[4];
        depth_load4(a, hi, e, v);
        s += (unsigned)v[0] + (unsigned)v[1] + (unsigned)v[2] + (unsigned)v[3];
    }
    const int t = wv::reduce_add((int)s);
    if (wv::lane() == 0) sums[tile] = t;
}
// tile `tile` of a[0, n) becomes its inclusive scan, in place, by one wave; incl (NULL: none) holds the inclusive scan of the tiles' sums
PLO_DEV void depth_tile_scan(int32_t *a, unsigned long long n, unsigned long long tile, const int32_t *incl) {
    const unsigned long long lo = tile * DEPTH_TILE;
    unsigned long long hi = lo + DEPTH_TILE;
    if (hi > n) hi = n;
    unsigned carry = incl && tile ? (unsigned)incl[tile - 1] : 0u;
    for (unsigned long long e0 = lo; e0 < hi; e0 += 4ull * PLO_WAVE) {  // (the same trips for every lane)
        const unsigned long long e = e0 + 4ull * (unsigned)wv::lane();
        int32_t v[4];
        depth_load4(a, hi, e < hi ? e : hi, v);
        const unsigned s = (unsigned)v[0] + (unsigned)v[1] + (unsigned)v[2] + (unsigned)v[3];
        const unsigned inc = (unsigned)wv::scan_add((int)s);
        unsigned run = carry + inc - s;
        if (e + 4 <= hi) {
            DepthVec4 t;
            t.x = (int)(run += (unsigned)v[0]);
            t.y = (int)(run += (unsigned)v[1]);
            t.z = (int)(run += (unsigned)v[2]);
            t.w = (int)(run += (unsigned)v[3]);
            *(DepthVec4 *)(a + e) = t;
        } else {
            for (int j = 0; j < 4; ++j)
                if (e + j < hi) a[e + j] = (int32_t)(run += (unsigned)v[j]);
        }
        carry += (unsigned)wv::bcast_last((int)inc);
    }
}
// a[0, n) becomes its inclusive scan by ONE wave: the top of the pyramid, n / PLO_DEPTH_TILE^2 values
PLO_DEV void depth_top_scan(int32_t *a, unsigned long long n) {
    unsigned carry = 0;
    for (unsigned long long e0 = 0; e0 < n; e0 += PLO_WAVE) {
        const unsigned long long e = e0 + (unsigned)wv::lane();
        const unsigned v = e < n ? (unsigned)a[e] : 0u;
        const unsigned inc = (unsigned)wv::scan_add((int)v);
        if (e < n) a[e] = (int32_t)(carry + inc);
        carry += (unsigned)wv::bcast_last((int)inc);
    }
}

// ---- windows ---------------------------------------------------------------------------------------------------------------------------------
struct DevDepthWin {
    const int32_t *arr;
    const int32_t *ref_len;
    const uint64_t *slot_off;
    const uint64_t *win_first;  // [n_ref + 1]
    uint32_t n_ref;
    uint32_t w;
    unsigned long long n_win;
    uint64_t *sum;              // [n_win]
};
// the chromosome of window g: the last r with win_first[r] <= g (chromosomes without windows are stepped over)
PLO_DEV uint32_t depth_upper(const uint64_t *first, uint32_t n_ref, unsigned long long g) {
    uint32_t a = 0, b = n_ref;
    while (b - a > 1) {
        const uint32_t m = a + ((b - a) >> 1);
        if (first[m] <= g) a = m;
        else b = m;
    }
    return a;
}
PLO_DEV void depth_window_span(const DevDepthWin &d, unsigned long long g, const int32_t *&a, unsigned long long &n) {
    const uint32_t r = depth_upper(d.win_first, d.n_ref, g);
    const unsigned long long lo = (g - d.win_first[r]) * d.w, len = (unsigned long long)(uint32_t)d.ref_len[r];
    a = d.arr + d.slot_off[r] + lo;
    n = len - lo < d.w ? len - lo : d.w;
}
// wave w of nw: a window a trip when the windows hold 64 bases or more, 64 windows a trip (a lane each) below that
PLO_DEV void depth_windows(const DevDepthWin &d, unsigned long long w, unsigned long long nw) {
    if (d.w >= PLO_WAVE) {
        for (unsigned long long g = w; g < d.n_win; g += nw) {
            const int32_t *a;
            unsigned long long n;
            depth_window_span(d, g, a, n);
            unsigned long long s = 0;
            for (unsigned long long k = (unsigned)wv::lane(); k < n; k += PLO_WAVE) s += (unsigned long long)(uint32_t)a[k];
            s = wave_scan_incl_u64(s);
            if (wv::lane() == 63) d.sum[g] = s;
        }
    } else {
        for (unsigned long long g = w * PLO_WAVE + (unsigned)wv::lane(); g < d.n_win; g += nw * PLO_WAVE) {
            const int32_t *a;
            unsigned long long n;
            depth_window_span(d, g, a, n);
            unsigned long long s = 0;
            for (unsigned long long k = 0; k < n; ++k) s += (unsigned long long)(uint32_t)a[k];
            d.sum[g] = s;
        }
    }
}

// ---- runs ------------------------------------------------------------------------------------------------------------------------------------
struct DevDepthRuns {
    const int32_t *arr;
    const int32_t *ref_len;
    const uint64_t *slot_off;
    uint32_t n_ref;
    unsigned long long n_entries;
    unsigned long long *cnt;          // [n_tiles] run starts of every tile
    const unsigned long long *start;  // [n_tiles + 1] their exclusive scan
    DepthRun *run;
};
// Tile `tile` of the array by one wave, 64 entries a trip.  Entry e of chromosome r at base b = e - slot_off[r] begins a run iff b < ref_len[r]
// and (b == 0 or its depth differs from the entry's in front).  EMIT false: the tile's starts are counted.  EMIT true: the start with number k
// (the tile's first + the starts in front of it inside the tile) writes ref_id, beg and depth of run k and, unless b == 0, the end of run
// k - 1; the entry b == ref_len[r] > 0 -- the slot's extra one -- writes the end of the chromosome's last run.  Every field has one writer.
template <bool EMIT>
PLO_DEV void depth_runs_tile(const DevDepthRuns &d, unsigned long long tile) {
    const unsigned long long lo = tile * DEPTH_TILE;
    unsigned long long hi = lo + DEPTH_TILE;
    if (hi > d.n_entries) hi = d.n_entries;
    const unsigned long long below_mask = (1ull << wv::lane()) - 1ull;
    uint32_t r = 0, b = d.n_ref;  // the last slot that begins at or before lo (n_ref >= 1: the array has entries)
    while (b - r > 1) {
        const uint32_t m = r + ((b - r) >> 1);
        if (d.slot_off[m] <= lo) r = m;
        else b = m;
    }
    unsigned long long k = EMIT ? d.start[tile] : 0ull;
    for (unsigned long long e0 = lo; e0 < hi; e0 += PLO_WAVE) {  // (the same trips for every lane)
        const unsigned long long e = e0 + (unsigned)wv::lane();
        bool is_start = false, is_end = false;
        unsigned long long base = 0;
        int32_t v = 0;
        if (e < hi) {
            while (r + 1 < d.n_ref && d.slot_off[r + 1] <= e) ++r;  // (a slot holds 64 entries at the least: a step or two)
            base = e - d.slot_off[r];
            const unsigned long long len = (unsigned long long)(uint32_t)d.ref_len[r];
            v = d.arr[e];
            is_start = base < len && (base == 0 || v != d.arr[e - 1]);
            is_end = base == len && len > 0;
        }
        const unsigned long long ms = wv::ballot(is_start);
        if (EMIT) {
            const unsigned long long me = k + (unsigned long long)__builtin_popcountll(ms & below_mask);
            if (is_start) {
                d.run[me].ref_id = (int32_t)r;
                d.run[me].beg = (int32_t)base;
                d.run[me].depth = v;
                if (base) d.run[me - 1].end = (int32_t)base;
            }
            if (is_end) d.run[me - 1].end = (int32_t)base;
        }
        k += (unsigned long long)__builtin_popcountll(ms);
    }
    if (!EMIT && wv::lane() == 0) d.cnt[tile] = k;
}

}  // namespace plo
#endif
