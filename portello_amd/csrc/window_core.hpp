// window_core.hpp -- the record walk and the window cut of plo_bam_read_window (bam_host.cpp:231-319) over a stretch of the inflated BAM
// stream in device memory.  The walk is a chain (next = at + 4 + block_size(at)); it is cut into segments of seg_bytes whose walks run side
// by side from GUESSED starts, and a serial pass over the segments (not over the records) keeps the walks whose guess was the true entry
// and repeats the others:
//   guess   (a wave per segment):  the lowest offset in the segment from which eight plausible records follow each other (or records up to
//                                  the end of the bytes): plausible_record's chain rule (bam_host.cpp:113-130, :183-200) without the
//                                  reference count.  A hint only: a wrong or missing guess costs time, never a result
//   walk    (a lane per segment):  from the guess until the position leaves the segment -> where it landed, primary / unmapped records and
//                                  unmapped bytes met
//   resolve (one wave):            segment by segment, the true entry of a segment is the landing of the last live segment in front of it;
//                                  a segment whose guess differs is walked again from the true entry.  Segments a record jumps over and
//                                  segments behind the end of the chain are dead: their counts are zeroed
//   scan    (waves):               the 64-bit exclusive scans of records_core.hpp over the three counts of every segment
//   find    (a lane per segment):  the host loop's stop tests in its order in front of every record, then its refusals; the lowest offset
//                                  at which one of them fires is where the window ends
//                                  (a part of a file: the host's range test stands among them, a record at or behind own_bytes ends the
//                                  window with PLO_CUT_PART_END; the walks may run past own_bytes, their counts there are never used)
//   emit    (a lane per segment):  read_rec_off and the unmapped records' places, then their bytes with copy_span (a workgroup per record)
// The chain ends in exactly one TERMINAL position: the end of the bytes, a record the bytes cut short, or a record the host refuses.
// Position stream_bytes itself belongs to the last segment (n / seg_bytes + 1 segments), so the end of the bytes is classified like a record.
// Every block_size is checked against stream_bytes before a byte behind it is read; nothing outside [stream, stream + stream_bytes) is read.
// A lane works on one segment (walk / find / emit) or the wave on one (guess / resolve); values every lane holds alike are called uniform.
// The same functions run under the CPU emulator (tests/emu/emu_cut.cpp).
#pragma once
#include <plo_wave.hpp>
#include <stdint.h>

#include "records_core.hpp"

namespace plo {

constexpr unsigned long long CUT_NONE = ~0ull;  // no guess / a dead segment (guess), the walk met the terminal position (land), nothing fired (fire)

// what stands at a position of the chain
enum { CUT_PRIMARY = 0, CUT_UNMAPPED = 1, CUT_SUPPLEMENTARY = 2,
       CUT_T_END = 3,      // at == stream_bytes
       CUT_T_TRUNC = 4,    // fewer than 4 bytes, or fewer than 4 + block_size
       CUT_T_SHORT = 5,    // block_size < 32
       CUT_T_LAYOUT = 6,   // Rec::layout_ok
       CUT_T_UNM_TID = 7   // flag 0x4 with tid >= 0
};
// why the find pass stopped (the low values are the ABI's PLO_CUT_*)
enum { CUT_WHY_ERR_TRUNC = 16, CUT_WHY_ERR_SHORT = 17, CUT_WHY_ERR_LAYOUT = 18, CUT_WHY_ERR_UNM_TID = 19 };
// result block (dwords pairs): what the host reads back in its one wait for the counts
enum { CR_AT = 0, CR_WHY = 1, CR_READS = 2, CR_UNMAPPED = 3, CR_UNM_BYTES = 4, CR_REWALKS = 5, CR_WORDS = 8 };

struct DevCut {
    const uint8_t *stream;
    unsigned long long n;          // stream_bytes
    unsigned long long seg_bytes;  // at least 64
    uint32_t n_seg;                // n / seg_bytes + 1
    unsigned long long max_records, max_unmapped, max_bytes;
    int final;
    int ranged;                    // a part of a file (plo_window_cut_part_dev): records at or behind own_bytes are the next part's
    unsigned long long own_bytes;  // offset of the first block that starts in the next part's stretch (BgzfIn::range_end as an inflated offset)
    // per segment
    unsigned long long *guess;        // entry: the guess, from resolve on the true entry of a live segment, CUT_NONE of a dead one
    unsigned long long *land;         // where the walk from `guess` left the segment, CUT_NONE: it met the terminal position
    unsigned long long *cnt;          // [3][n_seg]: primary records, unmapped records, bytes of the unmapped records
    const unsigned long long *start;  // [3][n_seg + 1]: their exclusive scans
    unsigned long long *fire;         // [5][n_seg]: offset, why, reads, unmapped, unmapped bytes at the first test that fired (offset CUT_NONE: none)
    unsigned long long *res;          // [CR_WORDS]; res[CR_AT] is the running minimum of the find pass
    // emit
    unsigned long long cut_at;
    uint64_t *read_rec_off, *unm_off, *unm_src;
    uint8_t *unmapped;
    unsigned long long n_unmapped, unmapped_bytes;
};

PLO_DEV unsigned long long cut_seg_end(const DevCut &d, uint32_t s) {  // (the last segment holds position n)
    const unsigned long long e = ((unsigned long long)s + 1) * d.seg_bytes;
    return e < d.n + 1 ? e : d.n + 1;
}

// what stands at `at` (<= n); bs = its block_size where it is a record
PLO_DEV int cut_classify(const DevCut &d, unsigned long long at, uint32_t &bs) {
    bs = 0;
    if (at == d.n) return CUT_T_END;
    if (d.n - at < 4) return CUT_T_TRUNC;
    const uint8_t *p = d.stream + at;
    bs = rec_rd32(p);
    if (bs < 32) return CUT_T_SHORT;
    if (bs > d.n - at - 4) return CUT_T_TRUNC;
    p += 4;
    const uint32_t lq = p[8], ncg = rec_rd16(p + 12), flag = rec_rd16(p + 14), lseq = rec_rd32(p + 16);
    // Rec::layout_ok (bam_internal.hpp:838): (l_seq + 1) / 2 in 32 bits as there
    if (32ull + lq + 4ull * ncg + (uint32_t)(lseq + 1u) / 2u + lseq > bs) return CUT_T_LAYOUT;
    if (flag & 0x4u) return (int)rec_rd32(p) >= 0 ? CUT_T_UNM_TID : CUT_UNMAPPED;
    return (flag & 0x800u) ? CUT_SUPPLEMENTARY : CUT_PRIMARY;
}

// ---- guess ------------------------------------------------------------------------------------------------------------------------------
// plausible_record (bam_host.cpp:113-130) without the reference count: 0 = no record here, 1 = a record (len), 2 = the bytes end inside it
PLO_DEV int cut_plausible(const DevCut &d, unsigned long long q, unsigned long long &len) {
    if (d.n - q < 36) return 2;
    const uint8_t *p = d.stream + q;
    const uint32_t bs = rec_rd32(p);
    if (bs < 32) return 0;
    p += 4;
    const uint32_t lq = p[8], ncg = rec_rd16(p + 12), lseq = rec_rd32(p + 16);
    if ((int)rec_rd32(p) < -1 || (int)rec_rd32(p + 20) < -1 || lq < 1) return 0;
    if (32ull + lq + 4ull * ncg + (uint32_t)(lseq + 1u) / 2u + lseq > bs) return 0;
    if (bs > d.n - q - 4) return 2;
    if (p[32 + lq - 1] != 0) return 0;
    for (uint32_t i = 0; i < ncg; ++i)
        if ((p[32 + lq + 4 * i] & 15u) > 8u) return 0;
    len = 4ull + bs;
    return 1;
}
// the wave of segment s (>= 1): every lane tests candidates of its own, the lowest that passes is the guess
PLO_DEV void cut_guess_segment(const DevCut &d, uint32_t s) {
    const unsigned long long lo = (unsigned long long)s * d.seg_bytes, hi = cut_seg_end(d, s), lane = (unsigned long long)wv::lane();
    unsigned long long found = CUT_NONE;
    for (unsigned long long c0 = lo; c0 < hi && found == CUT_NONE; c0 += 64) {  // (uniform)
        const unsigned long long c = c0 + lane;
        bool ok = false;
        if (c < hi && c < d.n && d.n - c >= 36) {
            unsigned long long q = c, len = 0;
            int n_ok = 0, r = 1;
            while (n_ok < 8 && q < d.n && (r = cut_plausible(d, q, len)) == 1) {
                q += len;
                ++n_ok;
            }
            ok = n_ok == 8 || (n_ok > 0 && (q == d.n || r == 2));
        }
        const unsigned long long m = wv::ballot(ok);
        if (m) found = c0 + (unsigned long long)__builtin_ctzll(m);
    }
    if (lane == 0) d.guess[s] = found;
}

// ---- walk ---------------------------------------------------------------------------------------------------------------------------------
// segment s from `from` (inside it): its counts and where the walk left it (returned, CUT_NONE: it met the terminal position)
PLO_DEV unsigned long long cut_walk_segment(const DevCut &d, uint32_t s, unsigned long long from, bool store) {
    const unsigned long long hi = cut_seg_end(d, s);
    unsigned long long at = from, np = 0, nu = 0, ub = 0;
    bool terminal = from == CUT_NONE;
    while (!terminal && at < hi) {
        uint32_t bs;
        const int k = cut_classify(d, at, bs);
        if (k >= CUT_T_END) {
            terminal = true;
            break;
        }
        if (k == CUT_PRIMARY) ++np;
        if (k == CUT_UNMAPPED) {
            ++nu;
            ub += 4ull + bs;
        }
        at += 4ull + bs;
    }
    if (store) {
        d.land[s] = terminal ? CUT_NONE : at;
        d.cnt[s] = np;
        d.cnt[(size_t)d.n_seg + s] = nu;
        d.cnt[2 * (size_t)d.n_seg + s] = ub;
    }
    return terminal ? CUT_NONE : at;
}

// ---- resolve (one wave) -----------------------------------------------------------------------------------------------------------------------
PLO_DEV void cut_zero_segments(const DevCut &d, unsigned long long lo, unsigned long long hi) {  // dead segments [lo, hi)
    for (unsigned long long s = lo + (unsigned long long)wv::lane(); s < hi; s += 64) {
        d.guess[s] = CUT_NONE;
        d.cnt[s] = 0;
        d.cnt[(size_t)d.n_seg + s] = 0;
        d.cnt[2 * (size_t)d.n_seg + s] = 0;
    }
}
PLO_DEV void cut_resolve(const DevCut &d) {
    const int lane = wv::lane();
    unsigned long long e = 0, rewalks = 0, g = 0, l = 0;  // e: the true entry of segment s (uniform)
    uint32_t s = 0, loaded = UINT32_MAX;
    for (;;) {
        if ((s & ~63u) != loaded) {  // the guesses and landings of 64 segments at a time: the chain then runs in registers
            loaded = s & ~63u;
            const uint32_t i = loaded + (uint32_t)lane;
            g = i < d.n_seg ? d.guess[i] : CUT_NONE;
            l = i < d.n_seg ? d.land[i] : CUT_NONE;
        }
        unsigned long long next = wv::shfl(l, (int)(s & 63u));
        if (wv::shfl(g, (int)(s & 63u)) != e) {  // (uniform) the guess was wrong or missing: walk the segment again, every lane alike
            next = cut_walk_segment(d, s, e, lane == 0);
            if (lane == 0) d.guess[s] = e;
            ++rewalks;
        }
        if (next == CUT_NONE) break;  // the terminal position lies in segment s
        const uint32_t s2 = (uint32_t)(next / d.seg_bytes);  // (> s: the walk left the segment; < n_seg: next <= n)
        cut_zero_segments(d, (unsigned long long)s + 1, s2);
        e = next;
        s = s2;
    }
    cut_zero_segments(d, (unsigned long long)s + 1, d.n_seg);
    if (lane == 0) {
        d.res[CR_AT] = CUT_NONE;
        d.res[CR_REWALKS] = rewalks;
    }
}

// ---- find ---------------------------------------------------------------------------------------------------------------------------------
PLO_DEV void cut_min_u64(unsigned long long *p, unsigned long long v) {
#ifdef PLO_EMULATOR
    if (v < *p) *p = v;
#else
    atomicMin(p, v);
#endif
}
// live segment s: the host loop (bam_host.cpp:257-297) over its records with the counts of the chain in front of it
PLO_DEV void cut_find_segment(const DevCut &d, uint32_t s) {
    const size_t ns = d.n_seg;
    unsigned long long at = d.guess[s];
    d.fire[s] = CUT_NONE;
    if (at == CUT_NONE) return;
    const unsigned long long hi = cut_seg_end(d, s);
    unsigned long long np = d.start[s], nu = d.start[ns + 1 + s], ub = d.start[2 * (ns + 1) + s];
    while (at < hi) {
        unsigned long long why = CUT_NONE;
        uint32_t bs = 0;
        if (np >= d.max_records) why = PLO_CUT_MAX_RECORDS;
        else if (nu >= d.max_unmapped) why = PLO_CUT_MAX_UNMAPPED;
        else if (at >= d.max_bytes && np + nu > 0) why = PLO_CUT_MAX_BYTES;
        else {
            const int k = cut_classify(d, at, bs);
            if (k == CUT_T_END) why = d.final ? (unsigned long long)PLO_CUT_EOF : (unsigned long long)PLO_CUT_END_OF_BYTES;
            else if (k == CUT_T_TRUNC && d.n - at < 4) why = d.final ? (unsigned long long)CUT_WHY_ERR_TRUNC : (unsigned long long)PLO_CUT_END_OF_BYTES;
            else if (d.ranged && at >= d.own_bytes) why = PLO_CUT_PART_END;  // (the host's range test, bam_host.cpp:268: in front of block_size < 32)
            else if (k == CUT_T_TRUNC) why = d.final ? (unsigned long long)CUT_WHY_ERR_TRUNC : (unsigned long long)PLO_CUT_END_OF_BYTES;
            else if (k == CUT_T_SHORT) why = CUT_WHY_ERR_SHORT;
            else if (k == CUT_T_LAYOUT) why = CUT_WHY_ERR_LAYOUT;
            else if (k == CUT_T_UNM_TID) why = CUT_WHY_ERR_UNM_TID;
            else if (k == CUT_PRIMARY) ++np;
            else if (k == CUT_UNMAPPED) {
                ++nu;
                ub += 4ull + bs;
            }
        }
        if (why != CUT_NONE) {
            d.fire[s] = at;
            d.fire[ns + s] = why;
            d.fire[2 * ns + s] = np;
            d.fire[3 * ns + s] = nu;
            d.fire[4 * ns + s] = ub;
            cut_min_u64(d.res + CR_AT, at);
            return;
        }
        at += 4ull + bs;
    }
}
// one thread: the firing of the lowest offset -> the result block (the chain's terminal position always fires)
PLO_DEV void cut_result(const DevCut &d) {
    const size_t ns = d.n_seg;
    const unsigned long long at = d.res[CR_AT];
    if (at == CUT_NONE) {  // (cannot be: kept so that a fault in the passes above is a status, not an index)
        d.res[CR_WHY] = CUT_NONE;
        return;
    }
    const size_t s = (size_t)(at / d.seg_bytes);
    d.res[CR_WHY] = d.fire[ns + s];
    d.res[CR_READS] = d.fire[2 * ns + s];
    d.res[CR_UNMAPPED] = d.fire[3 * ns + s];
    d.res[CR_UNM_BYTES] = d.fire[4 * ns + s];
}

// ---- emit ---------------------------------------------------------------------------------------------------------------------------------
PLO_DEV void cut_emit_segment(const DevCut &d, uint32_t s) {
    const size_t ns = d.n_seg;
    unsigned long long at = d.guess[s];
    if (s == 0) d.unm_off[d.n_unmapped] = d.unmapped_bytes;
    if (at == CUT_NONE || at >= d.cut_at) return;
    const unsigned long long hi = cut_seg_end(d, s);
    unsigned long long np = d.start[s], nu = d.start[ns + 1 + s], ub = d.start[2 * (ns + 1) + s];
    while (at < hi && at < d.cut_at) {  // (no terminal position in front of the cut)
        uint32_t bs;
        const int k = cut_classify(d, at, bs);
        if (k == CUT_PRIMARY) d.read_rec_off[np++] = at;
        if (k == CUT_UNMAPPED) {
            d.unm_src[nu] = at;
            d.unm_off[nu++] = ub;
            ub += 4ull + bs;
        }
        at += 4ull + bs;
    }
}
// unmapped record u by nt cooperating threads
PLO_DEV void cut_copy_unmapped(const DevCut &d, unsigned long long u, int tid, int nt) {
    copy_span<true>(d.unmapped + d.unm_off[u], d.stream + d.unm_src[u], d.unm_off[u + 1] - d.unm_off[u], tid, nt);
}

// ---- the first record of a part (plo_part_start_dev) ---------------------------------------------------------------------------------
// The loop of plo_bam_open_range (bam_host.cpp:183-202) over stream[0, n), the inflated bytes from the first byte of the part's first block:
// every candidate offset p with p + 36 <= n is an ACCEPT (a chain of eight plausible records, or of at least one that ends exactly at n with
// `final`), a CUT (a chain of at least one that the end of the bytes cuts short, without `final`: the host buffers more) or a reject; the
// lowest p that is no reject decides.  A lane per candidate, 64 candidates per wave step, tiles of `tile` candidates dealt in ascending order;
// the lowest accept and the lowest cut are kept in two 64-bit minima, and a wave leaves when its step lies above one of them: whatever it
// would find there is not the lowest, so the result does not depend on which waves left.
enum { PS_ACCEPT = 0, PS_CUT = 1, PS_TICKET = 2, PS_WORDS = 4 };

struct DevPart {
    const uint8_t *stream;
    unsigned long long n;       // stream_bytes
    unsigned long long n_cand;  // candidates: n - 35, or 0
    unsigned long long tile;    // candidates per tile, a multiple of 64
    unsigned long long n_tiles;
    uint32_t n_ref;
    int final;
    unsigned long long *res;  // [PS_WORDS]: both minima CUT_NONE and the ticket 0 at launch
};

// plausible_record (bam_host.cpp:113-130) in full, the reference ids against the header's list included: 0 = no record here, 1 = a record
// (len), 2 = the bytes end inside it (what the host's `ran_out` says of a record plausible_record refused).  q <= n
PLO_DEV int part_plausible(const DevPart &d, unsigned long long q, unsigned long long &len) {
    if (d.n - q < 36) return 2;
    const uint8_t *p = d.stream + q;
    const uint32_t bs = rec_rd32(p);
    if (bs < 32) return 0;
    if (bs > d.n - q - 4) return 2;  // (before anything behind the fixed fields is read)
    p += 4;
    const int32_t tid = (int32_t)rec_rd32(p), mtid = (int32_t)rec_rd32(p + 20), n_ref = (int32_t)d.n_ref;
    if (tid < -1 || tid >= n_ref || mtid < -1 || mtid >= n_ref) return 0;
    const uint32_t lq = p[8], ncg = rec_rd16(p + 12), lseq = rec_rd32(p + 16);
    if (lq < 1 || 32ull + lq + 4ull * ncg + (uint32_t)(lseq + 1u) / 2u + lseq > bs) return 0;
    if (p[32 + lq - 1] != 0) return 0;
    for (uint32_t i = 0; i < ncg; ++i)
        if ((p[32 + lq + 4 * i] & 15u) > 8u) return 0;
    len = 4ull + bs;
    return 1;
}
// candidate p (p + 36 <= n): 0 = reject, 1 = accept, 2 = cut
PLO_DEV int part_candidate(const DevPart &d, unsigned long long p) {
    unsigned long long q = p, len = 0;
    int ok = 0, r = 1;
    while (ok < 8 && !(q == d.n && d.final) && (r = part_plausible(d, q, len)) == 1) {
        q += len;
        ++ok;
    }
    if (ok == 8 || (ok > 0 && q == d.n && d.final)) return 1;
    return r == 2 && !d.final && ok > 0 ? 2 : 0;
}
PLO_DEV unsigned long long part_peek_u64(const unsigned long long *p) {
#ifdef PLO_EMULATOR
    return *p;
#else
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
}
// the wave's tile t (< n_tiles).  false: this tile reaches above a candidate that is no reject, and so does every later one
PLO_DEV bool part_start_tile(const DevPart &d, unsigned long long t) {
    const unsigned long long lo = t * d.tile, hi = lo + d.tile < d.n_cand ? lo + d.tile : d.n_cand, lane = (unsigned long long)wv::lane();
    for (unsigned long long c0 = lo; c0 < hi; c0 += 64) {  // (uniform)
        const unsigned long long a = part_peek_u64(d.res + PS_ACCEPT), b = part_peek_u64(d.res + PS_CUT);
        if (c0 > wv::bcast_first(a < b ? a : b)) return false;
        const unsigned long long c = c0 + lane;
        const int k = c < hi ? part_candidate(d, c) : 0;
        const unsigned long long m = wv::ballot(k != 0);
        if (m) {
            if (lane == (unsigned long long)__builtin_ctzll(m)) cut_min_u64(d.res + (k == 1 ? PS_ACCEPT : PS_CUT), c);
            return false;
        }
    }
    return true;
}

}  // namespace plo
