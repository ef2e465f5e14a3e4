// merge_core.hpp -- the k-way merge of coordinate-sorted record buffers that each lie in an allocation of their own
// (plo_runs_merge_plan_dev / plo_runs_merge_emit_dev).  The records are numbered run-major, g = run_first[r] + place, and the merged order
// is the pair (key, g) with sort_check_record's key (sort_core.hpp): unique, so the result does not depend on the launch geometry and is
// what plo_records_sort_dev gives over the runs' concatenation.
//   keys    (a thread per record): the record's run by a search over run_first, the checks of sort_check_record against the run's own
//           bytes / record_off before a byte of it is trusted, and MERGE_ERR_ORDER: a key below the key of the record before it in the run.
//           The lowest offending g goes out by an atomic min, what it broke into its slot of len
//   rank    (a thread per pair, one launch per round t < ceil(log2(n_runs))): the groups of round t are 2^t consecutive runs, group m lies at
//           [run_first[m 2^t], run_first[(m + 1) 2^t]) in every round.  A pair's place is its place in its own group plus its rank in the
//           sibling group; the left group holds the lower g, so the search compares keys only (lower bound from the left, upper bound from
//           the right).  A group without a sibling is copied.  No LDS: the runs arrive sorted
//   gather  (a thread per record; not for a refused input): the lengths in merged order; the 64-bit scan of records_core.hpp makes the merged record_off of them
//   chunks  (ONE lane): n_mapped by a search over the merged keys, and the chunk table by one search over record_off per chunk: chunk c
//           begins at record chunk_first[c] and holds as many following records as keep its bytes <= chunk_bytes, never fewer than one
//   copy    (a wave per MERGE_COPY_PIECE bytes of a chunk's OUTPUT): the records that reach into the piece are found by a search over the merged
//           offsets, the source of each is runs[r].bytes + runs[r].record_off[place], the part inside the piece goes through copy_span: the
//           pieces tile the chunk, so every byte is stored once; the waves also rebase the chunk's record_off
// The same functions run under the CPU emulator (tests/emu/emu_merge.cpp).
#pragma once
#include <plo_wave.hpp>
#include <stdint.h>

#include "sort_core.hpp"

namespace plo {

constexpr uint32_t MERGE_MAX_RUNS = 4096, MERGE_THREADS = 256, MERGE_NO_RECORD = 0xffffffffu;
constexpr unsigned long long MERGE_COPY_PIECE = 16384;
enum { MERGE_ERR_ORDER = 6 };  // behind SORT_ERR_*: the key is lower than the key of the record before it in the same run

struct MergeRun {  // plo_merge_run
    const uint8_t *bytes;
    unsigned long long n_bytes;
    uint32_t n_records;
    const uint64_t *record_off;
};

struct DevMerge {
    const MergeRun *runs;       // [n_runs] device copy of the descriptor table
    const uint32_t *run_first;  // [n_runs + 1] g of every run's first record; run_first[n_runs] == n
    uint32_t n_runs, n, n_ref;
    unsigned long long chunk_bytes;
    // workspace and output
    unsigned long long *key[2];  // [n] each: the rank rounds go from one to the other
    uint32_t *src[2];
    uint16_t *run_of;            // [n] the run of record g (and of place g of the key / src arrays: the groups keep their ranges)
    unsigned long long *len;     // [n] by g; an offending record's slot holds what it broke
    unsigned long long *mlen;    // [n] merged order
    const unsigned long long *off;  // [n + 1] their exclusive scan
    int *err;                    // [1] the lowest offending g, as (int)(g ^ 2^31): the signed order of these is the unsigned order of g
    uint32_t *res;               // [2] n_mapped, n_chunks
    uint32_t *chunk_first;       // [chunk_cap + 1]
    unsigned long long *chunk_off;  // [chunk_cap + 1] merged byte offset of the chunk's first record
    uint32_t chunk_cap;
};

PLO_HD int merge_err_word(uint32_t g) { return (int)(g ^ 0x80000000u); }

// the run of record g: the last r with run_first[r] <= g (an empty run shares its run_first with the run behind it)
PLO_DEV uint32_t merge_run_of(const uint32_t *run_first, uint32_t n_runs, uint32_t g) {
    uint32_t lo = 0, hi = n_runs;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (run_first[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}

PLO_DEV DevSort merge_run_view(const DevMerge &d, uint32_t r) {
    DevSort s = {};
    s.bytes = d.runs[r].bytes;
    s.n_bytes = d.runs[r].n_bytes;
    s.n = d.runs[r].n_records;
    s.record_off = d.runs[r].record_off;
    s.n_ref = d.n_ref;
    return s;
}

// record g: run, check, length, key; (key, g) into place g of key[0] / src[0]
PLO_DEV void merge_key_record(const DevMerge &d, uint32_t g) {
    const uint32_t r = merge_run_of(d.run_first, d.n_runs, g), place = g - d.run_first[r];
    const DevSort s = merge_run_view(d, r);
    unsigned long long key, len;
    int e = sort_check_record(s, place, key, len);
    if (!e && place) {  // (a record before this one that is refused itself is the lower offender: what is reported here then does not show)
        unsigned long long pkey, plen;
        if (!sort_check_record(s, place - 1, pkey, plen) && key < pkey) {
            e = MERGE_ERR_ORDER;
            key = ~0ull;
        }
    }
    if (e) wv::atomic_min(d.err, merge_err_word(g));
    d.len[g] = e ? (unsigned long long)e : len;
    d.run_of[g] = (uint16_t)r;
    d.key[0][g] = key;
    d.src[0][g] = g;
}

// round t: the pair at place p of (sk, ss) -> its place in the merge of its group of 2^t runs with the sibling group, in (dk, ds)
PLO_DEV void merge_rank_pair(const DevMerge &d, const unsigned long long *sk, const uint32_t *ss, unsigned long long *dk, uint32_t *ds, uint32_t t, uint32_t p) {
    const unsigned long long k = sk[p];
    const uint32_t m = (uint32_t)d.run_of[p] >> t, sib = m ^ 1u;
    const bool right = (m & 1u) != 0;
    const uint32_t nr = d.n_runs;
    const uint32_t own0 = d.run_first[m << t], pair0 = d.run_first[(m & ~1u) << t];
    const uint32_t s0 = d.run_first[(sib << t) < nr ? (sib << t) : nr], s1 = d.run_first[((sib + 1u) << t) < nr ? ((sib + 1u) << t) : nr];
    uint32_t lo = s0, hi = s1;
    while (lo < hi) {  // the sibling's pairs in front of this one: keys below it, and for a right pair the equal keys too
        const uint32_t mid = lo + ((hi - lo) >> 1);
        const unsigned long long km = sk[mid];
        if (km < k || (right && km == k)) lo = mid + 1;
        else hi = mid;
    }
    const uint32_t at = pair0 + (p - own0) + (lo - s0);
    dk[at] = k;
    ds[at] = ss[p];
}

// the length of the record at merged place j.  Nothing for a refused input: its keys are in no order, the rank rounds then leave places
// of src unwritten, and no such value may become an index
PLO_DEV void merge_gather(const DevMerge &d, const uint32_t *src, uint32_t j) {
    if (*d.err != merge_err_word(MERGE_NO_RECORD)) return;
    d.mlen[j] = d.len[src[j]];
}

// one lane: n_mapped and the chunk table of the merged stream (key, src, off final).  Nothing for a refused input.
PLO_DEV void merge_chunks(const DevMerge &d, const unsigned long long *key) {
    d.res[0] = d.res[1] = 0;
    if (*d.err != merge_err_word(MERGE_NO_RECORD)) return;
    uint32_t lo = 0, hi = d.n;
    const unsigned long long first_unplaced = (unsigned long long)d.n_ref << 32;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (key[mid] < first_unplaced) lo = mid + 1;
        else hi = mid;
    }
    d.res[0] = lo;
    uint32_t c = 0, first = 0;
    while (first < d.n && c < d.chunk_cap) {
        d.chunk_first[c] = first;
        d.chunk_off[c] = d.off[first];
        ++c;
        const unsigned long long base = d.off[first];
        uint32_t a = first + 1, b = d.n;  // the last e in [first + 1, n] with off[e] - base <= chunk_bytes (first + 1 where there is none)
        while (a < b) {
            const uint32_t mid = a + ((b - a + 1) >> 1);
            if (d.off[mid] - base <= d.chunk_bytes) a = mid;
            else b = mid - 1;
        }
        first = a;
    }
    d.chunk_first[c] = d.n;
    d.chunk_off[c] = d.off[d.n];
    d.res[1] = first < d.n ? 0xffffffffu : c;  // (the table's bound holds by construction: two chunks in a row pass chunk_bytes)
}

struct DevMergeEmit {
    const MergeRun *runs;
    const uint32_t *run_first;
    const uint16_t *run_of;
    const uint32_t *src;             // merged place -> g
    const unsigned long long *off;   // merged record_off
    uint32_t first, n;               // the chunk: records [first, first + n)
    uint8_t *out;                    // [off[first + n] - off[first]]
    unsigned long long *out_off;     // [n + 1] rebased
};

// bytes [piece * MERGE_COPY_PIECE, + MERGE_COPY_PIECE) of the chunk's output by nt cooperating threads
PLO_DEV void merge_copy_piece(const DevMergeEmit &d, unsigned long long piece, int tid, int nt) {
    const unsigned long long base = d.off[d.first], total = d.off[d.first + d.n] - base;
    const unsigned long long lo = piece * MERGE_COPY_PIECE;
    unsigned long long hi = lo + MERGE_COPY_PIECE;
    if (hi > total) hi = total;
    uint32_t a = d.first, b = d.first + d.n;
    while (a < b) {  // the first record of the chunk that ends behind lo
        const uint32_t m = a + ((b - a) >> 1);
        if (d.off[m + 1] - base > lo) b = m;
        else a = m + 1;
    }
    for (uint32_t j = a; j < d.first + d.n; ++j) {
        const unsigned long long r0 = d.off[j] - base, r1 = d.off[j + 1] - base;
        if (r0 >= hi) break;
        const unsigned long long s = r0 > lo ? r0 : lo, e = r1 < hi ? r1 : hi;
        const uint32_t g = d.src[j], r = d.run_of[g];
        const MergeRun &run = d.runs[r];
        copy_span<true>(d.out + s, run.bytes + run.record_off[g - d.run_first[r]] + (s - r0), e - s, tid, nt);
    }
}

// the chunk's record_off counted from its first byte: thread `tid` of `nt` in all
PLO_DEV void merge_rebase(const DevMergeEmit &d, unsigned long long tid, unsigned long long nt) {
    const unsigned long long base = d.off[d.first];
    for (unsigned long long j = tid; j <= d.n; j += nt) d.out_off[j] = d.off[d.first + j] - base;
}

}  // namespace plo
