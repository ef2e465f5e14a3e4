// sort_core.hpp -- the window's output records in coordinate order on the device (plo_records_sort_dev).  The key of a record is
//   (refID < 0 ? n_ref : refID) << 32 | (pos + 1) << 1 | reverse flag          (refID at +4, pos at +8, flag at +18 from the block_size word)
// and the records are ordered by the pair (key, input index), which is unique: the result does not depend on the launch geometry.
//   keys   (a workgroup per tile of SORT_TILE records): every record is checked (offsets, length, block_size, refID, pos) before a byte of
//          it is trusted, its length and key are made, and the tile's (key, index) pairs are sorted in LDS by a bitonic network.  A pair
//          order is total, so the network's instability does not show.  The lowest offending record goes out by an atomic min
//   merge  (a thread per pair, one launch per doubling): the pair's place in the merged run is its place in its own run plus its rank
//          in the sibling run, found by a binary search.  The runs are ranges of input indices, the left one the lower: on equal keys a
//          left pair goes first, so the search compares keys only (lower bound for a left pair, upper bound for a right one)
//   gather (a thread per record): the lengths in sorted order; the 64-bit scan of records_core.hpp makes the new record_off of them
//   copy   (a wave per SORT_COPY_CHUNK bytes of OUTPUT): the records that reach into the chunk are found by a search over the new offsets,
//          the part of each inside the chunk goes through copy_span (records_core.hpp): a 200 kB record is a dozen waves' work, a short one
//          one wave's, and the chunks tile the output, so every byte is stored once
// The same functions run under the CPU emulator (tests/emu/emu_sort.cpp).
#pragma once
#include <plo_wave.hpp>
#include <stdint.h>

#include "records_core.hpp"

namespace plo {

constexpr int SORT_NO_RECORD = 0x7fffffff;
constexpr uint32_t SORT_TILE = 1024, SORT_THREADS = 256, SORT_MIN_RECORD = 36;
constexpr unsigned long long SORT_COPY_CHUNK = 16384;
// what the lowest offending record broke (stored in its slot of DevSort::len)
enum { SORT_ERR_OFFSET = 1,  // record_off[0] != 0, record_off decreases or passes n_bytes, record_off[n] != n_bytes
       SORT_ERR_SHORT = 2,   // fewer than the 36 bytes of block_size + the fixed fields
       SORT_ERR_BLOCK = 3,   // block_size + 4 differs from the record's length
       SORT_ERR_REFID = 4,   // refID outside [-1, n_ref)
       SORT_ERR_POS = 5 };   // pos outside [-1, 2^31 - 2]

struct DevSort {
    // input (plo_sort_in)
    const uint8_t *bytes;
    unsigned long long n_bytes;
    uint32_t n;
    const uint64_t *record_off;
    uint32_t n_ref;
    // workspace and output
    unsigned long long *key[2];  // [n] each: the merge passes go from one to the other
    uint32_t *idx[2];
    unsigned long long *len;     // [n] input order; an offending record's slot holds its SORT_ERR_*
    unsigned long long *slen;    // [n] sorted order
    const unsigned long long *new_off;  // [n + 1] their exclusive scan
    uint8_t *out;
    int *err;            // [1] the lowest offending record (SORT_NO_RECORD: none)
    unsigned *n_mapped;  // [1] records with refID >= 0
};

// record i: its length and key, or what it breaks.  Nothing outside [bytes, bytes + n_bytes) is read.
PLO_DEV int sort_check_record(const DevSort &d, uint32_t i, unsigned long long &key, unsigned long long &len) {
    const unsigned long long a = d.record_off[i], b = d.record_off[i + 1];
    key = ~0ull;
    len = 0;
    if ((i == 0 && a != 0) || b < a || b > d.n_bytes || (i + 1 == d.n && b != d.n_bytes)) return SORT_ERR_OFFSET;
    len = b - a;
    if (len < SORT_MIN_RECORD) return SORT_ERR_SHORT;
    const uint8_t *p = d.bytes + a;
    if ((unsigned long long)rec_rd32(p) + 4 != len) return SORT_ERR_BLOCK;
    const int ref = (int)rec_rd32(p + 4), pos = (int)rec_rd32(p + 8);
    if (ref < -1 || (ref >= 0 && (uint32_t)ref >= d.n_ref)) return SORT_ERR_REFID;
    if (pos < -1 || pos > 0x7ffffffe) return SORT_ERR_POS;
    const unsigned rev = (rec_rd16(p + 18) >> 4) & 1u;
    key = ((unsigned long long)(ref < 0 ? d.n_ref : (uint32_t)ref) << 32) | ((unsigned long long)(uint32_t)(pos + 1) << 1) | rev;
    return 0;
}

PLO_DEV bool sort_pair_gt(unsigned long long ka, uint32_t ia, unsigned long long kb, uint32_t ib) { return ka > kb || (ka == kb && ia > ib); }

// tile `tile` by a workgroup of SORT_THREADS threads: check, lengths, keys, the bitonic network over lk / li (LDS, SORT_TILE entries each);
// the sorted pairs go to key[0] / idx[0].  Slots behind the last record hold (~0, ~0), above every pair of a record.
PLO_DEV void sort_tile(const DevSort &d, uint32_t tile, unsigned long long *lk, uint32_t *li) {
    const uint32_t tid = (uint32_t)wv::wave_id() * 64u + (uint32_t)wv::lane();
    const uint32_t base = tile * SORT_TILE;
    unsigned mapped = 0;
    for (uint32_t t = tid; t < SORT_TILE; t += SORT_THREADS) {  // (the same trips for every thread)
        const uint32_t i = base + t;
        unsigned long long key = ~0ull, len = 0;
        uint32_t ix = 0xffffffffu;
        bool m = false;
        if (i < d.n) {
            const int e = sort_check_record(d, i, key, len);
            if (e) wv::atomic_min(d.err, (int)i);
            d.len[i] = e ? (unsigned long long)e : len;
            ix = i;
            m = !e && (uint32_t)(key >> 32) < d.n_ref;
        }
        lk[t] = key;
        li[t] = ix;
        mapped += (unsigned)__builtin_popcountll(wv::ballot(m));
    }
    if (wv::lane() == 0 && mapped) wv::atomic_add_global(d.n_mapped, mapped);
    wv::block_sync();
    for (uint32_t k = 2; k <= SORT_TILE; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = tid; t < SORT_TILE / 2; t += SORT_THREADS) {
                const uint32_t a = ((t & ~(j - 1)) << 1) | (t & (j - 1)), b = a | j;
                const unsigned long long ka = lk[a], kb = lk[b];
                const uint32_t ia = li[a], ib = li[b];
                if (sort_pair_gt(ka, ia, kb, ib) == ((a & k) == 0)) {
                    lk[a] = kb;
                    li[a] = ib;
                    lk[b] = ka;
                    li[b] = ia;
                }
            }
            wv::block_sync();
        }
    for (uint32_t t = tid; t < SORT_TILE; t += SORT_THREADS)
        if (base + t < d.n) {
            d.key[0][base + t] = lk[t];
            d.idx[0][base + t] = li[t];
        }
}

// pair g of the sorted runs of `run` pairs in (sk, si) -> its place in the merge of its run with the sibling run, in (dk, di)
PLO_DEV void sort_merge_pair(const unsigned long long *sk, const uint32_t *si, unsigned long long *dk, uint32_t *di, uint32_t n, uint32_t run, uint32_t g) {
    const unsigned long long k = sk[g];
    const uint32_t r = g / run;
    const bool right = (r & 1u) != 0;
    const unsigned long long own0 = (unsigned long long)r * run, pair0 = (unsigned long long)(r & ~1u) * run;
    unsigned long long s0 = (unsigned long long)(r ^ 1u) * run, s1 = s0 + run;
    if (s0 > n) s0 = n;
    if (s1 > n) s1 = n;
    unsigned long long lo = s0, hi = s1;
    while (lo < hi) {  // the sibling's pairs in front of this one: keys below it, and for a right pair the equal keys too
        const unsigned long long mid = (lo + hi) >> 1, km = sk[mid];
        if (km < k || (right && km == k)) lo = mid + 1;
        else hi = mid;
    }
    const unsigned long long at = pair0 + (g - own0) + (lo - s0);
    dk[at] = k;
    di[at] = si[g];
}

// bytes [chunk * SORT_COPY_CHUNK, + SORT_COPY_CHUNK) of the output by nt cooperating threads
PLO_DEV void sort_copy_chunk(const DevSort &d, const uint32_t *perm, unsigned long long chunk, int tid, int nt) {
    const unsigned long long lo = chunk * SORT_COPY_CHUNK;
    unsigned long long hi = lo + SORT_COPY_CHUNK;
    if (hi > d.n_bytes) hi = d.n_bytes;
    uint32_t a = 0, b = d.n;
    while (a < b) {  // the first record that ends behind lo
        const uint32_t m = a + ((b - a) >> 1);
        if (d.new_off[m + 1] > lo) b = m;
        else a = m + 1;
    }
    for (uint32_t j = a; j < d.n; ++j) {
        const unsigned long long r0 = d.new_off[j], r1 = d.new_off[j + 1];
        if (r0 >= hi) break;
        const unsigned long long s = r0 > lo ? r0 : lo, e = r1 < hi ? r1 : hi;
        copy_span<true>(d.out + s, d.bytes + d.record_off[perm[j]] + (s - r0), e - s, tid, nt);
    }
}

}  // namespace plo
