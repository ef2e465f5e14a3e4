// index_core.hpp -- what a BAM index (BAI, SAMv1 5.2) needs of every record of a coordinate-sorted buffer (plo_records_index_dev): where
// the record stands, its reference, its 0-based half-open interval [beg, end) on it, whether FLAG & 4 is set, and reg2bin(beg, end).
//   refID >= 0   beg = max(pos, 0); rlen = the lengths of the ops M, D, N, =, X (codes 0, 2, 3, 7, 8) of the in-record CIGAR, a 64-bit sum
//                (the placeholder <l_seq>S<ref_len>N of a record with more than 65 535 ops gives ref_len by the same sum; the codes 9-15
//                consume nothing); end = beg + rlen, or beg + 1 when FLAG & 4 is set or rlen == 0
//   refID == -1  beg = -1, end = 0, bin 4680
// A record is refused -- before a byte of it is trusted -- for what plo_records_sort_dev refuses (sort_core.hpp, SORT_ERR_*), and then, in
// this order, for a CIGAR that leaves the record, an end behind 2^29 (BAI cannot address it), and a pair (refID < 0 ? n_ref : refID, pos)
// below the previous record's (the strand bit of the sort key is no part of it: a buffer sorted by position alone passes).
// The file has two parts.  The first is plain C++ without a wave primitive: the rule of one record by one thread, which the host's merge
// (bam_host.cpp) compiles too.  The second (behind PLO_WAVE, for the device and the emulator) gives a record to a WAVE: the fixed fields are
// read by every lane from the same addresses, the ops a lane each, 64 at a trip, coalesced; the lanes' sums meet in two DPP reductions of
// 24 bits each (a lane's sum stays below 2^38: 1 024 trips of an op below 2^28).  Both parts end in index_finish, so they cannot disagree.
// The same functions run under the CPU emulator (tests/emu/emu_index.cpp).
#pragma once
#include <stdint.h>

#ifndef PLO_HD
#define PLO_HD inline
#endif

namespace plo {

constexpr int INDEX_NO_RECORD = 0x7fffffff;
constexpr uint32_t INDEX_MAX_RECORDS = 0x07ffffffu;  // the lowest offender and its kind share one word: record << 4 | kind
constexpr long long INDEX_MAX_END = 1ll << 29;
constexpr uint32_t INDEX_BIN_UNPLACED = 4680;
// what the lowest offending record broke, behind SORT_ERR_* (1 .. 5)
enum { INDEX_ERR_CIGAR = 6,   // 36 + l_read_name + 4 n_cigar_op > 4 + block_size: the CIGAR leaves the record
       INDEX_ERR_END = 7,     // end > 2^29
       INDEX_ERR_ORDER = 8 }; // (refID < 0 ? n_ref : refID, pos) below the previous record's

struct IndexEntry {  // plo_index_entry (portello_liftover.h)
    uint64_t off;
    int32_t ref_id, beg, end;
    uint32_t flags;  // bit 0: FLAG & 4; bits 16 .. 31: the bin
};
static_assert(sizeof(IndexEntry) == 24, "plo_index_entry is 24 bytes");

PLO_HD unsigned index_rd16(const uint8_t *p) { return (unsigned)p[0] | ((unsigned)p[1] << 8); }
PLO_HD unsigned index_rd32(const uint8_t *p) { return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24); }

// SAMv1 5.3, for 0 <= beg < end <= 2^29
PLO_HD uint32_t index_reg2bin(long long beg, long long end) {
    --end;
    if (beg >> 14 == end >> 14) return (uint32_t)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (uint32_t)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (uint32_t)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (uint32_t)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (uint32_t)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

// the reference bases one CIGAR word consumes: its length for M, D, N, =, X (bits 0, 2, 3, 7, 8 of 0x18d), nothing for the other codes
PLO_HD unsigned long long index_op_reflen(unsigned op) { return ((0x18du >> (op & 15u)) & 1u) ? (unsigned long long)(op >> 4) : 0ull; }

// does the CIGAR of the record at p (len bytes, the block_size word included) stay inside it?  l_read_name at +12, n_cigar_op at +16
PLO_HD bool index_cigar_fits(const uint8_t *p, unsigned long long len, unsigned &cigar_at, unsigned &n_cigar) {
    cigar_at = 36u + p[12];
    n_cigar = index_rd16(p + 16);
    return (unsigned long long)cigar_at + 4ull * n_cigar <= len;
}

// the entry of a record with these fixed fields and this reference length -> 0 or INDEX_ERR_END
PLO_HD int index_finish(int ref, int pos, unsigned flag, unsigned long long rlen, unsigned long long off, IndexEntry &e) {
    const unsigned unm = (flag >> 2) & 1u;
    e.off = off;
    if (ref < 0) {
        e.ref_id = -1;
        e.beg = -1;
        e.end = 0;
        e.flags = unm | (INDEX_BIN_UNPLACED << 16);
        return 0;
    }
    const long long beg = pos < 0 ? 0 : pos;
    const long long end = (unm || rlen == 0) ? beg + 1 : beg + (long long)rlen;
    e.ref_id = ref;
    e.beg = (int32_t)beg;
    e.end = (int32_t)(end > INDEX_MAX_END ? 0 : end);
    e.flags = unm;
    if (end > INDEX_MAX_END) return INDEX_ERR_END;
    e.flags |= index_reg2bin(beg, end) << 16;
    return 0;
}

// is (ref, pos) below the previous record's (pref, ppos)?
PLO_HD bool index_order_breaks(int ref, int pos, int pref, int ppos, uint32_t n_ref) {
    const uint32_t a = ref < 0 ? n_ref : (uint32_t)ref, b = pref < 0 ? n_ref : (uint32_t)pref;
    return a < b || (a == b && pos < ppos);
}

// One record by one thread: p points at its block_size word, len = block_size + 4 >= 36, refID and pos have passed the sort's check.
// -> 0, INDEX_ERR_CIGAR or INDEX_ERR_END (the order is the caller's: it knows the record in front)
PLO_HD int index_entry_scalar(const uint8_t *p, unsigned long long len, unsigned long long off, IndexEntry &e) {
    unsigned at, nc;
    if (!index_cigar_fits(p, len, at, nc)) return INDEX_ERR_CIGAR;
    unsigned long long rlen = 0;
    for (unsigned k = 0; k < nc; ++k) rlen += index_op_reflen(index_rd32(p + at + 4u * k));
    return index_finish((int)index_rd32(p + 4), (int)index_rd32(p + 8), index_rd16(p + 18), rlen, off, e);
}

}  // namespace plo

#ifdef PLO_WAVE
#include "sort_core.hpp"

namespace plo {

struct DevBai {
    DevSort s;          // the input fields only (bytes, n_bytes, n, record_off, n_ref): what sort_check_record reads
    IndexEntry *entry;  // [n]
    int *err;           // [1] lowest offending record << 4 | what it broke (INDEX_NO_RECORD: none)
    unsigned *n_placed; // [1] records with refID >= 0
};

// the sum over the wave of per-lane values below 2^48, in every lane: two 32-bit DPP reductions of 24 bits a lane (64 x 2^24 = 2^30)
PLO_DEV unsigned long long index_wave_sum(unsigned long long v) {
    const unsigned lo = (unsigned)wv::reduce_add((int)(unsigned)(v & 0xffffffull));
    const unsigned hi = (unsigned)wv::reduce_add((int)(unsigned)((v >> 24) & 0xffffffull));
    return (unsigned long long)lo + ((unsigned long long)hi << 24);
}

// Record i by one wave (i wave-uniform; every lane takes the same path up to the op loop) -> 1 when it is placed (refID >= 0) and accepted.
// Nothing outside [bytes, bytes + n_bytes) is read: the fixed fields only behind sort_check_record, the ops only behind index_cigar_fits,
// the record in front only when it passes sort_check_record itself (one that does not is a lower offender, and decides the call).
PLO_DEV unsigned index_record(const DevBai &d, uint32_t i) {
    unsigned long long key, len;
    int kind = sort_check_record(d.s, i, key, len);
    const unsigned long long off = kind == SORT_ERR_OFFSET ? 0ull : d.s.record_off[i];
    const uint8_t *p = d.s.bytes + off;
    IndexEntry e;
    e.off = off;
    e.ref_id = -1;
    e.beg = -1;
    e.end = 0;
    e.flags = 0;
    unsigned at = 0, nc = 0;
    if (!kind && !index_cigar_fits(p, len, at, nc)) kind = INDEX_ERR_CIGAR;
    if (kind) nc = 0;  // (wave-uniform: the reductions below are reached by every lane either way)
    unsigned long long part = 0;
#pragma unroll 4
    for (unsigned k = (unsigned)wv::lane(); k < nc; k += PLO_WAVE) part += index_op_reflen(rec_rd32(p + at + 4u * k));
    const unsigned long long rlen = index_wave_sum(part);
    if (!kind) {
        const int ref = (int)rec_rd32(p + 4), pos = (int)rec_rd32(p + 8);
        kind = index_finish(ref, pos, rec_rd16(p + 18), rlen, off, e);
        if (!kind && i) {
            unsigned long long pkey, plen;
            if (!sort_check_record(d.s, i - 1, pkey, plen)) {
                const uint8_t *q = d.s.bytes + d.s.record_off[i - 1];
                if (index_order_breaks(ref, pos, (int)rec_rd32(q + 4), (int)rec_rd32(q + 8), d.s.n_ref)) kind = INDEX_ERR_ORDER;
            }
        }
    }
    if (wv::lane() == 0) {
        if (kind) wv::atomic_min(d.err, (int)((i << 4) | (unsigned)kind));
        else d.entry[i] = e;
    }
    return !kind && e.ref_id >= 0 ? 1u : 0u;
}

// the records w, w + nw, ... by wave w of nw
PLO_DEV void index_records(const DevBai &d, uint32_t w, uint32_t nw) {
    unsigned placed = 0;
    for (uint32_t i = w; i < d.s.n; i += nw) placed += index_record(d, i);
    if (wv::lane() == 0 && placed) wv::atomic_add_global(d.n_placed, placed);
}

}  // namespace plo
#endif
