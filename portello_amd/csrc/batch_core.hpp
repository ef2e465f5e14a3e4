// batch_core.hpp -- the liftover batch of a window built on the device: the arrays of window_batch (bam_host.cpp) in its `views` mode,
// i.e. get_seq_order_read_split_segments (split_read.rs:56-155) of every primary record as split_segments / real_cigar /
// read_clip_positions / parse_cigar_text (bam_internal.hpp) restate it, with the SA text cut as sa_tag_parser.rs:26-59 cuts it.
//   table (a thread per contig): open-addressing hash table over the caller's contig names, built on every call
//   plan  (a wave per read):     bounds of the source record, the aux walk to the first CG and the first SA, every SA segment parsed and
//                                checked in the host's order -> segment count, op count, the read's first failure
//   scan  (waves):               the 64-bit exclusive scans of records_core.hpp over both counts
//   emit  (a wave per read):     the per-read arrays, the segments in sequencing order (a rank count: stable, any number of segments),
//                                the CIGAR ops (the primary's copied, an SA segment's parsed from its text with one lane per op)
// A wave works on one read; values that every lane holds alike are called uniform.  The same functions run under the CPU emulator
// (tests/emu/emu_batch.cpp).
#pragma once
#include <plo_wave.hpp>
#include <stdint.h>

#include "records_core.hpp"

namespace plo {

// per-read plan: BB_PLAN_WORDS dwords
enum { BP_NCIG = 0,     // ops of the read's real CIGAR (the record's, or its CG:B,I field's behind the placeholder)
       BP_CIG_OFF = 1,  // their offset behind the block_size word
       BP_SA_OFF = 2,   // offset of the SA text behind the block_size word, 0: no SA field
       BP_SA_LEN = 3,   // its length without the NUL
       BB_PLAN_WORDS = 4 };
// d.err: [0] the lowest read with a data failure (BB_NO_READ: none), [1 + k] number of reads that failed bounds check REC_ERR_* k
enum { BB_ERR_WORDS = 1 + REC_ERR_N };
constexpr int BB_NO_READ = 0x7fffffff;

struct DevBatchBuild {
    // input (plo_batch_build_in)
    const uint8_t *records;
    unsigned long long records_bytes;
    const uint64_t *read_rec_off;
    uint32_t n_reads;
    uint32_t n_contigs;
    const uint32_t *contig_name_off;
    const uint8_t *contig_names;
    // label table: contig + 1 per slot, 0 = free; table_mask + 1 slots (a power of two, at least twice the contigs)
    uint32_t *table;
    uint32_t table_mask;
    // plan
    uint32_t *plan;                   // [n_reads][BB_PLAN_WORDS]
    unsigned long long *size;         // [2][n_reads]: segments, CIGAR ops of every read
    const unsigned long long *start;  // [2][n_reads + 1]: their exclusive scans
    uint32_t *err_kind;               // [n_reads] PLO_BB_ERR_*
    int *err;                         // [BB_ERR_WORDS]
    // emit: per segment in TEXT order (the primary first), at the read's first segment + its place in the text
    unsigned long long *t_key;  // so_start
    uint32_t *t_nops, *t_ctext, *t_clen, *t_contig, *t_dst;
    long long *t_pos;
    uint8_t *t_fwd;
    // output
    uint8_t *read_is_reverse;
    uint32_t *read_seq_len;
    uint64_t *read_seq_off, *read_qual_off;
    uint16_t *read_flags;
    uint32_t *seg_read, *seg_contig, *seg_cigar_off, *cigar;
    int64_t *seg_pos;
    uint8_t *seg_fwd;
};

// ---- label table ------------------------------------------------------------------------------------------------------------------------
PLO_DEV uint32_t bb_hash(const uint8_t *s, uint32_t n) {  // FNV-1a
    uint32_t h = 2166136261u;
    for (uint32_t i = 0; i < n; ++i) h = (h ^ s[i]) * 16777619u;
    return h;
}
// the slot's value if it was taken, 0 if this call took it
PLO_DEV uint32_t bb_slot_take(uint32_t *slot, uint32_t v) {
#ifdef PLO_EMULATOR
    const uint32_t old = *slot;
    if (!old) *slot = v;
    return old;
#else
    return atomicCAS(slot, 0u, v);
#endif
}
PLO_DEV void bb_table_insert(const DevBatchBuild &d, uint32_t c) {
    const uint32_t o = d.contig_name_off[c], n = d.contig_name_off[c + 1] - o;
    uint32_t h = bb_hash(d.contig_names + o, n) & d.table_mask;
    while (bb_slot_take(d.table + h, c + 1)) h = (h + 1) & d.table_mask;  // (more slots than names: a free one is met)
}
// index of the contig named [s, s + n), UINT32_MAX if there is none (names compared byte for byte)
PLO_DEV uint32_t bb_table_find(const DevBatchBuild &d, const uint8_t *s, uint32_t n) {
    uint32_t h = bb_hash(s, n) & d.table_mask;
    for (;;) {
        const uint32_t v = d.table[h];
        if (!v) return UINT32_MAX;
        const uint32_t o = d.contig_name_off[v - 1];
        if (d.contig_name_off[v] - o == n) {
            uint32_t k = 0;
            while (k < n && d.contig_names[o + k] == s[k]) ++k;
            if (k == n) return v - 1;
        }
        h = (h + 1) & d.table_mask;
    }
}

// ---- numbers (parse_uint / parse_int, bam_internal.hpp: the same unsigned arithmetic, the 2^62 cap at every digit) -------------------------
PLO_DEV bool bb_parse_uint(const uint8_t *s, const uint8_t *e, unsigned long long &v) {
    if (s == e) return false;
    v = 0;
    for (; s < e; ++s) {
        if (*s < '0' || *s > '9') return false;
        v = v * 10 + (unsigned long long)(*s - '0');
        if (v > (1ull << 62)) return false;
    }
    return true;
}
PLO_DEV bool bb_parse_int(const uint8_t *s, const uint8_t *e, long long &v) {
    bool neg = false;
    if (s < e && (*s == '-' || *s == '+')) {
        neg = *s == '-';
        ++s;
    }
    unsigned long long u;
    if (!bb_parse_uint(s, e, u)) return false;
    v = neg ? -(long long)u : (long long)u;
    return true;
}

// ---- CIGARs -----------------------------------------------------------------------------------------------------------------------------
PLO_DEV unsigned long long bb_wave_sum(unsigned long long x) { return wv::shfl(wave_scan_incl_u64(x), 63); }

// read_clip_positions (bam_internal.hpp:898-914) over the ops of a CIGAR, 64 at a time: every lane sums its own ops, finish() adds the lanes up
struct CigarSums {
    unsigned long long read = 0, clip = 0, left = 0;  // (per lane)
    uint32_t n_ops = 0;                               // (uniform)
    bool seen_other = false, aligned = false;         // (uniform) an op that is no clip / an M, = or X op was met
    // `has`: this lane holds op word c, lanes in op order
    PLO_DEV void add(bool has, uint32_t c) {
        const uint32_t t = c & 15u;
        const bool is_clip = has && (t == 4 || t == 5);
        const unsigned long long others = wv::ballot(has && !is_clip);
        const unsigned long long matches = wv::ballot(has && (t == 0 || t == 7 || t == 8));
        const unsigned long long all = wv::ballot(has);
        const int first_other = others ? __builtin_ctzll(others) : 64;
        if (has && ((0x1B3u >> t) & 1u)) read += c >> 4;  // M I S H = X
        if (is_clip) {
            clip += c >> 4;
            if (!seen_other && wv::lane() < first_other) left += c >> 4;
        }
        seen_other = seen_other || others != 0;
        aligned = aligned || matches != 0;
        n_ops += (uint32_t)__builtin_popcountll(all);
    }
    // -> size, clip start, clip end of the read (uniform)
    PLO_DEV void finish(unsigned long long &size, unsigned long long &start, unsigned long long &end) {
        size = bb_wave_sum(read);
        start = bb_wave_sum(left);
        end = size - (bb_wave_sum(clip) - start);
    }
};

// the ops at p (little-endian dwords at any alignment) summed and, with `out`, copied
PLO_DEV void bb_cigar_binary(const uint8_t *p, uint32_t n, uint32_t *out, CigarSums &cs) {
    const uint32_t lane = (uint32_t)wv::lane();
    for (uint32_t k = 0; k < n; k += 64) {
        const bool has = k + lane < n;
        const uint32_t c = has ? rec_rd32(p + 4ull * (k + lane)) : 0u;
        if (has && out) out[k + lane] = c;
        cs.add(has, c);
    }
}

PLO_DEV int bb_op_code(unsigned ch) {  // MIDNSHP=X, -1: no op letter
    switch (ch) {
        case 'M': return 0;
        case 'I': return 1;
        case 'D': return 2;
        case 'N': return 3;
        case 'S': return 4;
        case 'H': return 5;
        case 'P': return 6;
        case '=': return 7;
        case 'X': return 8;
        default: return -1;
    }
}
// parse_cigar_text (bam_internal.hpp:948-962) of [s, e), 64 bytes per step: the lane that holds an op letter parses the digits in front of
// it.  False if the text is malformed (the sums are void then); with `out` the ops are stored.
PLO_DEV bool bb_cigar_text(const uint8_t *s, const uint8_t *e, uint32_t *out, CigarSums &cs) {
    const unsigned long long n = (unsigned long long)(e - s);
    const unsigned long long lane = (unsigned long long)wv::lane();
    bool ok = true;
    for (unsigned long long k = 0; k < n; k += 64) {
        const unsigned long long i = k + lane;
        const bool in = i < n;
        const unsigned ch = in ? s[i] : (unsigned)'0';
        const int code = bb_op_code(ch);
        const bool digit = ch >= '0' && ch <= '9', is_op = in && code >= 0;
        bool bad = in && !digit && code < 0;
        uint32_t c = 0;
        if (is_op) {
            const uint8_t *d = s + i, *b = d;
            while (b > s && b[-1] >= '0' && b[-1] <= '9') --b;
            unsigned long long len = 0;
            if (b == d || !bb_parse_uint(b, d, len) || len > 0x0fffffffull) bad = true;
            c = (uint32_t)(len << 4) | (uint32_t)code;
        }
        if (in && i == n - 1 && digit) bad = true;  // digits without an op letter behind them
        const unsigned long long ops = wv::ballot(is_op);
        if (wv::ballot(bad)) ok = false;
        if (is_op && out && ok) out[cs.n_ops + (uint32_t)__builtin_popcountll(ops & ((1ull << lane) - 1ull))] = c;
        cs.add(is_op, c);
    }
    return ok;
}

// ---- the SA text --------------------------------------------------------------------------------------------------------------------------
// first `ch` in [s, e) or e (uniform)
PLO_DEV const uint8_t *bb_find(const uint8_t *s, const uint8_t *e, unsigned ch) {
    const unsigned long long n = (unsigned long long)(e - s), lane = (unsigned long long)wv::lane();
    for (unsigned long long k = 0; k < n; k += 64) {
        const unsigned long long m = wv::ballot(k + lane < n && s[k + lane] == ch);
        if (m) return s + k + (unsigned long long)__builtin_ctzll(m);
    }
    return e;
}
// the fields of segment [s, se) as split_terminator(',') yields them (sa_tag_parser.rs:26): a trailing empty field is dropped, an empty
// segment has none.  -> their number (7: more than six), f[k] / fe[k] of the first six
PLO_DEV int bb_fields(const uint8_t *s, const uint8_t *se, const uint8_t *f[6], const uint8_t *fe[6]) {
    if (s == se) return 0;
    const unsigned long long n = (unsigned long long)(se - s), lane = (unsigned long long)wv::lane();
    unsigned long long commas = 0;
    const uint8_t *cut[6];
    for (unsigned long long k = 0; k < n; k += 64) {
        unsigned long long m = wv::ballot(k + lane < n && s[k + lane] == ',');
        while (m) {
            if (commas < 6) cut[commas] = s + k + (unsigned long long)__builtin_ctzll(m);
            ++commas;
            m &= m - 1;
        }
    }
    const unsigned long long nf = commas + 1 - (se[-1] == ',' ? 1u : 0u);
    if (nf > 6) return 7;
    for (unsigned long long k = 0; k < nf; ++k) {
        f[k] = k ? cut[k - 1] + 1 : s;
        fe[k] = k < commas ? cut[k] : se;
    }
    return (int)nf;
}

// one SA segment (uniform)
struct SaSegment {
    uint32_t contig, n_ops;
    long long pos;
    bool fwd;
    unsigned long long so_start, so_end;
    const uint8_t *ctext, *ctext_end;
};
// segment [s, se) parsed and checked in the host's order (split_segments, bam_internal.hpp:1030-1067): field count, field parse, an aligned
// op, the primary's read size, the label.  -> PLO_BB_ERR_NONE or the first failure
PLO_DEV uint32_t bb_sa_segment(const DevBatchBuild &d, const uint8_t *s, const uint8_t *se, unsigned long long primary_size, uint32_t *ops_out, SaSegment &g) {
    const uint8_t *f[6], *fe[6];
    if (bb_fields(s, se, f, fe) != 6) return PLO_BB_ERR_FIELD_COUNT;
    long long pos1 = 0, nm = 0;
    unsigned long long mq = 0;
    CigarSums cs;
    const bool pos_ok = bb_parse_int(f[1], fe[1], pos1);
    const bool cig_ok = bb_cigar_text(f[3], fe[3], ops_out, cs);
    if (!pos_ok || !cig_ok || !bb_parse_uint(f[4], fe[4], mq) || mq > 255 || !bb_parse_int(f[5], fe[5], nm) || nm < -2147483648ll || nm > 2147483647ll)
        return PLO_BB_ERR_MALFORMED;
    g.pos = pos1 - 1;
    g.fwd = fe[2] - f[2] == 1 && f[2][0] == '+';
    g.n_ops = cs.n_ops;
    g.ctext = f[3];
    g.ctext_end = fe[3];
    if (!cs.aligned) return PLO_BB_ERR_UNALIGNED;
    unsigned long long sz, s0, e0;
    cs.finish(sz, s0, e0);
    if (sz != primary_size) return PLO_BB_ERR_READ_SIZE;
    g.so_start = g.fwd ? s0 : sz - e0;
    g.so_end = g.fwd ? e0 : sz - s0;
    g.contig = bb_table_find(d, f[0], (uint32_t)(fe[0] - f[0]));
    if (g.contig == UINT32_MAX) return PLO_BB_ERR_UNKNOWN_CONTIG;
    return PLO_BB_ERR_NONE;
}

// the primary's segment from the record's fixed fields and its real CIGAR (split_segments :985-997)
PLO_DEV void bb_primary(const uint8_t *p, const uint8_t *cig, uint32_t n_cig, uint32_t *ops_out, SaSegment &g, unsigned long long &size) {
    CigarSums cs;
    bb_cigar_binary(cig, n_cig, ops_out, cs);
    unsigned long long rs, re;
    cs.finish(size, rs, re);
    g.contig = rec_rd32(p);
    g.pos = (long long)(int)rec_rd32(p + 4);
    g.fwd = !(rec_rd16(p + 14) & 0x10u);
    g.n_ops = n_cig;
    g.so_start = g.fwd ? rs : size - re;
    g.so_end = g.fwd ? re : size - rs;
    g.ctext = g.ctext_end = nullptr;
}

// real_cigar (:966-979), shared with depth_core.hpp.  The in-record CIGAR (n_cig ops at cig, inside the record) is the placeholder
// <l_seq>S<n>N that bam_write1 leaves behind more than 65 535 ops
PLO_DEV bool bb_cigar_is_placeholder(const uint8_t *cig, uint32_t n_cig, uint32_t lseq) {
    if (n_cig != 2) return false;
    const unsigned c0 = rec_rd32(cig), c1 = rec_rd32(cig + 4);
    return (c0 & 15u) == 4 && (c0 >> 4) == lseq && (c1 & 15u) == 3;
}
// cig / n_cig: the in-record CIGAR on entry, the record's real CIGAR on return -- the ops of the field cg (the record's first CG field,
// complete inside the record, or NULL) when that is a B,I array and the in-record CIGAR is the placeholder
PLO_DEV void bb_real_cigar(const uint8_t *cg, uint32_t lseq, const uint8_t *&cig, uint32_t &n_cig) {
    if (cg && cg[2] == 'B' && cg[3] == 'I' && bb_cigar_is_placeholder(cig, n_cig, lseq)) {
        n_cig = rec_rd32(cg + 4);
        cig = cg + 8;
    }
}

// ---- plan -------------------------------------------------------------------------------------------------------------------------------
PLO_DEV void batch_plan_read(const DevBatchBuild &d, uint32_t r) {
    const bool lane0 = wv::lane() == 0;
    const uint32_t nr = d.n_reads;
    uint32_t *pl = d.plan + (size_t)r * BB_PLAN_WORDS;
    // the bounds of the source record, as records_plan_read checks them
    int berr = -1;
    const unsigned long long off = d.read_rec_off[r];
    const uint8_t *p = nullptr;
    uint32_t bs = 0, lq = 0, ncg = 0, lseq = 0;
    unsigned long long aux_off = 0;
    if (off > d.records_bytes || d.records_bytes - off < 4) {
        berr = REC_ERR_OFFSET;
    } else {
        bs = rec_rd32(d.records + off);
        if (bs < 32 || bs > d.records_bytes - off - 4) {
            berr = REC_ERR_BLOCK;
        } else {
            p = d.records + off + 4;
            lq = p[8];
            ncg = rec_rd16(p + 12);
            lseq = rec_rd32(p + 16);
            aux_off = 32ull + lq + 4ull * ncg + ((unsigned long long)lseq + 1) / 2 + lseq;
            if (aux_off > bs) berr = REC_ERR_LAYOUT;
        }
    }
    if (berr >= 0) {  // (uniform)
        if (lane0) {
            wv::atomic_add(d.err + 1 + berr, 1);
            d.size[r] = 0;
            d.size[(size_t)nr + r] = 0;
            d.err_kind[r] = PLO_BB_ERR_NONE;
        }
        return;
    }
    // aux_find for CG and for SA (bam_internal.hpp:873-884): the first field of either tag, nothing behind the first malformed field
    const uint8_t *e = p + bs, *a = p + aux_off, *cg = nullptr, *sa = nullptr;
    unsigned long long sa_len = 0;
    while (a < e && !(cg && sa)) {
        const unsigned long long n = aux_field_len_wave(a, e);
        if (!n) break;
        if (!cg && a[0] == 'C' && a[1] == 'G') cg = a;
        if (!sa && a[0] == 'S' && a[1] == 'A') {
            sa = a;
            sa_len = n;
        }
        a += n;
    }
    const uint8_t *cig = p + 32 + lq;
    uint32_t n_cig = ncg;
    bb_real_cigar(cg, lseq, cig, n_cig);
    SaSegment g;
    unsigned long long size = 0, n_ops = n_cig;
    bb_primary(p, cig, n_cig, nullptr, g, size);
    bool empty = g.so_start >= g.so_end;
    uint32_t kind = PLO_BB_ERR_NONE, n_seg = 1;
    if (sa && sa[2] != 'Z') {
        kind = PLO_BB_ERR_SA_NOT_Z;
        sa = nullptr;
    }
    if (sa) {
        const uint8_t *s = sa + 3, *te = sa + sa_len - 1;
        while (s < te) {  // split_terminator(';') (sa_tag_parser.rs:55-59)
            const uint8_t *se = bb_find(s, te, ';');
            kind = bb_sa_segment(d, s, se, size, nullptr, g);
            if (kind != PLO_BB_ERR_NONE) break;
            empty = empty || g.so_start >= g.so_end;
            n_ops += g.n_ops;
            ++n_seg;
            s = se < te ? se + 1 : te;
        }
    }
    if (kind == PLO_BB_ERR_NONE && empty) kind = PLO_BB_ERR_EMPTY_SEGMENT;  // (:146-152: behind every segment's own checks)
    if (lane0) {
        if (kind != PLO_BB_ERR_NONE) wv::atomic_min(d.err, (int)r);
        d.err_kind[r] = kind;
        d.size[r] = n_seg;
        d.size[(size_t)nr + r] = n_ops;
        pl[BP_NCIG] = n_cig;
        pl[BP_CIG_OFF] = (uint32_t)(cig - p);
        pl[BP_SA_OFF] = sa ? (uint32_t)(sa + 3 - p) : 0u;
        pl[BP_SA_LEN] = sa ? (uint32_t)(sa_len - 4) : 0u;
    }
}

// ---- emit (a batch without failures only) -------------------------------------------------------------------------------------------------
// hand-off through GLOBAL scratch between the lanes of the wave: the stores have left the wave (device scope) before any lane reads them
PLO_DEV void bb_sync_global() {
#ifdef PLO_EMULATOR
    wv::sync();
#else
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    __builtin_amdgcn_s_waitcnt(0);
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#endif
}
PLO_DEV void bb_store_segment(const DevBatchBuild &d, unsigned long long at, const SaSegment &g, uint32_t ctext_off) {
    d.t_key[at] = g.so_start;
    d.t_nops[at] = g.n_ops;
    d.t_ctext[at] = ctext_off;
    d.t_clen[at] = (uint32_t)(g.ctext_end - g.ctext);
    d.t_contig[at] = g.contig;
    d.t_pos[at] = g.pos;
    d.t_fwd[at] = g.fwd ? 1 : 0;
}

PLO_DEV void batch_emit_read(const DevBatchBuild &d, uint32_t r) {
    const uint32_t lane = (uint32_t)wv::lane(), nr = d.n_reads;
    const bool lane0 = lane == 0;
    const uint32_t *pl = d.plan + (size_t)r * BB_PLAN_WORDS;
    const unsigned long long off = d.read_rec_off[r];
    const uint8_t *p = d.records + off + 4;
    const uint32_t lq = p[8], ncg = rec_rd16(p + 12), lseq = rec_rd32(p + 16), flag = rec_rd16(p + 14);
    const unsigned long long S0 = d.start[r], O0 = d.start[(size_t)nr + 1 + r];
    const uint32_t ns = (uint32_t)(d.start[r + 1] - S0);
    if (lane0) {
        const unsigned long long seq_off = off + 4 + 32 + lq + 4ull * ncg;
        d.read_is_reverse[r] = (flag & 0x10u) ? 1 : 0;
        d.read_seq_len[r] = lseq;
        d.read_seq_off[r] = seq_off;
        d.read_flags[r] = (uint16_t)flag;
        d.read_qual_off[r] = seq_off + ((unsigned long long)lseq + 1) / 2;
        if (r + 1 == nr) d.seg_cigar_off[d.start[nr]] = (uint32_t)d.start[(size_t)nr + 1 + nr];
    }
    // 1. the segments in text order
    SaSegment g;
    unsigned long long size = 0;
    const uint8_t *cig = p + pl[BP_CIG_OFF];
    bb_primary(p, cig, pl[BP_NCIG], nullptr, g, size);
    if (lane0) bb_store_segment(d, S0, g, 0);
    if (pl[BP_SA_OFF]) {
        const uint8_t *s = p + pl[BP_SA_OFF], *te = s + pl[BP_SA_LEN];
        unsigned long long at = S0 + 1;
        while (s < te) {
            const uint8_t *se = bb_find(s, te, ';');
            (void)bb_sa_segment(d, s, se, size, nullptr, g);
            if (lane0) bb_store_segment(d, at, g, (uint32_t)(g.ctext - p));
            ++at;
            s = se < te ? se + 1 : te;
        }
    }
    bb_sync_global();
    // 2. std::stable_sort by so_start (:1073) as a rank count: rank(i) = #{j : key_j < key_i or (key_j == key_i and j < i)}; the ops of the
    // segments in front of i are counted in the same walk
    for (uint32_t i = lane; i < ns; i += 64) {
        const unsigned long long key = d.t_key[S0 + i];
        uint32_t rank = 0;
        unsigned long long before = 0;
        for (uint32_t j = 0; j < ns; ++j) {
            const unsigned long long kj = d.t_key[S0 + j];
            if (kj < key || (kj == key && j < i)) {
                ++rank;
                before += d.t_nops[S0 + j];
            }
        }
        const unsigned long long to = S0 + rank;
        d.seg_read[to] = r;
        d.seg_contig[to] = d.t_contig[S0 + i];
        d.seg_pos[to] = d.t_pos[S0 + i];
        d.seg_fwd[to] = d.t_fwd[S0 + i];
        d.seg_cigar_off[to] = (uint32_t)(O0 + before);
        d.t_dst[S0 + i] = (uint32_t)(O0 + before);
    }
    bb_sync_global();
    // 3. the ops
    {
        CigarSums cs;
        bb_cigar_binary(cig, pl[BP_NCIG], d.cigar + d.t_dst[S0], cs);
    }
    for (uint32_t i = 1; i < ns; ++i) {
        CigarSums cs;
        const uint8_t *ct = p + d.t_ctext[S0 + i];
        (void)bb_cigar_text(ct, ct + d.t_clen[S0 + i], d.cigar + d.t_dst[S0 + i], cs);
    }
}

}  // namespace plo
