// records_core.hpp -- output BAM records assembled on the device: the bytes of records_build (bam_host.cpp), i.e. of
// get_liftover_alignment_for_read_and_contig_segment (src/read_alignment_scanner.rs:245-284: clone_record :105-118, PS / ZM
// :254-268, pos / cigar / flags / bin :270-282) and finish_remapped_alignment_set (:310-366: unmapped copy :317-335, SA :348-364), serialised
// as htslib's bam_write1 does (CG:B,I beyond 65535 CIGAR ops).  Everything but the layout is already on the device: the lift result
// (DevWork), the finishing (flags, bin, reference end, reversed bases and qualities: finish_core.hpp) and the SA segments.
//   plan  (a wave per read):  bounds of the source record, the aux walk of aux_field_len / aux_find / plan_aux / has_cg_cigar
//                             (bam_internal.hpp, bam_host.cpp) -> at most six cuts sorted by offset, the kept length, the read's bytes
//   scan  (waves):            exclusive 64-bit scan of the reads' bytes and record counts
//   emit  (a workgroup per read): every byte of the read's records, the bulk as aligned 16-byte stores
// With DevRecords::item_nm (nm_core.hpp) every lifted record gets NM:i behind ZM:C.  With DevRecords::item_md_off / md_text (md_core.hpp) it
// gets MD:Z behind that (calmd appends NM, then MD), and the first field tagged MD of the source record, whatever its type, is cut from the
// lifted records (the sixth cut; an unmapped copy keeps it).  With DevRecords::item_eqx_off / eqx_ops (eqx_core.hpp) the CIGAR of every
// lifted record -- n_cigar_op, the ops in the record or in CG:B,I, the 65535 rule -- is that result's in place of the lift's.  Those are the
// three differences to the host builder.
// The same functions run under the CPU emulator (tests/emu/emu_records.cpp).
#pragma once
#include <plo_wave.hpp>
#include <stdint.h>

#include "finish_core.hpp"
#include "lift_types.hpp"

namespace plo {

// per-read plan: REC_PLAN_WORDS dwords
enum { RP_NCUT = 0, RP_KEPT = 1, RP_CUT_OFF = 2, RP_CUT_LEN = 8, RP_AUX_OFF = 14, RP_BLOCK = 15, REC_PLAN_WORDS = 16, REC_MAX_CUTS = 6 };
// d.err[k]: number of reads that failed check k
enum { REC_ERR_OFFSET = 0,  // read_rec_off points outside `records`
       REC_ERR_BLOCK = 1,   // block_size runs past the end of `records` (or is below the 32 fixed bytes)
       REC_ERR_LAYOUT = 2,  // l_qname / n_cigar / l_seq point outside the record
       REC_ERR_SEQLEN = 3,  // l_seq differs from the batch's read_seq_len (the reversed bases were made for that length)
       REC_ERR_N = 4 };

struct DevRecords {
    // input (plo_records_in)
    const uint8_t *records;
    unsigned long long records_bytes;
    const uint64_t *read_rec_off;
    const uint32_t *contig_name_off;  // (trusted like plo_sa_in's table: made by the caller from the BAM header, not from the stream)
    const uint8_t *contig_names;
    int is_target_region;
    // the context's finishing and SA results
    const uint16_t *item_flag, *item_bin;
    const int64_t *item_ref_end;
    const uint64_t *item_seq_off, *item_qual_off;
    const uint32_t *item_read;
    const uint32_t *read_n_lifted;
    const uint16_t *read_unmapped_flag;
    const uint64_t *read_seq_off, *read_qual_off;
    const uint8_t *rev_seq, *rev_qual;
    const uint32_t *sa_off;
    const uint8_t *sa_text;
    const uint32_t *item_nm;  // the context's plo_nm_dev result: NM:i behind ZM:C of every lifted record; NULL: no NM, the host builder's bytes
    const uint64_t *item_md_off;  // the context's plo_md_dev result: MD:Z behind ZM:C / NM:i of every lifted record, the source's first MD cut; NULL: neither
    const uint8_t *md_text;
    const uint64_t *item_eqx_off;  // the context's plo_eqx_dev result (eqx_core.hpp): the CIGAR of every lifted record with = / X for M, in ops; NULL: wk.out_cigar
    const uint32_t *eqx_ops;
    // the index: strand of the contig segments (PS suffix)
    const uint8_t *cs_is_fwd;
    const uint32_t *contig_seg_off;
    // workspace and output
    uint32_t *plan;            // [n_reads][REC_PLAN_WORDS]
    unsigned long long *size;  // [3][n_reads]: bytes, records, unmapped copies (0 / 1) of every read
    const unsigned long long *start;  // [3][n_reads + 1]: their exclusive scans
    uint64_t *record_off;      // [n_records + 1]
    uint8_t *out;
    unsigned *err;             // [REC_ERR_N]
};

PLO_DEV unsigned rec_rd16(const uint8_t *p) { return (unsigned)p[0] | ((unsigned)p[1] << 8); }
PLO_DEV unsigned rec_rd32(const uint8_t *p) { return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16) | ((unsigned)p[3] << 24); }
PLO_DEV void rec_wr16(uint8_t *p, unsigned v) {
    p[0] = (uint8_t)v;
    p[1] = (uint8_t)(v >> 8);
}
PLO_DEV void rec_wr32(uint8_t *p, unsigned v) {
    p[0] = (uint8_t)v;
    p[1] = (uint8_t)(v >> 8);
    p[2] = (uint8_t)(v >> 16);
    p[3] = (uint8_t)(v >> 24);
}

// aux_field_len (bam_internal.hpp:842-871) by the 64 lanes of a wave, every lane with the same arguments: length of the field at a,
// 0 if malformed or running past e.  A B array is skipped by its count; the NUL of a Z / H string is found 64 bytes per step.
PLO_DEV unsigned long long aux_field_len_wave(const uint8_t *a, const uint8_t *e) {
    const unsigned long long room = (unsigned long long)(e - a);
    if (room < 3) return 0;
    const unsigned t = a[2];
    unsigned long long n = 0;
    if (t == 'A' || t == 'c' || t == 'C') n = 1;
    else if (t == 's' || t == 'S') n = 2;
    else if (t == 'i' || t == 'I' || t == 'f') n = 4;
    else if (t == 'd') n = 8;
    else if (t == 'Z' || t == 'H') {
        const unsigned long long avail = room - 3;
        const unsigned long long lane = (unsigned long long)wv::lane();
        for (unsigned long long k = 0; k < avail && !n; k += 64) {
            const unsigned long long idx = k + lane;
            const bool z = idx < avail && a[3 + idx] == 0;
            const unsigned long long m = wv::ballot(z);
            if (m) n = k + (unsigned long long)__builtin_ctzll(m) + 1;
        }
        if (!n) return 0;
    } else if (t == 'B') {
        if (room < 8) return 0;
        const unsigned st = a[3];
        unsigned long long es;
        if (st == 'c' || st == 'C') es = 1;
        else if (st == 's' || st == 'S') es = 2;
        else if (st == 'i' || st == 'I' || st == 'f') es = 4;
        else return 0;
        n = 5 + es * (unsigned long long)rec_rd32(a + 4);
    } else {
        return 0;
    }
    return 3 + n <= room ? 3 + n : 0;
}

// the CIGAR item i's record carries: the lift's, or the = / X one of plo_eqx_dev while the context holds it.  bam_write1's 65535 rule goes by this count
PLO_DEV uint32_t rec_n_cigar(const DevWork &wk, const DevRecords &d, uint32_t i) {
    return d.item_eqx_off ? (uint32_t)(d.item_eqx_off[i + 1] - d.item_eqx_off[i]) : wk.cig_len[i];
}
PLO_DEV const uint32_t *rec_cigar(const DevWork &wk, const DevRecords &d, uint32_t i) {
    return d.item_eqx_off ? d.eqx_ops + d.item_eqx_off[i] : wk.out_cigar + wk.cig_off[i];
}

// bytes of a lifted record without its SA tag (records_build's lifted_size): `base` = 4 + 32 + l_qname + bases + qualities + kept aux
PLO_DEV unsigned long long rec_lifted_size(const DevBatch &bt, const DevWork &wk, const DevRecords &d, uint32_t i, unsigned long long base) {
    const uint32_t nc = rec_n_cigar(wk, d, i);
    const uint32_t contig = bt.seg_contig[wk.item_seg[i]];
    unsigned long long sz = base + (nc <= 0xffffu ? 4ull * nc : 8ull + 8ull + 4ull * nc);  // bam_write1: placeholder + CG:B,I
    sz += 3ull + (d.contig_name_off[contig + 1] - d.contig_name_off[contig]) + 6u + dec_digits(wk.item_cseg[i]) + 1u + 1u;  // PS:Z{contig}_split{n}{+|-}\0
    sz += 4 + (d.item_nm ? 7u : 0u);  // ZM:C, NM:i
    return d.item_md_off ? sz + 3ull + (d.item_md_off[i + 1] - d.item_md_off[i]) + 1 : sz;  // MD:Z{text}\0
}

// plan + size of read r by one wave (every lane computes the same values; lane 0 stores them)
PLO_DEV void records_plan_read(const DevBatch &bt, const DevWork &wk, const DevRecords &d, uint32_t r) {
    uint32_t *pl = d.plan + (size_t)r * REC_PLAN_WORDS;
    const bool lane0 = wv::lane() == 0;
    const uint32_t nr = bt.n_reads;
    int err = -1;
    const unsigned long long off = d.read_rec_off[r];
    const uint8_t *p = nullptr;
    uint32_t bs = 0, lq = 0, ncg = 0, lseq = 0;
    unsigned long long aux_off = 0;
    if (off > d.records_bytes || d.records_bytes - off < 4) {
        err = REC_ERR_OFFSET;
    } else {
        bs = rec_rd32(d.records + off);
        if (bs < 32 || bs > d.records_bytes - off - 4) {
            err = REC_ERR_BLOCK;
        } else {
            p = d.records + off + 4;
            lq = p[8];
            ncg = rec_rd16(p + 12);
            lseq = rec_rd32(p + 16);
            aux_off = 32ull + lq + 4ull * ncg + ((unsigned long long)lseq + 1) / 2 + lseq;
            if (aux_off > bs) err = REC_ERR_LAYOUT;
            else if (lseq != bt.read_seq_len[r]) err = REC_ERR_SEQLEN;
        }
    }
    if (err >= 0) {  // (wave-uniform)
        if (lane0) {
            wv::atomic_add_global(d.err + err, 1u);
            pl[RP_NCUT] = 0;
            d.size[r] = 0;
            d.size[nr + r] = 0;
            d.size[2 * (size_t)nr + r] = 0;
        }
        return;
    }
    // the walk of plan_aux (bam_host.cpp:736-767): the first NM, SA, PS, ZM are cut, the first CG when it is a B,I array and the stored
    // CIGAR is the <l_seq>S<n>N placeholder (has_cg_cigar :725-735); nothing behind the first malformed field is looked at.  With an MD
    // result the first MD of a read with lifted records is cut too (the unmapped copy of a read without keeps its aux bytes)
    const uint32_t nl = d.read_n_lifted[r];
    const bool cut_md = d.item_md_off != nullptr && nl > 0;
    const uint8_t *e = p + bs;
    const uint8_t *a = p + aux_off;
    unsigned seen = 0;
    uint32_t n_cut = 0, cut_total = 0, cg_slot = 0, cg_off = 0, cg_len = 0;
    while (a < e) {
        const unsigned long long n = aux_field_len_wave(a, e);
        if (!n) break;
        const unsigned t0 = a[0], t1 = a[1];
        const int k = (t0 == 'N' && t1 == 'M') ? 0 : (t0 == 'S' && t1 == 'A') ? 1 : (t0 == 'P' && t1 == 'S') ? 2 : (t0 == 'Z' && t1 == 'M') ? 3 : (t0 == 'C' && t1 == 'G') ? 4 : (cut_md && t0 == 'M' && t1 == 'D') ? 5 : -1;
        if (k >= 0 && !((seen >> k) & 1u)) {
            seen |= 1u << k;
            if (k != 4) {
                if (lane0) {
                    pl[RP_CUT_OFF + n_cut] = (uint32_t)(a - p);
                    pl[RP_CUT_LEN + n_cut] = (uint32_t)n;
                }
                ++n_cut;
                cut_total += (uint32_t)n;
            } else if (a[2] == 'B' && a[3] == 'I') {
                cg_slot = n_cut;
                cg_off = (uint32_t)(a - p);
                cg_len = (uint32_t)n;
            }
        }
        a += n;
    }
    if (cg_len) {
        bool placeholder = false;
        if (ncg == 2) {
            const unsigned c0 = rec_rd32(p + 32 + lq), c1 = rec_rd32(p + 32 + lq + 4);
            placeholder = (c0 & 15u) == 4 && (c0 >> 4) == lseq && (c1 & 15u) == 3;
        }
        if (placeholder) {
            if (lane0) {
                for (uint32_t j = n_cut; j > cg_slot; --j) {
                    pl[RP_CUT_OFF + j] = pl[RP_CUT_OFF + j - 1];
                    pl[RP_CUT_LEN + j] = pl[RP_CUT_LEN + j - 1];
                }
                pl[RP_CUT_OFF + cg_slot] = cg_off;
                pl[RP_CUT_LEN + cg_slot] = cg_len;
            }
            ++n_cut;
            cut_total += cg_len;
        }
    }
    const uint32_t kept = (uint32_t)(bs - aux_off) - cut_total;
    // sizes (records_build pass 1)
    const unsigned long long base = 4ull + 32 + lq + ((unsigned long long)lseq + 1) / 2 + lseq + kept;
    unsigned long long bytes = 0, nrec = 0;
    if (nl == 0) {
        if (!d.is_target_region) {  // unmapped copy :321-334
            bytes = base;
            nrec = 1;
        }
    } else {
        const uint32_t i0 = u32_lower_bound(d.item_read, wk.n_items, r), i1 = u32_lower_bound(d.item_read, wk.n_items, r + 1);
        unsigned long long sa_total = 0;
        for (uint32_t i = i0; i < i1; ++i)
            if (wk.status[i] == PLO_ITEM_LIFTED) sa_total += d.sa_off[i + 1] - d.sa_off[i];
        for (uint32_t i = i0; i < i1; ++i) {
            if (wk.status[i] != PLO_ITEM_LIFTED) continue;
            bytes += rec_lifted_size(bt, wk, d, i, base);
            if (nl > 1) bytes += 3ull + (sa_total - (d.sa_off[i + 1] - d.sa_off[i])) + 1;  // SA:Z of the other records (:352-364)
        }
        nrec = nl;
    }
    if (lane0) {
        pl[RP_NCUT] = n_cut;
        pl[RP_KEPT] = kept;
        pl[RP_AUX_OFF] = (uint32_t)aux_off;
        pl[RP_BLOCK] = bs;
        d.size[r] = bytes;
        d.size[nr + r] = nrec;
        d.size[2 * (size_t)nr + r] = nl == 0 ? nrec : 0;
    }
}

// ---- exclusive 64-bit scan (a 60 k-read window is ~1.4 GB of records, four of them pass 2^32): waves of 64 lanes x 8 values --------------
constexpr uint32_t REC_SCAN_CHUNK = 512;
PLO_DEV unsigned long long wave_scan_incl_u64(unsigned long long x) {
    const int l = wv::lane();
    for (int s = 1; s < 64; s <<= 1) {
        const unsigned long long t = wv::shfl(x, (l - s) & 63);
        if (l >= s) x += t;
    }
    return x;
}
// sum of chunk w -> partial[w]
PLO_DEV void rec_scan_sums(const unsigned long long *in, uint32_t n, uint32_t w, unsigned long long *partial) {
    const unsigned long long base = (unsigned long long)w * REC_SCAN_CHUNK + (unsigned long long)wv::lane() * 8;
    unsigned long long s = 0;
    for (int k = 0; k < 8; ++k)
        if (base + k < n) s += in[base + k];
    s = wave_scan_incl_u64(s);
    if (wv::lane() == 63) partial[w] = s;
}
// one wave: partial[] -> its exclusive scan, *total = the sum
PLO_DEV void rec_scan_partials(unsigned long long *partial, uint32_t nb, unsigned long long *total) {
    unsigned long long carry = 0;
    for (uint32_t b0 = 0; b0 < nb; b0 += 64) {
        const uint32_t i = b0 + (uint32_t)wv::lane();
        const unsigned long long v = i < nb ? partial[i] : 0;
        const unsigned long long inc = wave_scan_incl_u64(v);
        if (i < nb) partial[i] = carry + inc - v;
        carry += wv::shfl(inc, 63);
    }
    if (wv::lane() == 0) *total = carry;
}
// chunk w of out[] = exclusive scan of in[] (out[n] is written by rec_scan_partials)
PLO_DEV void rec_scan_apply(const unsigned long long *in, uint32_t n, uint32_t w, const unsigned long long *partial, unsigned long long *out) {
    const unsigned long long base = (unsigned long long)w * REC_SCAN_CHUNK + (unsigned long long)wv::lane() * 8;
    unsigned long long v[8], s = 0;
    for (int k = 0; k < 8; ++k) {
        v[k] = base + k < n ? in[base + k] : 0;
        s += v[k];
    }
    unsigned long long run = partial[w] + wave_scan_incl_u64(s) - s;
    for (int k = 0; k < 8; ++k) {
        if (base + k < n) out[base + k] = run;
        run += v[k];
    }
}

// ---- emit ------------------------------------------------------------------------------------------------------------------------------
PLO_DEV void copy_bytes(uint8_t *dst, const uint8_t *src, unsigned long long lo, unsigned long long hi, int tid, int nt) {
    for (unsigned long long i = lo + (unsigned long long)tid; i < hi; i += (unsigned long long)nt) dst[i] = src[i];
}
// dst[0, len) = src[0, len) by nt cooperating threads, source and destination at any byte alignment.  VEC: the destination's aligned
// 16-byte chunks are stored whole, their source bytes read as aligned dwords and realigned by funnel shifts; the head, the tail and the
// chunks whose dwords would reach outside [src, src + len) go bytewise -- nothing outside the span is read.
template <bool VEC>
PLO_DEV void copy_span(uint8_t *dst, const uint8_t *src, unsigned long long len, int tid, int nt) {
    if (!VEC) {
        copy_bytes(dst, src, 0, len, tid, nt);
        return;
    }
    unsigned long long head = (16u - (unsigned)((uintptr_t)dst & 15u)) & 15u;
    if (head > len) head = len;
    const unsigned long long nch = (len - head) >> 4;
    const uint8_t *s0 = src + head;
    const unsigned sh = (unsigned)((uintptr_t)s0 & 3u);
    // chunk c reads the dwords [s0 + 16 c - sh, + 16 (sh == 0) or + 20)
    unsigned long long c_lo = head >= sh ? 0 : 1, c_hi = nch;
    if (sh && nch && len - head - 16 * nch < 4 - sh) c_hi = nch - 1;
    if (c_lo > c_hi) c_lo = c_hi;
    copy_bytes(dst, src, 0, head + 16 * c_lo, tid, nt);
    copy_bytes(dst, src, head + 16 * c_hi, len, tid, nt);
    uint8_t *d0 = dst + head;
    // four chunks per thread per trip, the loads of all four before the first store
    for (unsigned long long cb = c_lo + (unsigned long long)tid; cb < c_hi; cb += 4ull * (unsigned long long)nt) {
        unsigned w[4][5];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned long long c = cb + (unsigned long long)u * (unsigned long long)nt;
            const uint32_t *q = (const uint32_t *)(s0 + 16 * (c < c_hi ? c : cb) - sh);
            w[u][0] = q[0];
            w[u][1] = q[1];
            w[u][2] = q[2];
            w[u][3] = q[3];
            w[u][4] = sh ? q[4] : 0u;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const unsigned long long c = cb + (unsigned long long)u * (unsigned long long)nt;
            if (c >= c_hi) break;
            U4 o;
            o.x = (unsigned)((((unsigned long long)w[u][1] << 32) | w[u][0]) >> (8 * sh));
            o.y = (unsigned)((((unsigned long long)w[u][2] << 32) | w[u][1]) >> (8 * sh));
            o.z = (unsigned)((((unsigned long long)w[u][3] << 32) | w[u][2]) >> (8 * sh));
            o.w = (unsigned)((((unsigned long long)w[u][4] << 32) | w[u][3]) >> (8 * sh));
            *(U4 *)(d0 + 16 * c) = o;
        }
    }
}

// the kept aux bytes of the source record (copy_aux, bam_host.cpp:768-777); returns their end
template <bool VEC>
PLO_DEV uint8_t *rec_copy_aux(uint8_t *q, const uint8_t *p, const uint32_t *pl, int tid, int nt) {
    uint32_t cur = pl[RP_AUX_OFF];
    const uint32_t n_cut = pl[RP_NCUT];
    for (uint32_t j = 0; j < n_cut; ++j) {
        const uint32_t co = pl[RP_CUT_OFF + j];
        copy_span<VEC>(q, p + cur, co - cur, tid, nt);
        q += co - cur;
        cur = co + pl[RP_CUT_LEN + j];
    }
    copy_span<VEC>(q, p + cur, pl[RP_BLOCK] - cur, tid, nt);
    return q + (pl[RP_BLOCK] - cur);
}

// every byte of the records of read r (records_build pass 2) by nt cooperating threads; thread 0 also stores their record_off
template <bool VEC>
PLO_DEV void records_emit_read(const DevBatch &bt, const DevWork &wk, const DevRecords &d, uint32_t r, int tid, int nt) {
    const uint32_t nr = bt.n_reads;
    const unsigned long long at = d.start[r];
    unsigned long long k = d.start[(size_t)nr + 1 + r];
    if (d.start[(size_t)nr + 2 + r] == k) return;  // no record (is_target_region, nothing lifted)
    const uint32_t *pl = d.plan + (size_t)r * REC_PLAN_WORDS;
    const uint8_t *p = d.records + d.read_rec_off[r] + 4;
    const uint32_t lq = p[8], lseq = rec_rd32(p + 16), seqb = (lseq + 1) / 2, ncg = rec_rd16(p + 12);
    const uint8_t *src_seq = p + 32 + lq + 4ull * ncg;
    const unsigned long long base = 4ull + 32 + lq + seqb + lseq + pl[RP_KEPT];
    uint8_t *o = d.out + at;
    const uint32_t nl = d.read_n_lifted[r];
    if (nl == 0) {  // unmapped copy :321-334
        uint8_t *b = o + 4;
        if (tid == 0) {
            d.record_off[k] = at;
            rec_wr32(o, (unsigned)(base - 4));
            rec_wr32(b, 0xffffffffu);
            rec_wr32(b + 4, 0xffffffffu);
            b[8] = (uint8_t)lq;
            b[9] = 255;
            rec_wr16(b + 10, rec_rd16(p + 10));
            rec_wr16(b + 12, 0);
            rec_wr16(b + 14, d.read_unmapped_flag[r]);
            rec_wr32(b + 16, lseq);
            for (int j = 20; j < 32; ++j) b[j] = p[j];  // mate reference, mate position, template length: untouched
        }
        uint8_t *q = b + 32;
        copy_span<VEC>(q, p + 32, lq, tid, nt);
        q += lq;
        if (d.read_seq_off[r] != PLO_NO_FLIP) {
            copy_span<VEC>(q, d.rev_seq + d.read_seq_off[r], seqb, tid, nt);
            copy_span<VEC>(q + seqb, d.rev_qual + d.read_qual_off[r], lseq, tid, nt);
        } else {
            copy_span<VEC>(q, src_seq, (unsigned long long)seqb + lseq, tid, nt);
        }
        q += (unsigned long long)seqb + lseq;
        rec_copy_aux<VEC>(q, p, pl, tid, nt);
        return;
    }
    const uint32_t i0 = u32_lower_bound(d.item_read, wk.n_items, r), i1 = u32_lower_bound(d.item_read, wk.n_items, r + 1);
    unsigned long long sa_total = 0;
    for (uint32_t i = i0; i < i1; ++i)
        if (wk.status[i] == PLO_ITEM_LIFTED) sa_total += d.sa_off[i + 1] - d.sa_off[i];
    for (uint32_t i = i0; i < i1; ++i) {
        if (wk.status[i] != PLO_ITEM_LIFTED) continue;
        const uint32_t nc = rec_n_cigar(wk, d, i);
        const uint32_t *cg = rec_cigar(wk, d, i);
        const long long pos = wk.pos[i];
        unsigned long long size = rec_lifted_size(bt, wk, d, i, base);
        if (nl > 1) size += 3ull + (sa_total - (d.sa_off[i + 1] - d.sa_off[i])) + 1;
        uint8_t *b = o + 4;
        if (tid == 0) {
            d.record_off[k] = (uint64_t)(o - d.out);
            rec_wr32(o, (unsigned)(size - 4));
            rec_wr32(b, wk.chrom[i]);
            rec_wr32(b + 4, (unsigned)(int)pos);
            b[8] = (uint8_t)lq;
            b[9] = wk.mapq[i];
            rec_wr16(b + 10, d.item_bin[i]);  // :278-279
            rec_wr16(b + 12, nc <= 0xffffu ? nc : 2u);
            rec_wr16(b + 14, d.item_flag[i]);
            rec_wr32(b + 16, lseq);
            for (int j = 20; j < 32; ++j) b[j] = p[j];
        }
        uint8_t *q = b + 32;
        copy_span<VEC>(q, p + 32, lq, tid, nt);
        q += lq;
        if (nc <= 0xffffu) {
            copy_span<VEC>(q, (const uint8_t *)cg, 4ull * nc, tid, nt);
            q += 4ull * nc;
        } else {  // bam_write1: <l_seq>S<ref_len>N, the real CIGAR goes into CG:B,I behind the other tags
            if (tid == 0) {
                rec_wr32(q, (lseq << 4) | 4u);
                rec_wr32(q + 4, ((unsigned)(d.item_ref_end[i] - pos) << 4) | 3u);
            }
            q += 8;
        }
        if (d.item_seq_off[i] != PLO_NO_FLIP) {  // reverse_alignment_seq_and_qual :125-133, made by k_revcomp
            copy_span<VEC>(q, d.rev_seq + d.item_seq_off[i], seqb, tid, nt);
            copy_span<VEC>(q + seqb, d.rev_qual + d.item_qual_off[i], lseq, tid, nt);
        } else {
            copy_span<VEC>(q, src_seq, (unsigned long long)seqb + lseq, tid, nt);
        }
        q += (unsigned long long)seqb + lseq;
        q = rec_copy_aux<VEC>(q, p, pl, tid, nt);
        // PS:Z "{contig}_split{cseg}{+|-}" (:254-265), ZM:C original MAPQ (:266-268)
        const uint32_t contig = bt.seg_contig[wk.item_seg[i]], cseg = wk.item_cseg[i];
        const uint32_t cn0 = d.contig_name_off[contig], cnl = d.contig_name_off[contig + 1] - cn0;
        copy_span<VEC>(q + 3, d.contig_names + cn0, cnl, tid, nt);
        const uint32_t dg = dec_digits(cseg);
        if (tid == nt - 1) {
            q[0] = 'P';
            q[1] = 'S';
            q[2] = 'Z';
            uint8_t *t = q + 3 + cnl;
            const char split[6] = {'_', 's', 'p', 'l', 'i', 't'};
            for (int j = 0; j < 6; ++j) t[j] = (uint8_t)split[j];
            t = put_dec(t + 6, cseg);
            t[0] = d.cs_is_fwd[d.contig_seg_off[contig] + cseg] ? '+' : '-';
            t[1] = 0;
            t[2] = 'Z';
            t[3] = 'M';
            t[4] = 'C';
            t[5] = p[9];
            if (d.item_nm) {  // NM:i, always type i: the form samtools calmd appends
                t[6] = 'N';
                t[7] = 'M';
                t[8] = 'i';
                rec_wr32(t + 9, d.item_nm[i]);
            }
        }
        q += 3ull + cnl + 6 + dg + 2 + 4 + (d.item_nm ? 7u : 0u);
        if (d.item_md_off) {  // MD:Z behind NM:i, the order calmd appends them in
            const unsigned long long ml = d.item_md_off[i + 1] - d.item_md_off[i];
            if (tid == 0) {
                q[0] = 'M';
                q[1] = 'D';
                q[2] = 'Z';
                q[3 + ml] = 0;
            }
            copy_bytes(q + 3, d.md_text + d.item_md_off[i], 0, ml, tid, nt);  // (a short text: bytewise, and no further instance of the 16-byte copy in the kernel)
            q += 3ull + ml + 1;
        }
        if (nl > 1) {  // SA:Z: the segments of the read's other records, in record order (:352-364)
            if (tid == 0) {
                q[0] = 'S';
                q[1] = 'A';
                q[2] = 'Z';
            }
            q += 3;
            for (uint32_t j = i0; j < i1; ++j) {
                if (j == i || wk.status[j] != PLO_ITEM_LIFTED) continue;
                const uint32_t sl = d.sa_off[j + 1] - d.sa_off[j];
                copy_span<VEC>(q, d.sa_text + d.sa_off[j], sl, tid, nt);
                q += sl;
            }
            if (tid == 0) q[0] = 0;
            q += 1;
        }
        if (nc > 0xffffu) {
            if (tid == 0) {
                q[0] = 'C';
                q[1] = 'G';
                q[2] = 'B';
                q[3] = 'I';
                rec_wr32(q + 4, nc);
            }
            copy_span<VEC>(q + 8, (const uint8_t *)cg, 4ull * nc, tid, nt);
            q += 8 + 4ull * nc;
        }
        o += size;
        ++k;
    }
}

}  // namespace plo
