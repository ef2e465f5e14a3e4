// tests/emu/emu_records.cpp -- records_core.hpp (the device code of plo_records_build_dev) executed on the host: the plan and the
// scans by emulated waves (tests/emu/plo_wave.hpp), the emit by plain loops over the threads of a workgroup.
// TEST INFRASTRUCTURE ONLY.  Built as a shared library (tests/emu_records_lib.py) and, with -DEMU_RECORDS_MAIN, as a program for the
// AddressSanitizer run: every input sits in a heap block of its exact size there, so a read outside a record is caught.
#include <plo_wave.hpp>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../portello_amd/csrc/records_core.hpp"

using namespace plo;

namespace {
struct RecState {
    std::vector<uint32_t> item_read, plan;
    std::vector<unsigned long long> size, start, partial;
    uint64_t *record_off = nullptr;
    uint8_t *out = nullptr;
    ~RecState() {
        free(record_off);
        free(out);
    }
};
RecState *g_rec = nullptr;

void scan64(const unsigned long long *in, uint32_t n, unsigned long long *out, std::vector<unsigned long long> &partial, unsigned order_seed) {
    const uint32_t nb = n ? (n + REC_SCAN_CHUNK - 1) / REC_SCAN_CHUNK : 1;
    partial.assign(nb, 0);
    for (uint32_t w = 0; w < nb; ++w) {
        wv::EmuWave ew;
        ew.order_seed = order_seed;
        ew.run([&]() { rec_scan_sums(in, n, w, partial.data()); });
    }
    {
        wv::EmuWave ew;
        ew.order_seed = order_seed;
        ew.run([&]() { rec_scan_partials(partial.data(), nb, out + n); });
    }
    for (uint32_t w = 0; w < nb; ++w) {
        wv::EmuWave ew;
        ew.order_seed = order_seed;
        ew.run([&]() { rec_scan_apply(in, n, w, partial.data(), out); });
    }
}
}  // namespace

extern "C" void emu_scan64(const uint64_t *in, uint32_t n, uint64_t *out /* n + 1 */, unsigned order_seed) {
    std::vector<unsigned long long> partial;
    scan64((const unsigned long long *)in, n, (unsigned long long *)out, partial, order_seed);
}

// `lift`, `fin`, `sa_off` / `sa_text`: host arrays (the C oracle's lift result, emu_finish_batch's and emu_sa_segments' results of
// tests/emu/emu_harness.cpp); `ix`: the index description (strand of the contig segments).  err4: the four bounds counters.
// Returns 0, or 1 when a bounds check failed (nothing is emitted then, as on the device).
extern "C" int emu_records_build(const plo_batch_in *in, const plo_batch_out *lift, const plo_finish_out *fin, const uint32_t *sa_off, const uint8_t *sa_text,
                                 const plo_index_desc *ix, const plo_records_in *rin, int vec, int nthreads, unsigned order_seed, plo_records_out *out,
                                 unsigned *err4) {
    memset(out, 0, sizeof(*out));
    DevBatch bt;
    memset(&bt, 0, sizeof(bt));
    bt.read_seq_len = in->read_seq_len;
    bt.seg_read = in->seg_read;
    bt.seg_contig = in->seg_contig;
    bt.seq_fmt = in->seq_fmt;
    bt.n_reads = in->n_reads;
    bt.n_segs = in->n_segs;
    DevWork wk;
    memset(&wk, 0, sizeof(wk));
    const uint32_t n = lift->n_items, nr = in->n_reads;
    wk.n_items = n;
    wk.item_seg = (uint32_t *)lift->item_seg;
    wk.item_cseg = (uint32_t *)lift->item_cseg;
    wk.status = (uint8_t *)lift->item_status;
    wk.mapq = (uint8_t *)lift->item_mapq;
    wk.chrom = (uint32_t *)lift->item_chrom_index;
    wk.pos = (int64_t *)lift->item_ref_pos;
    wk.cig_off = (uint64_t *)lift->item_cigar_off;
    wk.cig_len = (uint32_t *)lift->item_cigar_len;
    wk.out_cigar = (uint32_t *)lift->cigar;
    delete g_rec;
    RecState *s = g_rec = new RecState();
    s->item_read.assign(n ? n : 1, 0);
    for (uint32_t i = 0; i < n; ++i) s->item_read[i] = in->seg_read[lift->item_seg[i]];
    s->plan.assign((size_t)(nr ? nr : 1) * REC_PLAN_WORDS, 0);
    s->size.assign((size_t)3 * (nr ? nr : 1), 0);
    s->start.assign((size_t)3 * ((size_t)nr + 1), 0);
    std::vector<uint8_t> cs_fwd(ix->seg_is_fwd_strand, ix->seg_is_fwd_strand + ix->n_segments);
    DevRecords d;
    memset(&d, 0, sizeof(d));
    d.records = rin->records;
    d.records_bytes = rin->records_bytes;
    d.read_rec_off = rin->read_rec_off;
    d.contig_name_off = rin->contig_name_off;
    d.contig_names = rin->contig_names;
    d.is_target_region = rin->is_target_region;
    d.item_flag = fin->item_flag;
    d.item_bin = fin->item_bin;
    d.item_ref_end = fin->item_ref_end;
    d.item_seq_off = fin->item_seq_off;
    d.item_qual_off = fin->item_qual_off;
    d.item_read = s->item_read.data();
    d.read_n_lifted = fin->read_n_lifted;
    d.read_unmapped_flag = fin->read_unmapped_flag;
    d.read_seq_off = fin->read_seq_off;
    d.read_qual_off = fin->read_qual_off;
    d.rev_seq = fin->rev_seq;
    d.rev_qual = fin->rev_qual;
    d.sa_off = sa_off;
    d.sa_text = sa_text;
    d.cs_is_fwd = cs_fwd.data();
    d.contig_seg_off = ix->contig_seg_off;
    d.plan = s->plan.data();
    d.size = s->size.data();
    d.start = s->start.data();
    unsigned err[REC_ERR_N] = {0, 0, 0, 0};
    d.err = err;
    for (uint32_t r = 0; r < nr; ++r) {
        wv::EmuWave ew;
        ew.order_seed = order_seed;
        ew.run([&]() { records_plan_read(bt, wk, d, r); });
    }
    for (int k = 0; k < REC_ERR_N; ++k) err4[k] = err[k];
    if (err[0] || err[1] || err[2] || err[3]) return 1;
    for (int y = 0; y < 3; ++y) scan64(s->size.data() + (size_t)y * nr, nr, s->start.data() + (size_t)y * ((size_t)nr + 1), s->partial, order_seed);
    const unsigned long long n_bytes = s->start[nr], n_rec = s->start[(size_t)nr + 1 + nr], n_unm = s->start[2 * ((size_t)nr + 1) + nr];
    // blocks of the exact size: a write (or, under AddressSanitizer, a read) outside them is an error
    s->out = (uint8_t *)aligned_alloc(16, (size_t)((n_bytes + 15) & ~15ull) + 16);
    memset(s->out, 0xEE, (size_t)((n_bytes + 15) & ~15ull) + 16);
    s->record_off = (uint64_t *)malloc((size_t)(n_rec + 1) * 8);
    d.out = s->out;
    d.record_off = s->record_off;
    for (uint32_t r = 0; r < nr; ++r)
        for (int t = 0; t < nthreads; ++t) {
            if (vec) records_emit_read<true>(bt, wk, d, r, t, nthreads);
            else records_emit_read<false>(bt, wk, d, r, t, nthreads);
        }
    s->record_off[n_rec] = n_bytes;
    {  // every byte of [0, n_bytes) is written: a second emit over another fill gives the same bytes
        std::vector<uint8_t> first(s->out, s->out + n_bytes);
        memset(s->out, 0x11, (size_t)n_bytes);
        for (uint32_t r = 0; r < nr; ++r)
            for (int t = 0; t < nthreads; ++t) {
                if (vec) records_emit_read<true>(bt, wk, d, r, t, nthreads);
                else records_emit_read<false>(bt, wk, d, r, t, nthreads);
            }
        if (n_bytes && memcmp(first.data(), s->out, (size_t)n_bytes) != 0) return 3;  // a byte no store reached
    }
    for (size_t k = (size_t)n_bytes; k < (size_t)((n_bytes + 15) & ~15ull) + 16; ++k)
        if (s->out[k] != 0xEE) return 2;  // a store behind the last record
    out->bytes = s->out;
    out->n_bytes = n_bytes;
    out->n_records = (uint32_t)n_rec;
    out->record_off = s->record_off;
    out->n_unmapped_copies = (uint32_t)n_unm;
    out->n_lifted = (uint32_t)(n_rec - n_unm);
    return 0;
}

extern "C" void emu_records_free(void) {
    delete g_rec;
    g_rec = nullptr;
}

#ifdef EMU_RECORDS_MAIN
// emu_records_asan IN OUT: the unmapped copies of forward-strand records that have no lift items (plan, scan, emit with both copy
// instantiations).  IN: u64 records_bytes, u32 n_reads, the records, u64 read_rec_off[n_reads].  OUT: u64 n_bytes, u32 n_records, the bytes.
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t nb = 0;
    uint32_t nr = 0;
    if (fread(&nb, 8, 1, f) != 1 || fread(&nr, 4, 1, f) != 1) return 2;
    uint8_t *records = (uint8_t *)malloc(nb ? nb : 1);  // exact size
    uint64_t *rec_off = (uint64_t *)malloc((size_t)(nr ? nr : 1) * 8);
    if ((nb && fread(records, 1, nb, f) != nb) || (nr && fread(rec_off, 8, nr, f) != nr)) return 2;
    fclose(f);
    std::vector<uint32_t> seq_len(nr ? nr : 1, 0), n_lifted(nr ? nr : 1, 0), seg_read(1, 0), seg_contig(1, 0), zero32(2, 0);
    std::vector<uint16_t> uflag(nr ? nr : 1, 0);
    std::vector<uint64_t> no_flip(nr ? nr : 1, PLO_NO_FLIP);
    for (uint32_t r = 0; r < nr; ++r) {
        const uint8_t *p = records + rec_off[r] + 4;
        seq_len[r] = rec_rd32(p + 16);
        unsigned fl = rec_rd16(p + 14);
        if (fl & 0x10) return 3;  // forward-strand records only (no finishing pass in this program)
        uflag[r] = (uint16_t)((fl | 0x4) & ~0x800u);
    }
    plo_batch_in in;
    memset(&in, 0, sizeof(in));
    in.n_reads = nr;
    in.read_seq_len = seq_len.data();
    in.seg_read = seg_read.data();
    in.seg_contig = seg_contig.data();
    in.seq_fmt = PLO_SEQ_BAM4;
    plo_batch_out lift;
    memset(&lift, 0, sizeof(lift));
    plo_finish_out fin;
    memset(&fin, 0, sizeof(fin));
    fin.read_n_lifted = n_lifted.data();
    fin.read_unmapped_flag = uflag.data();
    fin.read_seq_off = no_flip.data();
    fin.read_qual_off = no_flip.data();
    plo_index_desc ix;
    memset(&ix, 0, sizeof(ix));
    uint8_t fwd = 1;
    ix.seg_is_fwd_strand = &fwd;
    ix.contig_seg_off = zero32.data();
    plo_records_in rin;
    memset(&rin, 0, sizeof(rin));
    rin.records = records;
    rin.records_bytes = nb;
    rin.read_rec_off = rec_off;
    rin.contig_name_off = zero32.data();
    rin.contig_names = &fwd;
    std::vector<uint8_t> first;
    for (int vec = 1; vec >= 0; --vec) {
        plo_records_out out;
        unsigned err[4];
        int rc = emu_records_build(&in, &lift, &fin, zero32.data(), &fwd, &ix, &rin, vec, 7, vec ? 0u : 5u, &out, err);
        if (rc) return 10 + rc;
        if (vec) {
            first.assign(out.bytes, out.bytes + out.n_bytes);
            FILE *o = fopen(argv[2], "wb");
            if (!o) return 2;
            fwrite(&out.n_bytes, 8, 1, o);
            fwrite(&out.n_records, 4, 1, o);
            fwrite(out.bytes, 1, out.n_bytes, o);
            fclose(o);
        } else if (first.size() != out.n_bytes || memcmp(first.data(), out.bytes, out.n_bytes) != 0) {
            return 4;  // the byte copy disagrees with the 16-byte one
        }
    }
    emu_records_free();
    free(records);
    free(rec_off);
    return 0;
}
#endif
