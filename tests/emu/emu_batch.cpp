// tests/emu/emu_batch.cpp -- batch_core.hpp (the device code of plo_batch_build_dev) executed on the host: the plan, the scans and the emit
// by emulated waves (tests/emu/plo_wave.hpp), the label table by a plain loop over the contigs.
// TEST INFRASTRUCTURE ONLY.  Built as a shared library (tests/emu_batch_lib.py) and, with -DEMU_BATCH_MAIN, as a program for the
// AddressSanitizer + UBSan run: every input sits in a heap block of its exact size there, so a read outside a record is caught.
#include <plo_wave.hpp>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../portello_amd/csrc/batch_core.hpp"

using namespace plo;

namespace {
struct BatchState {
    std::vector<uint32_t> table, plan, err_kind, t_nops, t_ctext, t_clen, t_contig, t_dst;
    std::vector<unsigned long long> size, start, partial, t_key;
    std::vector<long long> t_pos;
    std::vector<uint8_t> t_fwd;
    // outputs: blocks of the exact size
    uint8_t *rev = nullptr, *seg_fwd = nullptr;
    uint32_t *len = nullptr, *seg_read = nullptr, *seg_contig = nullptr, *coff = nullptr, *cigar = nullptr;
    uint64_t *soff = nullptr, *qoff = nullptr;
    uint16_t *flags = nullptr;
    int64_t *seg_pos = nullptr;
    ~BatchState() {
        free(rev);
        free(seg_fwd);
        free(len);
        free(seg_read);
        free(seg_contig);
        free(coff);
        free(cigar);
        free(soff);
        free(qoff);
        free(flags);
        free(seg_pos);
    }
};
BatchState *g_bb = nullptr;

template <class T>
T *exact(size_t n) {
    return (T *)malloc((n ? n : 1) * sizeof(T));
}

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

// plo_batch_build_dev's steps with host pointers.  -> PLO_OK, PLO_ERR_INVALID_ARG (a bounds check failed: bounds[REC_ERR_*] counts them),
// PLO_ERR_DATA (out->err_read / err_kind) or PLO_ERR_RANGE; the arrays of `out` live until emu_batch_free / the next call
extern "C" int emu_batch_build(const plo_batch_build_in *in, unsigned order_seed, plo_batch_build_out *out, int *bounds) {
    memset(out, 0, sizeof(*out));
    out->err_read = UINT32_MAX;
    for (int k = 0; k < REC_ERR_N; ++k) bounds[k] = 0;
    delete g_bb;
    BatchState *s = g_bb = new BatchState();
    const uint32_t nr = in->n_reads;
    uint32_t slots = 64;
    while (slots < 2 * in->n_contigs) slots <<= 1;
    s->table.assign(slots, 0);
    s->plan.assign((size_t)(nr ? nr : 1) * BB_PLAN_WORDS, 0);
    s->size.assign((size_t)2 * (nr ? nr : 1), 0);
    s->start.assign((size_t)2 * ((size_t)nr + 1), 0);
    s->err_kind.assign(nr ? nr : 1, 0);
    int err[BB_ERR_WORDS] = {BB_NO_READ, 0, 0, 0, 0};
    DevBatchBuild d;
    memset(&d, 0, sizeof(d));
    d.records = in->records;
    d.records_bytes = in->records_bytes;
    d.read_rec_off = in->read_rec_off;
    d.n_reads = nr;
    d.n_contigs = in->n_contigs;
    d.contig_name_off = in->contig_name_off;
    d.contig_names = in->contig_names;
    d.table = s->table.data();
    d.table_mask = slots - 1;
    d.plan = s->plan.data();
    d.size = s->size.data();
    d.start = s->start.data();
    d.err_kind = s->err_kind.data();
    d.err = err;
    for (uint32_t c = 0; c < in->n_contigs; ++c) bb_table_insert(d, c);
    for (uint32_t r = 0; r < nr; ++r) {
        wv::EmuWave ew;
        ew.order_seed = order_seed;
        ew.run([&]() { batch_plan_read(d, r); });
    }
    for (int k = 0; k < REC_ERR_N; ++k) bounds[k] = err[1 + k];
    if (err[1 + REC_ERR_OFFSET] || err[1 + REC_ERR_BLOCK] || err[1 + REC_ERR_LAYOUT]) return PLO_ERR_INVALID_ARG;
    if (err[0] != BB_NO_READ) {
        out->err_read = (uint32_t)err[0];
        out->err_kind = s->err_kind[err[0]];
        return PLO_ERR_DATA;
    }
    for (int y = 0; y < 2; ++y) scan64(s->size.data() + (size_t)y * nr, nr, s->start.data() + (size_t)y * ((size_t)nr + 1), s->partial, order_seed);
    const unsigned long long ns = s->start[nr], n_ops = s->start[(size_t)nr + 1 + nr];
    if (n_ops > 0x7fffffffull || ns > 0xfffffffeull) return PLO_ERR_RANGE;
    s->t_key.assign(ns ? ns : 1, 0);
    s->t_nops.assign(ns ? ns : 1, 0);
    s->t_ctext.assign(ns ? ns : 1, 0);
    s->t_clen.assign(ns ? ns : 1, 0);
    s->t_contig.assign(ns ? ns : 1, 0);
    s->t_dst.assign(ns ? ns : 1, 0);
    s->t_pos.assign(ns ? ns : 1, 0);
    s->t_fwd.assign(ns ? ns : 1, 0);
    d.t_key = s->t_key.data();
    d.t_nops = s->t_nops.data();
    d.t_ctext = s->t_ctext.data();
    d.t_clen = s->t_clen.data();
    d.t_contig = s->t_contig.data();
    d.t_dst = s->t_dst.data();
    d.t_pos = s->t_pos.data();
    d.t_fwd = s->t_fwd.data();
    d.read_is_reverse = s->rev = exact<uint8_t>(nr);
    d.read_seq_len = s->len = exact<uint32_t>(nr);
    d.read_seq_off = s->soff = exact<uint64_t>(nr);
    d.read_qual_off = s->qoff = exact<uint64_t>(nr);
    d.read_flags = s->flags = exact<uint16_t>(nr);
    d.seg_read = s->seg_read = exact<uint32_t>(ns);
    d.seg_contig = s->seg_contig = exact<uint32_t>(ns);
    d.seg_pos = s->seg_pos = exact<int64_t>(ns);
    d.seg_fwd = s->seg_fwd = exact<uint8_t>(ns);
    d.seg_cigar_off = s->coff = exact<uint32_t>(ns + 1);
    d.cigar = s->cigar = exact<uint32_t>(n_ops);
    // a fill no result can be mistaken for: an element that no store reached stays visible to the comparison
    memset(s->seg_read, 0xEE, (ns ? ns : 1) * 4);
    memset(s->seg_contig, 0xEE, (ns ? ns : 1) * 4);
    memset(s->coff, 0xEE, (ns + 1) * 4);
    memset(s->cigar, 0xEE, (n_ops ? n_ops : 1) * 4);
    if (!nr) s->coff[0] = 0;
    for (uint32_t r = 0; r < nr; ++r) {
        wv::EmuWave ew;
        ew.order_seed = order_seed;
        ew.run([&]() { batch_emit_read(d, r); });
    }
    plo_batch_in &bi = out->batch;
    bi.n_reads = nr;
    bi.read_is_reverse = s->rev;
    bi.read_seq_len = s->len;
    bi.read_seq_off = s->soff;
    bi.seq = in->records;
    bi.seq_bytes = in->records_bytes;
    bi.seq_fmt = PLO_SEQ_BAM4;
    bi.n_segs = (uint32_t)ns;
    bi.seg_read = s->seg_read;
    bi.seg_contig = s->seg_contig;
    bi.seg_pos = s->seg_pos;
    bi.seg_is_fwd_strand = s->seg_fwd;
    bi.seg_cigar_off = s->coff;
    bi.cigar = s->cigar;
    out->fin.read_flags = s->flags;
    out->fin.qual = in->records;
    out->fin.read_qual_off = s->qoff;
    out->fin.qual_bytes = in->records_bytes;
    return PLO_OK;
}

extern "C" void emu_batch_free(void) {
    delete g_bb;
    g_bb = nullptr;
}

#ifdef EMU_BATCH_MAIN
// emu_batch_asan IN OUT.  IN: u64 records_bytes, u32 n_reads, u32 n_contigs, u32 names_bytes, the records, u64 read_rec_off[n_reads],
// u32 contig_name_off[n_contigs + 1], the names.  OUT: u32 status, err_read, err_kind, n_reads, n_segs, n_ops, then (status 0) the arrays
// in the order read_is_reverse, read_seq_len, read_seq_off, read_flags, read_qual_off, seg_read, seg_contig, seg_pos, seg_is_fwd_strand,
// seg_cigar_off, cigar
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t nb = 0;
    uint32_t nr = 0, nc = 0, nn = 0;
    if (fread(&nb, 8, 1, f) != 1 || fread(&nr, 4, 1, f) != 1 || fread(&nc, 4, 1, f) != 1 || fread(&nn, 4, 1, f) != 1) return 2;
    uint8_t *records = (uint8_t *)malloc(nb ? nb : 1);  // exact size
    uint64_t *rec_off = (uint64_t *)malloc((size_t)(nr ? nr : 1) * 8);
    uint32_t *name_off = (uint32_t *)malloc(((size_t)nc + 1) * 4);
    uint8_t *names = (uint8_t *)malloc(nn ? nn : 1);
    if ((nb && fread(records, 1, nb, f) != nb) || (nr && fread(rec_off, 8, nr, f) != nr) || fread(name_off, 4, (size_t)nc + 1, f) != (size_t)nc + 1 ||
        (nn && fread(names, 1, nn, f) != nn))
        return 2;
    fclose(f);
    plo_batch_build_in in;
    memset(&in, 0, sizeof(in));
    in.records = records;
    in.records_bytes = nb;
    in.read_rec_off = rec_off;
    in.n_reads = nr;
    in.n_contigs = nc;
    in.contig_name_off = name_off;
    in.contig_names = names;
    plo_batch_build_out out;
    int bounds[REC_ERR_N];
    const int st = emu_batch_build(&in, 3u, &out, bounds);
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    const uint32_t ns = out.batch.n_segs, n_ops = st == PLO_OK ? out.batch.seg_cigar_off[ns] : 0;
    const uint32_t head[6] = {(uint32_t)st, out.err_read, out.err_kind, nr, ns, n_ops};
    fwrite(head, 4, 6, o);
    if (st == PLO_OK) {
        fwrite(out.batch.read_is_reverse, 1, nr, o);
        fwrite(out.batch.read_seq_len, 4, nr, o);
        fwrite(out.batch.read_seq_off, 8, nr, o);
        fwrite(out.fin.read_flags, 2, nr, o);
        fwrite(out.fin.read_qual_off, 8, nr, o);
        fwrite(out.batch.seg_read, 4, ns, o);
        fwrite(out.batch.seg_contig, 4, ns, o);
        fwrite(out.batch.seg_pos, 8, ns, o);
        fwrite(out.batch.seg_is_fwd_strand, 1, ns, o);
        fwrite(out.batch.seg_cigar_off, 4, (size_t)ns + 1, o);
        fwrite(out.batch.cigar, 4, n_ops, o);
    }
    fclose(o);
    emu_batch_free();
    free(records);
    free(rec_off);
    free(name_off);
    free(names);
    return 0;
}
#endif
