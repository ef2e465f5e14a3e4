// tests/emu/emu_eqx.cpp -- eqx_core.hpp (the device code of plo_eqx_dev) executed on the host by emulated waves (tests/emu/plo_wave.hpp): the
// count pass, the 64-bit scan of records_core.hpp and the emit pass; and records_core.hpp with DevRecords::item_eqx_off / eqx_ops set (the
// = / X CIGAR of plo_records_build_dev in the record or in CG:B,I), with or without item_nm and item_md_off / md_text.
// TEST INFRASTRUCTURE ONLY.  Built as a shared library (tests/emu_eqx_lib.py) and, with -DEMU_EQX_MAIN, as a program for the
// AddressSanitizer run: the CIGAR, the bases, the chromosome and the ops of every case sit in heap blocks of their exact sizes there, so a
// read outside a record's bases or a chromosome and a store outside the item's ops are caught.
#include "emu_md.cpp"

#include "../../portello_amd/csrc/eqx_core.hpp"

namespace {
constexpr uint32_t EQX_CANARY = 0xA5A5A5A5u;  // no op of a test's CIGAR (an H of 2^28 - 1 bases and change)

template <bool WRITE>
void run_eqx_pass(const DevBatch &bt, const DevWork &wk, DevEqx d, unsigned order_seed, unsigned item_seed) {
    unsigned ticket = 0;
    d.ticket = &ticket;
    run_pass(
        wk.n_items, order_seed, item_seed, [&]() { eqx_items<WRITE>(bt, wk, d); }, [&](uint32_t i) { eqx_item<WRITE>(bt, wk, d, i); });
}

struct EqxResult {
    std::vector<unsigned long long> len, off;  // [n], [n + 1]
    uint32_t *block = nullptr;                 // guard + total + guard ops
    size_t guard = 0;
    int status = PLO_OK, check = 0;            // check: 2 = a store outside the ops, 3 = an op no store reached
    uint32_t err_item = UINT32_MAX;
    ~EqxResult() { free(block); }
    const uint32_t *ops() const { return block + guard; }
    unsigned long long total() const { return off.empty() ? 0 : off.back(); }
};

// count, scan, emit.  The ops lie in a heap block of guard + total + guard dwords filled with EQX_CANARY.
void run_eqx(const DevBatch &bt, const DevWork &wk, DevEqx d, unsigned order_seed, unsigned item_seed, size_t guard, EqxResult &r) {
    const uint32_t n = wk.n_items;
    int err = NM_NO_ITEM;
    r.len.assign(n ? n : 1, 0xDEADBEEFull);
    r.off.assign((size_t)n + 1, 0);
    d.item_len = r.len.data();
    d.err_item = &err;
    run_eqx_pass<false>(bt, wk, d, order_seed, item_seed);
    if (err != NM_NO_ITEM) {
        r.status = PLO_ERR_RANGE;
        r.err_item = (uint32_t)err;
        return;
    }
    std::vector<unsigned long long> partial;
    scan64(r.len.data(), n, r.off.data(), partial, order_seed);
    const size_t total = (size_t)r.off[n], words = guard + total + guard;
    r.guard = guard;
    r.block = (uint32_t *)malloc(words ? words * 4 : 1);
    for (size_t k = 0; k < words; ++k) r.block[k] = EQX_CANARY;
    d.item_eqx_off = r.off.data();
    d.eqx_ops = r.block + guard;
    run_eqx_pass<true>(bt, wk, d, order_seed, item_seed);
    for (size_t k = 0; k < guard; ++k)
        if (r.block[k] != EQX_CANARY || r.block[guard + total + k] != EQX_CANARY) r.check = 2;
    for (size_t k = 0; k < total; ++k)
        if (r.block[guard + k] == EQX_CANARY) r.check = 3;
}

EqxResult *g_eqx = nullptr;
}  // namespace

// a whole batch, as emu_md_batch.  item_eqx_off: [n_items + 1].  Returns PLO_OK or PLO_ERR_RANGE (*err_item = the lowest offending item), or
// -2 / -3 when the emit stored outside the ops / left one of them unwritten.  The ops stay with the library: emu_eqx_ops copies them.
extern "C" int emu_eqx_batch(const plo_batch_in *in, const plo_batch_out *lift, const uint64_t *item_seq_off, const uint8_t *rev_seq, const plo_index_desc *ix,
                             unsigned order_seed, unsigned item_seed, uint64_t *item_eqx_off, uint64_t *item_len, uint32_t *err_item) {
    const BatchWalk b(in, lift, item_seq_off, rev_seq, ix);
    DevEqx d;
    memset(&d, 0, sizeof(d));
    static_cast<AlnSrc &>(d) = b.src;
    delete g_eqx;
    g_eqx = new EqxResult();
    run_eqx(b.bt, b.wk, d, order_seed, item_seed, 16, *g_eqx);
    *err_item = g_eqx->err_item;
    if (g_eqx->status != PLO_OK) return g_eqx->status;
    for (uint32_t i = 0; i <= b.wk.n_items; ++i) item_eqx_off[i] = g_eqx->off[i];
    for (uint32_t i = 0; i < b.wk.n_items; ++i) item_len[i] = g_eqx->len[i];
    return g_eqx->check ? -g_eqx->check : PLO_OK;
}
extern "C" void emu_eqx_ops(uint32_t *dst) {
    if (g_eqx && g_eqx->total()) memcpy(dst, g_eqx->ops(), (size_t)g_eqx->total() * 4);
}
extern "C" void emu_eqx_free() {
    delete g_eqx;
    g_eqx = nullptr;
}

namespace {
// one item on its own, as md_one
void eqx_one(const uint32_t *ops, uint32_t n_ops, const uint8_t *seq, uint32_t l_seq, int flip, const uint8_t *ref, int chrom_len, int64_t ref_pos, unsigned order_seed,
             size_t guard, EqxResult &r) {
    const OneWalk w(ops, n_ops, seq, l_seq, flip, ref, chrom_len, ref_pos);
    DevEqx d;
    memset(&d, 0, sizeof(d));
    static_cast<AlnSrc &>(d) = w.src;
    run_eqx(w.bt, w.wk, d, order_seed, order_seed ? 1u : 0u, guard, r);
}
}  // namespace

// -> PLO_OK / PLO_ERR_RANGE / -2 / -3 (see emu_eqx_batch) / -4 (more ops than cap).  *len: the count pass's op count; out[0, *len)
extern "C" int emu_eqx_one(const uint32_t *ops, uint32_t n_ops, const uint8_t *seq, uint32_t l_seq, int flip, const uint8_t *ref, int chrom_len, int64_t ref_pos,
                           unsigned order_seed, uint64_t *len, uint32_t *out, uint64_t cap) {
    EqxResult r;
    eqx_one(ops, n_ops, seq, l_seq, flip, ref, chrom_len, ref_pos, order_seed, 16, r);
    *len = 0;
    if (r.status != PLO_OK) return r.status;
    *len = r.len[0];
    if (r.total() != r.len[0] || r.total() > cap) return -4;
    if (r.total()) memcpy(out, r.ops(), (size_t)r.total() * 4);
    return r.check ? -r.check : PLO_OK;
}

// emu_md_records_build (tests/emu/emu_md.cpp) with DevRecords::item_eqx_off / eqx_ops as well: the CIGAR of every lifted record is the
// result's.  item_nm, item_md_off and item_eqx_off may each be NULL.
extern "C" int emu_eqx_records_build(const plo_batch_in *in, const plo_batch_out *lift, const plo_finish_out *fin, const uint32_t *sa_off, const uint8_t *sa_text,
                                     const plo_index_desc *ix, const plo_records_in *rin, const uint32_t *item_nm, const uint64_t *item_md_off, const uint8_t *md_text,
                                     const uint64_t *item_eqx_off, const uint32_t *eqx_ops, int vec, int nthreads, unsigned order_seed, plo_records_out *out) {
    memset(out, 0, sizeof(*out));
    DevBatch bt;
    DevWork wk;
    fill_work(bt, wk, in, lift);
    const uint32_t n = lift->n_items, nr = in->n_reads;
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
    d.item_nm = item_nm;
    d.item_md_off = item_md_off;
    d.md_text = item_md_off ? md_text : nullptr;
    d.item_eqx_off = item_eqx_off;
    d.eqx_ops = item_eqx_off ? eqx_ops : nullptr;
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
    if (err[0] || err[1] || err[2] || err[3]) return 1;
    for (int y = 0; y < 3; ++y) scan64(s->size.data() + (size_t)y * nr, nr, s->start.data() + (size_t)y * ((size_t)nr + 1), s->partial, order_seed);
    const unsigned long long n_bytes = s->start[nr], n_rec = s->start[(size_t)nr + 1 + nr], n_unm = s->start[2 * ((size_t)nr + 1) + nr];
    const size_t room = (size_t)((n_bytes + 15) & ~15ull) + 16;
    s->out = (uint8_t *)aligned_alloc(16, room);
    memset(s->out, 0xEE, room);
    s->record_off = (uint64_t *)malloc((size_t)(n_rec + 1) * 8);
    d.out = s->out;
    d.record_off = s->record_off;
    auto emit = [&]() {
        for (uint32_t r = 0; r < nr; ++r)
            for (int t = 0; t < nthreads; ++t) {
                if (vec) records_emit_read<true>(bt, wk, d, r, t, nthreads);
                else records_emit_read<false>(bt, wk, d, r, t, nthreads);
            }
    };
    emit();
    s->record_off[n_rec] = n_bytes;
    for (size_t k = 0; k < (size_t)n_bytes; ++k)
        if (s->out[k] == 0xEE) {  // (a byte of the fill may be a record's own: look again over another fill)
            std::vector<uint8_t> first(s->out, s->out + n_bytes);
            memset(s->out, 0x11, (size_t)n_bytes);
            emit();
            if (memcmp(first.data(), s->out, (size_t)n_bytes) != 0) return 3;  // a byte no store reached
            break;
        }
    for (size_t k = (size_t)n_bytes; k < room; ++k)
        if (s->out[k] != 0xEE) return 2;  // a store behind the last record
    out->bytes = s->out;
    out->n_bytes = n_bytes;
    out->n_records = (uint32_t)n_rec;
    out->record_off = s->record_off;
    out->n_unmapped_copies = (uint32_t)n_unm;
    out->n_lifted = (uint32_t)(n_rec - n_unm);
    return 0;
}

#ifdef EMU_EQX_MAIN
// emu_eqx_asan IN OUT.  IN: emu_nm_asan's (u32 n_cases, then per case u32 n_ops, u32 l_seq, u32 flip, u32 front, i32 chrom_len, i64 ref_pos,
// u32 order_seed, the ops, the bases, the chromosome).  Every array goes into a heap block of its exact size, the output ops too (no guard
// around them).  OUT per case: i32 status, u64 len, the len ops.
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    FILE *o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    uint32_t n_cases = 0;
    if (fread(&n_cases, 4, 1, f) != 1) return 2;
    for (uint32_t k = 0; k < n_cases; ++k) {
        uint32_t h[4], seed;
        int32_t clen;
        int64_t pos;
        if (fread(h, 4, 4, f) != 4 || fread(&clen, 4, 1, f) != 1 || fread(&pos, 8, 1, f) != 1 || fread(&seed, 4, 1, f) != 1) return 2;
        const uint32_t n_ops = h[0], l_seq = h[1], flip = h[2], front = h[3], seqb = (l_seq + 1) / 2;
        uint32_t *ops = (uint32_t *)malloc((size_t)n_ops * 4);
        uint8_t *block = (uint8_t *)malloc((size_t)front + seqb);
        uint8_t *ref = (uint8_t *)malloc((size_t)clen);
        if ((n_ops && fread(ops, 4, n_ops, f) != n_ops) || (seqb && fread(block + front, 1, seqb, f) != seqb) || (clen && fread(ref, 1, (size_t)clen, f) != (size_t)clen)) return 2;
        EqxResult r;
        eqx_one(ops, n_ops, block + front, l_seq, (int)flip, ref, clen, pos, seed, 0, r);
        const int32_t st = r.status != PLO_OK ? r.status : r.check ? -r.check : r.total() != r.len[0] ? -4 : PLO_OK;
        const uint64_t len = st == PLO_OK ? r.total() : 0;
        fwrite(&st, 4, 1, o);
        fwrite(&len, 8, 1, o);
        if (len) fwrite(r.ops(), 4, (size_t)len, o);
        free(ops);
        free(block);
        free(ref);
    }
    fclose(f);
    fclose(o);
    return 0;
}
#endif
