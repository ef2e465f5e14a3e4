// tests/emu/emu_nm.cpp -- nm_core.hpp (the device code of plo_nm_dev) executed on the host by emulated waves (tests/emu/plo_wave.hpp), and
// records_core.hpp with DevRecords::item_nm set (the NM:i field of plo_records_build_dev).
// TEST INFRASTRUCTURE ONLY.  Built as a shared library (tests/emu_nm_lib.py) and, with -DEMU_NM_MAIN, as a program for the
// AddressSanitizer run: the CIGAR, the bases and the chromosome of every case sit in heap blocks of their exact sizes there, so a read
// outside a record's bases or outside a chromosome is caught.
#include "emu_records.cpp"

#include "../../portello_amd/csrc/nm_core.hpp"

namespace {
// one pass over the items (emu_md.cpp and emu_eqx.cpp run theirs through it too): item_seed 0 = the ticket loop `items` in one wave,
// otherwise `item(i)` for every item in shuffled order, a wave each
template <class Items, class Item>
void run_pass(uint32_t n, unsigned order_seed, unsigned item_seed, Items items, Item item) {
    if (!item_seed) {
        wv::EmuWave ew;
        ew.order_seed = order_seed;
        ew.run(items);
        return;
    }
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; ++i) order[i] = i;
    unsigned rs = item_seed;
    for (uint32_t i = n; i > 1; --i) {
        rs = rs * 1664525u + 1013904223u;
        std::swap(order[i - 1], order[(rs >> 8) % i]);
    }
    for (uint32_t i : order) {
        wv::EmuWave ew;
        ew.order_seed = order_seed;
        ew.run([&]() { item(i); });
    }
}

int run_nm(const DevBatch &bt, const DevWork &wk, DevNm d, unsigned order_seed, unsigned item_seed, uint64_t *n_cmp, uint32_t *err_item) {
    unsigned long long cmp_total = 0, lane_cmp[64] = {0};
    int err = NM_NO_ITEM;
    unsigned ticket = 0;
    d.n_cmp = &cmp_total;
    d.err_item = &err;
    d.ticket = &ticket;
    run_pass(
        wk.n_items, order_seed, item_seed, [&]() { nm_items(bt, wk, d); },
        [&](uint32_t i) {
            unsigned long long c = 0;
            nm_item(bt, wk, d, i, c);
            lane_cmp[wv::lane()] += c;
        });
    for (int l = 0; l < 64; ++l) cmp_total += lane_cmp[l];
    *n_cmp = cmp_total;
    *err_item = err == NM_NO_ITEM ? UINT32_MAX : (uint32_t)err;
    return err == NM_NO_ITEM ? PLO_OK : PLO_ERR_RANGE;
}

void fill_work(DevBatch &bt, DevWork &wk, const plo_batch_in *in, const plo_batch_out *lift) {
    memset(&bt, 0, sizeof(bt));
    bt.read_seq_len = in->read_seq_len;
    bt.read_seq_off = in->read_seq_off;
    bt.seq = in->seq;
    bt.seq_bytes = in->seq_bytes;
    bt.seg_read = in->seg_read;
    bt.seg_contig = in->seg_contig;
    bt.seq_fmt = in->seq_fmt;
    bt.n_reads = in->n_reads;
    bt.n_segs = in->n_segs;
    memset(&wk, 0, sizeof(wk));
    wk.n_items = lift->n_items;
    wk.item_seg = (uint32_t *)lift->item_seg;
    wk.item_cseg = (uint32_t *)lift->item_cseg;
    wk.status = (uint8_t *)lift->item_status;
    wk.mapq = (uint8_t *)lift->item_mapq;
    wk.chrom = (uint32_t *)lift->item_chrom_index;
    wk.pos = (int64_t *)lift->item_ref_pos;
    wk.cig_off = (uint64_t *)lift->item_cigar_off;
    wk.cig_len = (uint32_t *)lift->item_cigar_len;
    wk.out_cigar = (uint32_t *)lift->cigar;
}

// the source fields of DevNm, DevMd and DevEqx
AlnSrc fill_src(const uint64_t *item_seq_off, const uint8_t *rev_seq, const uint8_t *const *chrom_seq, const int *chrom_len, uint32_t n_chroms) {
    AlnSrc s;
    memset(&s, 0, sizeof(s));
    s.item_seq_off = item_seq_off;
    s.rev_seq = rev_seq;
    s.chrom_seq = chrom_seq;
    s.chrom_len = chrom_len;
    s.n_chroms = n_chroms;
    return s;
}

// a whole batch and its source: `lift` = host arrays of a lift result, item_seq_off / rev_seq = emu_finish_batch's, `ix` = the index
// description (its chromosomes)
struct BatchWalk {
    DevBatch bt;
    DevWork wk;
    std::vector<int> clen;
    AlnSrc src;
    BatchWalk(const plo_batch_in *in, const plo_batch_out *lift, const uint64_t *item_seq_off, const uint8_t *rev_seq, const plo_index_desc *ix)
        : clen(ix->n_chroms ? ix->n_chroms : 1, 0) {
        fill_work(bt, wk, in, lift);
        for (uint32_t c = 0; c < ix->n_chroms; ++c) clen[c] = (int)ix->chrom_len[c];
        src = fill_src(item_seq_off, rev_seq, ix->chrom_seq, clen.data(), ix->n_chroms);
    }
};

// one item on its own: ops[n_ops], the record's bases seq[(l_seq + 1) / 2] (flip != 0: handed over as the reversed bases of the finishing,
// otherwise as the batch's), the chromosome ref[chrom_len] and the item's position on it
struct OneWalk {
    const uint32_t zero = 0;
    const uint64_t off0 = 0;
    const uint8_t lifted = PLO_ITEM_LIFTED;
    uint32_t n_ops, l_seq;
    uint64_t seq_off;
    const uint8_t *ref;
    int chrom_len;
    int64_t ref_pos;
    DevBatch bt;
    DevWork wk;
    AlnSrc src;
    OneWalk(const uint32_t *ops, uint32_t n_ops_, const uint8_t *seq, uint32_t l_seq_, int flip, const uint8_t *ref_, int chrom_len_, int64_t ref_pos_)
        : n_ops(n_ops_), l_seq(l_seq_), seq_off(flip ? 0 : PLO_NO_FLIP), ref(ref_), chrom_len(chrom_len_), ref_pos(ref_pos_) {
        memset(&bt, 0, sizeof(bt));
        bt.read_seq_len = &l_seq;
        bt.read_seq_off = &off0;
        bt.seq = flip ? nullptr : seq;
        bt.seq_bytes = flip ? 0 : (l_seq + 1) / 2;
        bt.seg_read = &zero;
        bt.seq_fmt = PLO_SEQ_BAM4;
        bt.n_reads = bt.n_segs = 1;
        memset(&wk, 0, sizeof(wk));
        wk.n_items = 1;
        wk.item_seg = (uint32_t *)&zero;
        wk.status = (uint8_t *)&lifted;
        wk.chrom = (uint32_t *)&zero;
        wk.pos = &ref_pos;
        wk.cig_off = (uint64_t *)&off0;
        wk.cig_len = &n_ops;
        wk.out_cigar = (uint32_t *)ops;
        src = fill_src(&seq_off, flip ? seq : nullptr, &ref, &chrom_len, 1);
    }
    OneWalk(const OneWalk &) = delete;
};
}  // namespace

// a whole batch (BatchWalk).  item_nm: [n_items].  Returns PLO_OK or PLO_ERR_RANGE (*err_item = the lowest offending item).
extern "C" int emu_nm_batch(const plo_batch_in *in, const plo_batch_out *lift, const uint64_t *item_seq_off, const uint8_t *rev_seq, const plo_index_desc *ix,
                            unsigned order_seed, unsigned item_seed, uint32_t *item_nm, uint64_t *n_cmp, uint32_t *err_item) {
    const BatchWalk b(in, lift, item_seq_off, rev_seq, ix);
    DevNm d;
    memset(&d, 0, sizeof(d));
    static_cast<AlnSrc &>(d) = b.src;
    d.item_nm = item_nm;
    return run_nm(b.bt, b.wk, d, order_seed, item_seed, n_cmp, err_item);
}

// one item on its own (OneWalk).  -> PLO_OK / PLO_ERR_RANGE
extern "C" int emu_nm_one(const uint32_t *ops, uint32_t n_ops, const uint8_t *seq, uint32_t l_seq, int flip, const uint8_t *ref, int chrom_len, int64_t ref_pos,
                          unsigned order_seed, uint32_t *nm, uint64_t *n_cmp) {
    const OneWalk w(ops, n_ops, seq, l_seq, flip, ref, chrom_len, ref_pos);
    DevNm d;
    memset(&d, 0, sizeof(d));
    static_cast<AlnSrc &>(d) = w.src;
    d.item_nm = nm;
    uint32_t err_item;
    return run_nm(w.bt, w.wk, d, order_seed, order_seed ? 1u : 0u, n_cmp, &err_item);
}

// emu_records_build (tests/emu/emu_records.cpp) with DevRecords::item_nm: the records with NM:i behind ZM:C.  item_nm NULL: the same call.
extern "C" int emu_nm_records_build(const plo_batch_in *in, const plo_batch_out *lift, const plo_finish_out *fin, const uint32_t *sa_off, const uint8_t *sa_text,
                                    const plo_index_desc *ix, const plo_records_in *rin, const uint32_t *item_nm, int vec, int nthreads, unsigned order_seed,
                                    plo_records_out *out) {
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
    for (uint32_t r = 0; r < nr; ++r)
        for (int t = 0; t < nthreads; ++t) {
            if (vec) records_emit_read<true>(bt, wk, d, r, t, nthreads);
            else records_emit_read<false>(bt, wk, d, r, t, nthreads);
        }
    s->record_off[n_rec] = n_bytes;
    for (size_t k = 0; k < (size_t)n_bytes; ++k)
        if (s->out[k] == 0xEE) {  // (a byte of the fill may be a record's own: look again over another fill)
            std::vector<uint8_t> first(s->out, s->out + n_bytes);
            memset(s->out, 0x11, (size_t)n_bytes);
            for (uint32_t r = 0; r < nr; ++r)
                for (int t = 0; t < nthreads; ++t) {
                    if (vec) records_emit_read<true>(bt, wk, d, r, t, nthreads);
                    else records_emit_read<false>(bt, wk, d, r, t, nthreads);
                }
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

#ifdef EMU_NM_MAIN
// emu_nm_asan IN OUT.  IN: u32 n_cases, then per case u32 n_ops, u32 l_seq, u32 flip, u32 front, i32 chrom_len, i64 ref_pos, u32 order_seed, the ops,
// the bases, the chromosome.  Every array goes into a heap block of its exact size; with `front` the bases lie that many bytes into a
// block that ends with them (their start then meets every residue of the 8-byte words).  OUT per case: u32 status, u32 nm, u64 n_cmp.
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
        uint32_t nm = 0;
        uint64_t cmp = 0;
        const uint32_t st = (uint32_t)emu_nm_one(ops, n_ops, block + front, l_seq, (int)flip, ref, clen, pos, seed, &nm, &cmp);
        fwrite(&st, 4, 1, o);
        fwrite(&nm, 4, 1, o);
        fwrite(&cmp, 8, 1, o);
        free(ops);
        free(block);
        free(ref);
    }
    fclose(f);
    fclose(o);
    return 0;
}
#endif
