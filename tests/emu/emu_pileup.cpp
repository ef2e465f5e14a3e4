// tests/emu/emu_pileup.cpp -- pileup_core.hpp (the device code of plo_pileup_*) executed on the host: a pileup object whose kernels are
// emulated waves of 64 lanes (tests/emu/plo_wave.hpp), launched as engine.hip launches them -- the check over all records, then the add;
// the sites as count, the 64-bit scan of records_core.hpp, emit.  The library is built with a small PLO_PILEUP_TILE (tests/emu_pileup_lib.py),
// so that small inputs reach the tile seams.  Every accepted add is repeated on a shadow array by the one-thread form of the rule,
// pileup_add_scalar: the two arrays and the two event counts must agree (status -4 otherwise).
// TEST INFRASTRUCTURE ONLY.  Built as a shared library and, with -DEMU_PILEUP_MAIN, as a program for the AddressSanitizer run: every array,
// the records, every chromosome's bases, the depths and the counters too, sits in a heap block of its exact size.
#include <plo_wave.hpp>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../portello_amd/csrc/pileup_core.hpp"

using namespace plo;

namespace {
template <class T>
T *exact(size_t n) {  // a heap block of exactly n elements (one byte when n == 0: no access to it is in range)
    return (T *)malloc(n ? n * sizeof(T) : 1);
}

struct EmuPileup {
    uint32_t n_ref = 0;
    int32_t *ref_len = nullptr, *slot_beg = nullptr, *slot_end = nullptr;
    uint64_t *slot_off = nullptr;
    unsigned long long n_bases = 0;
    int32_t *arr = nullptr, *shadow = nullptr;
    uint8_t **chrom = nullptr;
    uint32_t exclude = 0;
    PileupSite *sites = nullptr;
    unsigned long long n_sites = 0;
};

void each_wave(unsigned seed, unsigned long long nw, const std::function<void(unsigned long long)> &fn) {
    wv::EmuWave ew;
    ew.order_seed = seed;
    for (unsigned long long k = 0; k < nw; ++k) {
        const unsigned long long w = seed & 1u ? nw - 1 - k : k;
        ew.run([&]() { fn(w); });
    }
}
// nt tiles over a few waves, every wave taking the tiles w, w + nw, ...
void each_tile(unsigned seed, unsigned long long nt, const std::function<void(unsigned long long)> &fn) {
    const unsigned long long nw = nt < 1 + seed % 4 ? nt : 1 + seed % 4;
    each_wave(seed, nw, [&](unsigned long long w) {
        for (unsigned long long t = w; t < nt; t += nw) fn(t);
    });
}
}  // namespace

extern "C" {

unsigned emu_pileup_tile() { return PLO_PILEUP_TILE; }

void emu_pileup_destroy(void *h);

// chrom_cat: the chromosomes' bytes one behind the other; regions: n_regions x (ref_id, beg, end).  -> NULL and *status when refused
void *emu_pileup_create(uint32_t n_ref, const int32_t *ref_len, const uint8_t *chrom_cat, uint32_t exclude, uint32_t n_regions, const int32_t *regions, int *status) {
    EmuPileup *o = new EmuPileup();
    o->n_ref = n_ref;
    o->ref_len = exact<int32_t>(n_ref);
    memcpy(o->ref_len, ref_len, (size_t)n_ref * 4);
    o->slot_beg = exact<int32_t>(n_ref);
    o->slot_end = exact<int32_t>(n_ref);
    o->slot_off = exact<uint64_t>((size_t)n_ref + 1);
    PileupRegion *rg = exact<PileupRegion>(n_regions);
    memcpy(rg, regions, (size_t)n_regions * sizeof(PileupRegion));
    uint32_t which = 0;
    const int bad = pileup_layout(n_ref, o->ref_len, n_regions, rg, o->slot_beg, o->slot_end, o->slot_off, which);
    free(rg);
    if (bad) {
        *status = PLO_ERR_INVALID_ARG;
        emu_pileup_destroy(o);
        return nullptr;
    }
    o->n_bases = o->slot_off[n_ref];
    o->arr = exact<int32_t>((size_t)o->n_bases * PILEUP_CHANNELS);
    o->shadow = exact<int32_t>((size_t)o->n_bases * PILEUP_CHANNELS);
    memset(o->arr, 0, (size_t)o->n_bases * PILEUP_CHANNELS * 4);
    memset(o->shadow, 0, (size_t)o->n_bases * PILEUP_CHANNELS * 4);
    o->chrom = exact<uint8_t *>(n_ref);
    size_t at = 0;
    for (uint32_t r = 0; r < n_ref; ++r) {
        // (a block of the chromosome's exact size; the pieces are cut at the 16-byte lines of the ADDRESSES, so any start is as good)
        o->chrom[r] = exact<uint8_t>((size_t)ref_len[r]);
        memcpy(o->chrom[r], chrom_cat + at, (size_t)ref_len[r]);
        at += (size_t)ref_len[r];
    }
    o->exclude = exclude;
    *status = PLO_OK;
    return o;
}

void emu_pileup_destroy(void *h) {
    EmuPileup *o = (EmuPileup *)h;
    if (o->chrom)
        for (uint32_t r = 0; r < o->n_ref; ++r) free(o->chrom[r]);
    free(o->chrom);
    free(o->ref_len);
    free(o->slot_beg);
    free(o->slot_end);
    free(o->slot_off);
    free(o->arr);
    free(o->shadow);
    free(o->sites);
    delete o;
}

uint64_t emu_pileup_bases(void *h) { return ((EmuPileup *)h)->n_bases; }
void emu_pileup_slots(void *h, uint64_t *slot_off, int32_t *slot_beg, int32_t *slot_end) {
    EmuPileup *o = (EmuPileup *)h;
    memcpy(slot_off, o->slot_off, ((size_t)o->n_ref + 1) * 8);
    memcpy(slot_beg, o->slot_beg, (size_t)o->n_ref * 4);
    memcpy(slot_end, o->slot_end, (size_t)o->n_ref * 4);
}
void emu_pileup_array(void *h, int32_t *out) { memcpy(out, ((EmuPileup *)h)->arr, (size_t)((EmuPileup *)h)->n_bases * PILEUP_CHANNELS * 4); }

int emu_pileup_reset(void *h) {
    EmuPileup *o = (EmuPileup *)h;
    memset(o->arr, 0, (size_t)o->n_bases * PILEUP_CHANNELS * 4);
    memset(o->shadow, 0, (size_t)o->n_bases * PILEUP_CHANNELS * 4);
    free(o->sites);
    o->sites = nullptr;
    o->n_sites = 0;
    return PLO_OK;
}

// the add as engine.hip issues it: k_pileup_check over every record, then k_pileup_add, which reads the check's word first
int emu_pileup_add(void *h, const uint8_t *bytes, uint64_t n_bytes, uint32_t n, const uint64_t *record_off, unsigned order_seed, uint32_t n_waves, uint32_t *n_counted,
                   uint32_t *err_record, uint32_t *err_kind, uint64_t *n_events) {
    EmuPileup *o = (EmuPileup *)h;
    *n_counted = 0;
    *err_record = UINT32_MAX;
    *err_kind = 0;
    *n_events = 0;
    if (!n) return PLO_OK;
    int err = DEPTH_NO_RECORD;
    unsigned counted = 0;
    unsigned long long events = 0, want_events = 0;
    uint64_t *plan = exact<uint64_t>(n);
    memset(plan, 0xA5, (size_t)n * 8);
    DevPileup d;
    memset(&d, 0, sizeof(d));
    d.s.bytes = bytes;
    d.s.n_bytes = n_bytes;
    d.s.n = n;
    d.s.record_off = record_off;
    d.s.n_ref = o->n_ref;
    d.ref_len = o->ref_len;
    d.slot_off = o->slot_off;
    d.slot_beg = o->slot_beg;
    d.slot_end = o->slot_end;
    d.arr = o->arr;
    d.exclude_flags = o->exclude;
    d.chrom_seq = o->chrom;
    d.plan = plan;
    d.err = &err;
    d.n_counted = &counted;
    d.n_events = &events;
    if (!n_waves) n_waves = 1;
    each_wave(order_seed, n_waves, [&](unsigned long long w) { pileup_check_records(d, (uint32_t)w, n_waves); });
    each_wave(order_seed + 2, n_waves, [&](unsigned long long w) { pileup_add_records(d, (uint32_t)w, n_waves); });
    int st = PLO_OK;
    if (err != DEPTH_NO_RECORD) {
        *err_record = (uint32_t)err >> 4;
        *err_kind = (uint32_t)err & 15u;
        st = PLO_ERR_INVALID_ARG;
    } else {
        *n_counted = counted;
        *n_events = events;
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t nc = (uint32_t)plan[i];
            if (!nc) continue;
            const uint8_t *p = bytes + record_off[i];
            const uint32_t ref = index_rd32(p + 4);
            want_events += pileup_add_scalar(p + (plan[i] >> 32), nc, p + 36u + p[12] + 4u * index_rd16(p + 16), (long long)(int)index_rd32(p + 8), o->chrom[ref], o->slot_beg[ref],
                                             o->slot_end[ref], o->shadow + o->slot_off[ref] * PILEUP_CHANNELS);
        }
    }
    if (memcmp(o->arr, o->shadow, (size_t)o->n_bases * PILEUP_CHANNELS * 4) != 0 || events != want_events) st = -4;
    free(plan);
    return st;
}

// depth_cat: the depths of every base, chromosome behind chromosome (put into a depth object's slots here), or NULL; depth_state: 0 an open
// depth object, 1 a finished one, 2 a finished one over another chromosome list.  The sites stay with the object (emu_pileup_sites_copy).
int emu_pileup_sites(void *h, const int32_t *depth_cat, int depth_state, uint32_t mask, int32_t min_count, uint32_t num, uint32_t den, unsigned order_seed, uint64_t *n_sites) {
    EmuPileup *o = (EmuPileup *)h;
    *n_sites = 0;
    if (pileup_sites_refused(min_count, num, den, depth_cat != nullptr, depth_state != 0, depth_state != 2)) return PLO_ERR_INVALID_ARG;
    free(o->sites);
    o->sites = nullptr;
    o->n_sites = 0;
    const unsigned long long nt = (o->n_bases + PILEUP_TILE - 1) / PILEUP_TILE;
    if (!nt) return PLO_OK;
    uint64_t *dslot = exact<uint64_t>((size_t)o->n_ref + 1);
    const unsigned long long dn = depth_layout(o->n_ref, o->ref_len, dslot);
    int32_t *darr = nullptr;
    if (depth_cat) {
        darr = exact<int32_t>((size_t)dn);
        memset(darr, 0, (size_t)dn * 4);
        size_t at = 0;
        for (uint32_t r = 0; r < o->n_ref; ++r) {
            memcpy(darr + dslot[r], depth_cat + at, (size_t)o->ref_len[r] * 4);
            at += (size_t)o->ref_len[r];
        }
    }
    const uint32_t nb = (uint32_t)((nt + REC_SCAN_CHUNK - 1) / REC_SCAN_CHUNK);
    unsigned long long *cnt = exact<unsigned long long>((size_t)nt), *start = exact<unsigned long long>((size_t)nt + 1), *partial = exact<unsigned long long>(nb);
    DevPileupSites d;
    memset(&d, 0, sizeof(d));
    d.arr = o->arr;
    d.slot_off = o->slot_off;
    d.slot_beg = o->slot_beg;
    d.n_ref = o->n_ref;
    d.n_bases = o->n_bases;
    d.depth = darr;
    d.depth_slot_off = dslot;
    d.chrom_seq = o->chrom;
    d.channel_mask = mask;
    d.min_count = min_count;
    d.frac_num = num;
    d.frac_den = den;
    d.cnt = cnt;
    d.start = start;
    each_tile(order_seed, nt, [&](unsigned long long t) { pileup_sites_tile<false>(d, t); });
    each_tile(order_seed, nb, [&](unsigned long long b) { rec_scan_sums(cnt, (uint32_t)nt, (uint32_t)b, partial); });
    each_wave(order_seed, 1, [&](unsigned long long) { rec_scan_partials(partial, nb, start + nt); });
    each_tile(order_seed, nb, [&](unsigned long long b) { rec_scan_apply(cnt, (uint32_t)nt, (uint32_t)b, partial, start); });
    o->n_sites = start[nt];
    o->sites = exact<PileupSite>((size_t)o->n_sites);
    memset(o->sites, 0xA5, (size_t)o->n_sites * sizeof(PileupSite));
    d.site = o->sites;
    each_tile(order_seed, nt, [&](unsigned long long t) { pileup_sites_tile<true>(d, t); });
    free(cnt);
    free(start);
    free(partial);
    free(dslot);
    free(darr);
    *n_sites = o->n_sites;
    return PLO_OK;
}
void emu_pileup_sites_copy(void *h, uint8_t *out) { memcpy(out, ((EmuPileup *)h)->sites, (size_t)((EmuPileup *)h)->n_sites * sizeof(PileupSite)); }

}  // extern "C"

#ifdef EMU_PILEUP_MAIN
// emu_pileup_asan IN OUT.  IN: u32 n_cases, then per case u32 n_ref, exclude, n_regions, n_adds, mask, i32 min_count, u32 num, den, has_depth,
// pad; i32 ref_len[n_ref]; i32 regions[3 n_regions]; the chromosomes' bytes; with has_depth i32 depths[sum ref_len]; and per add u32 n,
// u32 order_seed, u32 n_waves, u32 pad, u64 n_bytes, record_off [n + 1], the bytes.  OUT per case: i32 create status and, when it is 0: per add
// i32 status, u32 err_record, u32 err_kind, u32 n_counted, u64 n_events; then u64 n_bases, the array; i32 sites status, u64 n_sites, the sites.
namespace {
template <class T>
bool rd(FILE *f, T *p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }
}  // namespace
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    FILE *o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    uint32_t n_cases = 0;
    if (!rd(f, &n_cases, 1)) return 2;
    for (uint32_t c = 0; c < n_cases; ++c) {
        uint32_t h[10];
        if (!rd(f, h, 10)) return 2;
        const uint32_t n_ref = h[0], n_regions = h[2];
        int32_t *ref_len = exact<int32_t>(n_ref), *regions = exact<int32_t>((size_t)n_regions * 3);
        if (!rd(f, ref_len, n_ref) || !rd(f, regions, (size_t)n_regions * 3)) return 2;
        size_t total = 0;
        for (uint32_t r = 0; r < n_ref; ++r) total += ref_len[r] > 0 ? (size_t)ref_len[r] : 0;
        uint8_t *chrom = exact<uint8_t>(total);
        int32_t *depth = h[8] ? exact<int32_t>(total) : nullptr;
        if (!rd(f, chrom, total) || (depth && !rd(f, depth, total))) return 2;
        int32_t cst = 0;
        void *d = emu_pileup_create(n_ref, ref_len, chrom, h[1], n_regions, regions, &cst);
        fwrite(&cst, 4, 1, o);
        for (uint32_t a = 0; a < h[3]; ++a) {
            uint32_t g[4];
            uint64_t n_bytes;
            if (!rd(f, g, 4) || !rd(f, &n_bytes, 1)) return 2;
            uint64_t *off = exact<uint64_t>((size_t)g[0] + 1);
            uint8_t *bytes = exact<uint8_t>((size_t)n_bytes);
            if (!rd(f, off, (size_t)g[0] + 1) || !rd(f, bytes, (size_t)n_bytes)) return 2;
            if (d) {
                uint32_t nc = 0, er = 0, ek = 0;
                uint64_t ne = 0;
                const int32_t st = emu_pileup_add(d, bytes, n_bytes, g[0], off, g[1], g[2], &nc, &er, &ek, &ne);
                fwrite(&st, 4, 1, o);
                fwrite(&er, 4, 1, o);
                fwrite(&ek, 4, 1, o);
                fwrite(&nc, 4, 1, o);
                fwrite(&ne, 8, 1, o);
            }
            free(off);
            free(bytes);
        }
        if (d) {
            const uint64_t nb = emu_pileup_bases(d);
            int32_t *arr = exact<int32_t>((size_t)nb * PILEUP_CHANNELS);
            emu_pileup_array(d, arr);
            fwrite(&nb, 8, 1, o);
            fwrite(arr, 4, (size_t)nb * PILEUP_CHANNELS, o);
            free(arr);
            uint64_t n_sites = 0;
            const int32_t sst = emu_pileup_sites(d, depth, 1, h[4], (int32_t)h[5], h[6], h[7], c, &n_sites);
            uint8_t *sites = exact<uint8_t>((size_t)n_sites * sizeof(PileupSite));
            if (sst == PLO_OK) emu_pileup_sites_copy(d, sites);
            fwrite(&sst, 4, 1, o);
            fwrite(&n_sites, 8, 1, o);
            fwrite(sites, sizeof(PileupSite), (size_t)n_sites, o);
            free(sites);
            emu_pileup_destroy(d);
        }
        free(ref_len);
        free(regions);
        free(chrom);
        free(depth);
    }
    fclose(f);
    fclose(o);
    return 0;
}
#endif
