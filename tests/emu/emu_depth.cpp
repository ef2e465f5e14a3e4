// tests/emu/emu_depth.cpp -- depth_core.hpp (the device code of plo_depth_*) executed on the host: a depth object whose kernels are emulated
// waves of 64 lanes (tests/emu/plo_wave.hpp), launched as engine.hip launches them -- the check over all records, then the add; the five
// launches of the finish; windows; runs (count, the 64-bit scan of records_core.hpp, emit).  The library is built with a small
// PLO_DEPTH_TILE (tests/emu_depth_lib.py), so that small inputs reach the tile seams of every level.  Every accepted add is repeated on a
// shadow array by the one-thread form of the rule, depth_add_scalar: the two arrays must agree (status -4 otherwise).
// TEST INFRASTRUCTURE ONLY.  Built as a shared library and, with -DEMU_DEPTH_MAIN, as a program for the AddressSanitizer run: every array,
// the records and the depth array too, sits in a heap block of its exact size.
#include <plo_wave.hpp>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../portello_amd/csrc/depth_core.hpp"

using namespace plo;

namespace {
template <class T>
T *exact(size_t n) {  // a heap block of exactly n elements (one byte when n == 0: no access to it is in range)
    return (T *)malloc(n ? n * sizeof(T) : 1);
}

struct EmuDepth {
    uint32_t n_ref = 0;
    int32_t *ref_len = nullptr;
    uint64_t *slot_off = nullptr;
    unsigned long long n_entries = 0;
    int32_t *arr = nullptr, *shadow = nullptr;
    uint32_t exclude = 0;
    int count_del = 0;
    bool finished = false;
    DepthRun *runs = nullptr;
    unsigned long long n_runs = 0;
};

void each_wave(unsigned seed, unsigned long long nw, const std::function<void(unsigned long long)> &fn) {
    wv::EmuWave ew;
    ew.order_seed = seed;
    for (unsigned long long k = 0; k < nw; ++k) {
        const unsigned long long w = seed & 1u ? nw - 1 - k : k;
        ew.run([&]() { fn(w); });
    }
}
// nt tiles over a few waves, every wave taking the tiles w, w + nw, ... (a launch of the device gives every tile a wave of its own; the
// result cannot depend on that, and starting an emulated wave costs far more than a tile)
void each_tile(unsigned seed, unsigned long long nt, const std::function<void(unsigned long long)> &fn) {
    const unsigned long long nw = nt < 1 + seed % 4 ? nt : 1 + seed % 4;
    each_wave(seed, nw, [&](unsigned long long w) {
        for (unsigned long long t = w; t < nt; t += nw) fn(t);
    });
}
unsigned long long tiles(unsigned long long n) { return (n + DEPTH_TILE - 1) / DEPTH_TILE; }
}  // namespace

extern "C" {

unsigned emu_depth_tile() { return PLO_DEPTH_TILE; }

void *emu_depth_create(uint32_t n_ref, const int32_t *ref_len, uint32_t exclude, int count_del) {
    EmuDepth *o = new EmuDepth();
    o->n_ref = n_ref;
    o->ref_len = exact<int32_t>(n_ref);
    memcpy(o->ref_len, ref_len, (size_t)n_ref * 4);
    o->slot_off = exact<uint64_t>((size_t)n_ref + 1);
    o->n_entries = depth_layout(n_ref, o->ref_len, o->slot_off);
    o->arr = exact<int32_t>((size_t)o->n_entries);
    o->shadow = exact<int32_t>((size_t)o->n_entries);
    memset(o->arr, 0, (size_t)o->n_entries * 4);
    memset(o->shadow, 0, (size_t)o->n_entries * 4);
    o->exclude = exclude;
    o->count_del = count_del;
    return o;
}

void emu_depth_destroy(void *h) {
    EmuDepth *o = (EmuDepth *)h;
    free(o->ref_len);
    free(o->slot_off);
    free(o->arr);
    free(o->shadow);
    free(o->runs);
    delete o;
}

uint64_t emu_depth_entries(void *h) { return ((EmuDepth *)h)->n_entries; }
void emu_depth_slots(void *h, uint64_t *slot_off) { memcpy(slot_off, ((EmuDepth *)h)->slot_off, ((size_t)((EmuDepth *)h)->n_ref + 1) * 8); }
void emu_depth_array(void *h, int32_t *out) { memcpy(out, ((EmuDepth *)h)->arr, (size_t)((EmuDepth *)h)->n_entries * 4); }

int emu_depth_reset(void *h) {
    EmuDepth *o = (EmuDepth *)h;
    memset(o->arr, 0, (size_t)o->n_entries * 4);
    memset(o->shadow, 0, (size_t)o->n_entries * 4);
    o->finished = false;
    return PLO_OK;
}

// the add as engine.hip issues it: k_depth_check over every record, then k_depth_add, which reads the check's word first
int emu_depth_add(void *h, const uint8_t *bytes, uint64_t n_bytes, uint32_t n, const uint64_t *record_off, unsigned order_seed, uint32_t n_waves, uint32_t *n_counted,
                  uint32_t *err_record, uint32_t *err_kind) {
    EmuDepth *o = (EmuDepth *)h;
    *n_counted = 0;
    *err_record = UINT32_MAX;
    *err_kind = 0;
    if (!depth_call_allowed(o->finished, DEPTH_CALL_ADD)) return PLO_ERR_INVALID_ARG;
    if (!n) return PLO_OK;
    int err = DEPTH_NO_RECORD;
    unsigned counted = 0;
    uint64_t *plan = exact<uint64_t>(n);
    memset(plan, 0xA5, (size_t)n * 8);
    DevDepth d;
    memset(&d, 0, sizeof(d));
    d.s.bytes = bytes;
    d.s.n_bytes = n_bytes;
    d.s.n = n;
    d.s.record_off = record_off;
    d.s.n_ref = o->n_ref;
    d.ref_len = o->ref_len;
    d.slot_off = o->slot_off;
    d.arr = o->arr;
    d.exclude_flags = o->exclude;
    d.count_del = o->count_del;
    d.plan = plan;
    d.err = &err;
    d.n_counted = &counted;
    if (!n_waves) n_waves = 1;
    each_wave(order_seed, n_waves, [&](unsigned long long w) { depth_check_records(d, (uint32_t)w, n_waves); });
    each_wave(order_seed + 2, n_waves, [&](unsigned long long w) { depth_add_records(d, (uint32_t)w, n_waves); });
    int st = PLO_OK;
    if (err != DEPTH_NO_RECORD) {
        *err_record = (uint32_t)err >> 4;
        *err_kind = (uint32_t)err & 15u;
        st = PLO_ERR_INVALID_ARG;
    } else {
        *n_counted = counted;
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t nc = (uint32_t)plan[i];
            if (!nc) continue;
            const uint8_t *p = bytes + record_off[i];
            depth_add_scalar(p + (plan[i] >> 32), nc, (long long)(int)index_rd32(p + 8), o->count_del != 0, o->shadow + o->slot_off[index_rd32(p + 4)]);
        }
    }
    if (memcmp(o->arr, o->shadow, (size_t)o->n_entries * 4) != 0) st = -4;
    free(plan);
    return st;
}

// the five launches of plo_depth_finish_dev
int emu_depth_finish(void *h, unsigned order_seed) {
    EmuDepth *o = (EmuDepth *)h;
    if (!depth_call_allowed(o->finished, DEPTH_CALL_FINISH)) return PLO_ERR_INVALID_ARG;
    const unsigned long long n0 = o->n_entries, n1 = tiles(n0), n2 = tiles(n1);
    int32_t *s1 = exact<int32_t>((size_t)n1), *s2 = exact<int32_t>((size_t)n2);
    each_tile(order_seed, n1, [&](unsigned long long t) { depth_tile_sum(o->arr, n0, t, s1); });
    each_tile(order_seed, n2, [&](unsigned long long t) { depth_tile_sum(s1, n1, t, s2); });
    if (n2) each_wave(order_seed, 1, [&](unsigned long long) { depth_top_scan(s2, n2); });
    each_tile(order_seed, n2, [&](unsigned long long t) { depth_tile_scan(s1, n1, t, s2); });
    each_tile(order_seed, n1, [&](unsigned long long t) { depth_tile_scan(o->arr, n0, t, s1); });
    free(s1);
    free(s2);
    o->finished = true;
    return PLO_OK;
}

uint64_t emu_depth_n_windows(void *h, uint32_t w) {
    EmuDepth *o = (EmuDepth *)h;
    std::vector<uint64_t> first((size_t)o->n_ref + 1);
    return w ? depth_win_layout(o->n_ref, o->ref_len, w, first.data()) : 0;
}

// sum: exactly emu_depth_n_windows(w) values; win_first: n_ref + 1
int emu_depth_windows(void *h, uint32_t w, unsigned order_seed, uint32_t n_waves, uint64_t *sum, uint64_t *win_first) {
    EmuDepth *o = (EmuDepth *)h;
    if (!w || !depth_call_allowed(o->finished, DEPTH_CALL_WINDOWS)) return PLO_ERR_INVALID_ARG;
    DevDepthWin d;
    memset(&d, 0, sizeof(d));
    d.arr = o->arr;
    d.ref_len = o->ref_len;
    d.slot_off = o->slot_off;
    d.win_first = win_first;
    d.n_ref = o->n_ref;
    d.w = w;
    d.n_win = depth_win_layout(o->n_ref, o->ref_len, w, win_first);
    d.sum = sum;
    if (!n_waves) n_waves = 1;
    if (d.n_win) each_wave(order_seed, n_waves, [&](unsigned long long k) { depth_windows(d, k, n_waves); });
    return PLO_OK;
}

// count, the 64-bit scan, emit; the runs stay with the object until the next call (emu_depth_runs_copy)
int emu_depth_runs(void *h, unsigned order_seed, uint64_t *n_runs) {
    EmuDepth *o = (EmuDepth *)h;
    *n_runs = 0;
    if (!depth_call_allowed(o->finished, DEPTH_CALL_RUNS)) return PLO_ERR_INVALID_ARG;
    free(o->runs);
    o->runs = nullptr;
    o->n_runs = 0;
    const unsigned long long nt = tiles(o->n_entries);
    if (!nt) return PLO_OK;
    const uint32_t nb = (uint32_t)((nt + REC_SCAN_CHUNK - 1) / REC_SCAN_CHUNK);
    unsigned long long *cnt = exact<unsigned long long>((size_t)nt), *start = exact<unsigned long long>((size_t)nt + 1), *partial = exact<unsigned long long>(nb);
    DevDepthRuns d;
    memset(&d, 0, sizeof(d));
    d.arr = o->arr;
    d.ref_len = o->ref_len;
    d.slot_off = o->slot_off;
    d.n_ref = o->n_ref;
    d.n_entries = o->n_entries;
    d.cnt = cnt;
    d.start = start;
    each_tile(order_seed, nt, [&](unsigned long long t) { depth_runs_tile<false>(d, t); });
    each_tile(order_seed, nb, [&](unsigned long long b) { rec_scan_sums(cnt, (uint32_t)nt, (uint32_t)b, partial); });
    each_wave(order_seed, 1, [&](unsigned long long) { rec_scan_partials(partial, nb, start + nt); });
    each_tile(order_seed, nb, [&](unsigned long long b) { rec_scan_apply(cnt, (uint32_t)nt, (uint32_t)b, partial, start); });
    o->n_runs = start[nt];
    o->runs = exact<DepthRun>((size_t)o->n_runs);
    memset(o->runs, 0xA5, (size_t)o->n_runs * sizeof(DepthRun));
    d.run = o->runs;
    each_tile(order_seed, nt, [&](unsigned long long t) { depth_runs_tile<true>(d, t); });
    free(cnt);
    free(start);
    free(partial);
    *n_runs = o->n_runs;
    return PLO_OK;
}
void emu_depth_runs_copy(void *h, uint8_t *out) { memcpy(out, ((EmuDepth *)h)->runs, (size_t)((EmuDepth *)h)->n_runs * sizeof(DepthRun)); }

}  // extern "C"

#ifdef EMU_DEPTH_MAIN
// emu_depth_asan IN OUT.  IN: u32 n_cases, then per case u32 n_ref, u32 exclude, u32 count_del, u32 w, u32 n_adds, i32 ref_len[n_ref], and per
// add u32 n, u32 order_seed, u32 n_waves, u32 pad, u64 n_bytes, record_off [n + 1], the bytes.  OUT per case: per add i32 status, u32 err_record,
// u32 err_kind, u32 n_counted; then u64 n_entries, the difference array; the depth array behind the finish; u64 n_win, win_first [n_ref + 1],
// the sums; u64 n_runs, the runs.
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
        uint32_t h[5];
        if (!rd(f, h, 5)) return 2;
        const uint32_t n_ref = h[0], w = h[3];
        int32_t *ref_len = exact<int32_t>(n_ref);
        if (!rd(f, ref_len, n_ref)) return 2;
        void *d = emu_depth_create(n_ref, ref_len, h[1], (int)h[2]);
        for (uint32_t a = 0; a < h[4]; ++a) {
            uint32_t g[4];
            uint64_t n_bytes;
            if (!rd(f, g, 4) || !rd(f, &n_bytes, 1)) return 2;
            uint64_t *off = exact<uint64_t>((size_t)g[0] + 1);
            uint8_t *bytes = exact<uint8_t>((size_t)n_bytes);
            if (!rd(f, off, (size_t)g[0] + 1) || !rd(f, bytes, (size_t)n_bytes)) return 2;
            uint32_t nc = 0, er = 0, ek = 0;
            const int32_t st = emu_depth_add(d, bytes, n_bytes, g[0], off, g[1], g[2], &nc, &er, &ek);
            fwrite(&st, 4, 1, o);
            fwrite(&er, 4, 1, o);
            fwrite(&ek, 4, 1, o);
            fwrite(&nc, 4, 1, o);
            free(off);
            free(bytes);
        }
        const uint64_t ne = emu_depth_entries(d);
        int32_t *arr = exact<int32_t>((size_t)ne);
        fwrite(&ne, 8, 1, o);
        emu_depth_array(d, arr);
        fwrite(arr, 4, (size_t)ne, o);
        if (emu_depth_finish(d, c) != PLO_OK) return 3;
        emu_depth_array(d, arr);
        fwrite(arr, 4, (size_t)ne, o);
        free(arr);
        const uint64_t n_win = emu_depth_n_windows(d, w);
        uint64_t *sum = exact<uint64_t>((size_t)n_win), *first = exact<uint64_t>((size_t)n_ref + 1);
        if (emu_depth_windows(d, w, c, 3, sum, first) != PLO_OK) return 3;
        fwrite(&n_win, 8, 1, o);
        fwrite(first, 8, (size_t)n_ref + 1, o);
        fwrite(sum, 8, (size_t)n_win, o);
        free(sum);
        free(first);
        uint64_t n_runs = 0;
        if (emu_depth_runs(d, c, &n_runs) != PLO_OK) return 3;
        uint8_t *runs = exact<uint8_t>((size_t)n_runs * 16);
        emu_depth_runs_copy(d, runs);
        fwrite(&n_runs, 8, 1, o);
        fwrite(runs, 16, (size_t)n_runs, o);
        free(runs);
        free(ref_len);
        emu_depth_destroy(d);
    }
    fclose(f);
    fclose(o);
    return 0;
}
#endif
