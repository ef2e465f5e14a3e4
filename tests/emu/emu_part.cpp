// tests/emu/emu_part.cpp -- the device code of API 11 executed on the host: part_start_tile (plo_part_start_dev) by the emulated waves of a
// workgroup that take tiles of candidates by ticket, in ascending or in shuffled order; the window cut with the range test
// (plo_window_cut_part_dev: emu_cut.cpp's steps with DevCut::own_bytes set); and the host-only header walk with own_bytes
// (plo_bgzf_inflate_part_dev, bgzf_walk.hpp).
// TEST INFRASTRUCTURE ONLY.  Built as a shared library (tests/emu_part_lib.py) and, with -DEMU_PART_MAIN, as a program for the
// AddressSanitizer + UBSan run: every stream sits in a heap block of its exact size there, so a read outside it is caught.
#include <plo_wave.hpp>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../portello_amd/csrc/bgzf_walk.hpp"
#include "../../portello_amd/csrc/window_core.hpp"

using namespace plo;

namespace {
struct CutState {
    std::vector<unsigned long long> guess, land, cnt, start, partial, fire, res;
    uint64_t *rec_off = nullptr, *unm_off = nullptr, *unm_src = nullptr;
    uint8_t *unm = nullptr;
    ~CutState() {
        free(rec_off);
        free(unm_off);
        free(unm_src);
        free(unm);
    }
};
CutState *g_cut = nullptr;

template <class T>
T *exact(size_t n) {
    return (T *)malloc((n ? n : 1) * sizeof(T));
}
template <class F>
void wave(unsigned order_seed, F f) {
    wv::EmuWave ew;
    ew.order_seed = order_seed;
    ew.run(f);
}
template <class F>
void lanes(uint32_t ns, unsigned order_seed, F f) {
    for (uint32_t w = 0; w < (ns + 63) / 64; ++w)
        wave(order_seed, [&]() {
            const uint32_t s = w * 64 + (uint32_t)wv::lane();
            if (s < ns) f(s);
        });
}
void scan64(const unsigned long long *in, uint32_t n, unsigned long long *out, std::vector<unsigned long long> &partial, unsigned order_seed) {
    const uint32_t nb = n ? (n + REC_SCAN_CHUNK - 1) / REC_SCAN_CHUNK : 1;
    partial.assign(nb, 0);
    for (uint32_t w = 0; w < nb; ++w) wave(order_seed, [&]() { rec_scan_sums(in, n, w, partial.data()); });
    wave(order_seed, [&]() { rec_scan_partials(partial.data(), nb, out + n); });
    for (uint32_t w = 0; w < nb; ++w) wave(order_seed, [&]() { rec_scan_apply(in, n, w, partial.data(), out); });
}
}  // namespace

// plo_part_start_dev's kernel with host pointers and tiles of `tile` candidates (a multiple of 64), by the two waves of one emulated
// workgroup that draw tickets.  tile_seed == 0: the kernel as it stands -- ticket t is tile t, and a wave leaves at the first tile that
// part_start_tile reports as lying above a find.  tile_seed != 0: ticket t is tile perm[t] of a shuffled order and no wave leaves early, so
// tiles above and below the result run in any order and each decides for itself what it skips: the result must be the same.
extern "C" int emu_part_start(const plo_part_start_in *in, unsigned long long tile, unsigned order_seed, unsigned tile_seed, plo_part_start_out *out) {
    memset(out, 0, sizeof(*out));
    out->kind = PLO_PART_NONE;
    out->first_off = UINT64_MAX;
    if (!tile || tile % 64) return PLO_ERR_INVALID_ARG;
    if (in->stream_bytes < 36) return PLO_OK;
    unsigned long long res[PS_WORDS] = {CUT_NONE, CUT_NONE, 0, 0};
    DevPart d;
    memset(&d, 0, sizeof(d));
    d.stream = in->stream;
    d.n = in->stream_bytes;
    d.n_cand = d.n - 35;
    d.tile = tile;
    d.n_tiles = (d.n_cand + tile - 1) / tile;
    d.n_ref = in->n_ref;
    d.final = in->final ? 1 : 0;
    d.res = res;
    std::vector<unsigned long long> perm(d.n_tiles);
    for (unsigned long long t = 0; t < d.n_tiles; ++t) perm[t] = t;
    unsigned rs = tile_seed;
    for (unsigned long long i = d.n_tiles; tile_seed && i > 1; --i) {
        rs = rs * 1664525u + 1013904223u;
        std::swap(perm[i - 1], perm[(rs >> 8) % i]);
    }
    wv::EmuWave ew;
    ew.nw = 2;
    ew.order_seed = order_seed;
    ew.run([&]() {
        for (;;) {
            unsigned long long t = 0;
            if (wv::lane() == 0) t = wv::atomic_add_global(d.res + PS_TICKET, 1ull);
            t = wv::bcast_first(t);
            if (t >= d.n_tiles) return;
            if (!part_start_tile(d, perm[t]) && !tile_seed) return;
        }
    });
    const unsigned long long acc = res[PS_ACCEPT], cut = res[PS_CUT];
    if ((acc != CUT_NONE && acc >= d.n_cand) || (cut != CUT_NONE && cut >= d.n_cand)) return PLO_ERR_INTERNAL;
    if (acc < cut) {
        out->kind = PLO_PART_FOUND;
        out->first_off = acc;
    } else if (cut != CUT_NONE) {
        out->kind = PLO_PART_NEED_MORE;
    }
    return PLO_OK;
}

// plo_window_cut_part_dev's steps with host pointers and segments of `seg_bytes` (emu_cut.cpp's emu_window_cut with the range test)
extern "C" int emu_window_cut_part(const plo_window_cut_part_in *in, unsigned long long seg_bytes, unsigned order_seed, int no_guess, plo_window_cut_out *out) {
    memset(out, 0, sizeof(*out));
    out->err_off = UINT64_MAX;
    if (!in->max_records || seg_bytes < 64) return PLO_ERR_INVALID_ARG;
    delete g_cut;
    CutState *s = g_cut = new CutState();
    const unsigned long long n = in->stream_bytes;
    const uint32_t ns = (uint32_t)(n / seg_bytes + 1);
    s->guess.assign(ns, 0xEEEEEEEEEEEEEEEEull);
    s->land.assign(ns, 0xEEEEEEEEEEEEEEEEull);
    s->cnt.assign(3 * (size_t)ns, 0xEEEEEEEEEEEEEEEEull);
    s->start.assign(3 * ((size_t)ns + 1), 0);
    s->fire.assign(5 * (size_t)ns, 0xEEEEEEEEEEEEEEEEull);
    s->res.assign(CR_WORDS, 0);
    DevCut d;
    memset(&d, 0, sizeof(d));
    d.stream = in->stream;
    d.n = n;
    d.seg_bytes = seg_bytes;
    d.n_seg = ns;
    d.max_records = in->max_records;
    d.max_unmapped = in->max_unmapped ? in->max_unmapped : 4ull * in->max_records + 1024;
    d.max_bytes = in->max_bytes ? in->max_bytes : std::max<unsigned long long>(1ull << 30, std::min<unsigned long long>(8ull << 30, (unsigned long long)in->max_records << 16));
    d.final = in->final ? 1 : 0;
    d.ranged = in->own_bytes != UINT64_MAX;
    d.own_bytes = in->own_bytes;
    d.guess = s->guess.data();
    d.land = s->land.data();
    d.cnt = s->cnt.data();
    d.start = s->start.data();
    d.fire = s->fire.data();
    d.res = s->res.data();
    s->guess[0] = 0;
    for (uint32_t g = 1; g < ns; ++g) {
        if (no_guess) s->guess[g] = CUT_NONE;
        else wave(order_seed, [&]() { cut_guess_segment(d, g); });
    }
    lanes(ns, order_seed, [&](uint32_t g) { (void)cut_walk_segment(d, g, d.guess[g], true); });
    wave(order_seed, [&]() { cut_resolve(d); });
    for (int y = 0; y < 3; ++y) scan64(s->cnt.data() + (size_t)y * ns, ns, s->start.data() + (size_t)y * ((size_t)ns + 1), s->partial, order_seed);
    lanes(ns, order_seed, [&](uint32_t g) { cut_find_segment(d, g); });
    cut_result(d);
    const unsigned long long at = s->res[CR_AT], why = s->res[CR_WHY];
    out->n_rewalks = (uint32_t)s->res[CR_REWALKS];
    if (at > n || why == CUT_NONE) return PLO_ERR_INTERNAL;
    if (why >= CUT_WHY_ERR_TRUNC) {
        out->err_off = at;
        return why == CUT_WHY_ERR_UNM_TID ? PLO_ERR_DATA : PLO_ERR_IO;
    }
    const unsigned long long nr = s->res[CR_READS], nu = s->res[CR_UNMAPPED], ub = s->res[CR_UNM_BYTES];
    d.cut_at = at;
    d.read_rec_off = s->rec_off = exact<uint64_t>(nr);
    d.unm_off = s->unm_off = exact<uint64_t>(nu + 1);
    d.unm_src = s->unm_src = exact<uint64_t>(nu);
    d.unmapped = s->unm = exact<uint8_t>(ub);
    memset(s->rec_off, 0xEE, (nr ? nr : 1) * 8);
    memset(s->unm_off, 0xEE, (nu + 1) * 8);
    memset(s->unm, 0xEE, ub ? ub : 1);
    d.n_unmapped = nu;
    d.unmapped_bytes = ub;
    lanes(ns, order_seed, [&](uint32_t g) { cut_emit_segment(d, g); });
    if (nu)
        wave(order_seed, [&]() {
            for (unsigned long long u = 0; u < nu; ++u) cut_copy_unmapped(d, u, wv::lane(), 64);
        });
    out->n_reads = (uint32_t)nr;
    out->read_rec_off = s->rec_off;
    out->n_unmapped = (uint32_t)nu;
    out->unmapped_off = s->unm_off;
    out->unmapped = s->unm;
    out->unmapped_bytes = ub;
    out->window_bytes = at;
    out->ended_by = (int32_t)why;
    return PLO_OK;
}

extern "C" void emu_part_free(void) {
    delete g_cut;
    g_cut = nullptr;
}

// bgzf_walk over b[0, n), which lies at file_off of a file whose part ends at range_end: -> its return code
extern "C" int emu_bgzf_walk_part(const uint8_t *b, unsigned long long n, unsigned long long cap, unsigned long long file_off, unsigned long long range_end,
                                  unsigned long long *consumed, unsigned long long *n_bytes, unsigned long long *own_bytes, uint32_t *n_blocks) {
    std::vector<BgzfWalkBlk> v;
    uint64_t c = 0, u = 0, own = 0;
    const int rc = bgzf_walk(b, (size_t)n, cap, v, &c, &u, file_off, range_end, &own);
    *consumed = c;
    *n_bytes = u;
    *own_bytes = own;
    *n_blocks = (uint32_t)v.size();
    return rc;
}

#ifdef EMU_PART_MAIN
// emu_part_asan IN OUT.  IN: u32 n_cases, then per case u32 mode and
//   mode 0 (part start): u64 stream_bytes, u64 tile, u32 n_ref, u32 final, u32 order_seed, u32 tile_seed, the stream
//                        -> OUT: u32 status, u32 kind, u64 first_off
//   mode 1 (cut):        u64 stream_bytes, u64 seg_bytes, u64 max_unmapped, u64 max_bytes, u64 own_bytes, u32 max_records, u32 final, the stream
//                        -> OUT: u32 status, ended_by, n_reads, n_unmapped, u64 window_bytes, err_off, unmapped_bytes, then (status 0)
//                           read_rec_off, the unmapped bytes
static bool rd(FILE *f, void *p, size_t n) { return fread(p, 1, n, f) == n; }
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    uint32_t n_cases = 0;
    if (!rd(f, &n_cases, 4)) return 2;
    for (uint32_t k = 0; k < n_cases; ++k) {
        uint32_t mode = 0;
        if (!rd(f, &mode, 4)) return 2;
        if (mode == 0) {
            uint64_t h[2];
            uint32_t g[4];
            if (!rd(f, h, 16) || !rd(f, g, 16)) return 2;
            uint8_t *stream = (uint8_t *)malloc(h[0] ? h[0] : 1);  // exact size
            if (!rd(f, stream, h[0])) return 2;
            plo_part_start_in in;
            memset(&in, 0, sizeof(in));
            in.stream = stream;
            in.stream_bytes = h[0];
            in.n_ref = g[0];
            in.final = (int32_t)g[1];
            plo_part_start_out out;
            const int st = emu_part_start(&in, h[1], g[2], g[3], &out);
            const uint32_t head[2] = {(uint32_t)st, (uint32_t)out.kind};
            fwrite(head, 4, 2, o);
            fwrite(&out.first_off, 8, 1, o);
            free(stream);
        } else {
            uint64_t h[5];
            uint32_t g[2];
            if (!rd(f, h, 40) || !rd(f, g, 8)) return 2;
            uint8_t *stream = (uint8_t *)malloc(h[0] ? h[0] : 1);
            if (!rd(f, stream, h[0])) return 2;
            plo_window_cut_part_in in;
            memset(&in, 0, sizeof(in));
            in.stream = stream;
            in.stream_bytes = h[0];
            in.max_records = g[0];
            in.max_unmapped = h[2];
            in.max_bytes = h[3];
            in.final = (int32_t)g[1];
            in.own_bytes = h[4];
            plo_window_cut_out out;
            const int st = emu_window_cut_part(&in, h[1], 3u, 0, &out);
            const uint32_t head[4] = {(uint32_t)st, (uint32_t)out.ended_by, out.n_reads, out.n_unmapped};
            const uint64_t head2[3] = {out.window_bytes, out.err_off, out.unmapped_bytes};
            fwrite(head, 4, 4, o);
            fwrite(head2, 8, 3, o);
            if (st == PLO_OK) {
                fwrite(out.read_rec_off, 8, out.n_reads, o);
                fwrite(out.unmapped, 1, out.unmapped_bytes, o);
            }
            emu_part_free();
            free(stream);
        }
    }
    fclose(f);
    fclose(o);
    return 0;
}
#endif
