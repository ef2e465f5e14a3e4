// tests/emu/emu_cut.cpp -- window_core.hpp (the device code of plo_window_cut_dev) executed on the host: the guess, the walks, the resolve
// pass, the scans, the find and the emit passes by emulated waves (tests/emu/plo_wave.hpp), with segments of any size; and the host-only
// header walk of plo_bgzf_inflate_dev (bgzf_walk.hpp).
// TEST INFRASTRUCTURE ONLY.  Built as a shared library (tests/emu_cut_lib.py) and, with -DEMU_CUT_MAIN, as a program for the
// AddressSanitizer + UBSan run: the stream sits in a heap block of its exact size there, so a read outside it is caught.
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
    // outputs: blocks of the exact size
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
// a kernel with a lane per segment
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

// plo_window_cut_dev's steps with host pointers and segments of `seg_bytes`; no_guess != 0: every guess is "none" (the result must not
// change).  The arrays of `out` live until emu_cut_free / the next call; out->n_rewalks counts the segments the resolve pass walked again.
extern "C" int emu_window_cut(const plo_window_cut_in *in, unsigned long long seg_bytes, unsigned order_seed, int no_guess, plo_window_cut_out *out) {
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
    // a fill no result can be mistaken for
    memset(s->rec_off, 0xEE, (nr ? nr : 1) * 8);
    memset(s->unm_off, 0xEE, (nu + 1) * 8);
    memset(s->unm, 0xEE, ub ? ub : 1);
    d.n_unmapped = nu;
    d.unmapped_bytes = ub;
    lanes(ns, order_seed, [&](uint32_t g) { cut_emit_segment(d, g); });
    if (nu)  // (one wave strides over the records as a workgroup of k_cut_copy does)
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

extern "C" void emu_cut_free(void) {
    delete g_cut;
    g_cut = nullptr;
}

// bgzf_walk over b[0, n): -> its return code; blk[6 * i ..] = off, coff, clen, uoff, ulen, crc of block i (the first cap_blocks of them)
extern "C" int emu_bgzf_walk(const uint8_t *b, unsigned long long n, unsigned long long cap, unsigned long long *consumed, unsigned long long *n_bytes, uint32_t *n_blocks,
                             unsigned long long *blk, uint32_t cap_blocks) {
    std::vector<BgzfWalkBlk> v;
    uint64_t c = 0, u = 0;
    const int rc = bgzf_walk(b, (size_t)n, cap, v, &c, &u);
    *consumed = c;
    *n_bytes = u;
    *n_blocks = (uint32_t)v.size();
    for (uint32_t i = 0; i < v.size() && i < cap_blocks; ++i) {
        const unsigned long long f[6] = {v[i].off, v[i].coff, v[i].clen, v[i].uoff, v[i].ulen, v[i].crc};
        memcpy(blk + 6 * (size_t)i, f, sizeof(f));
    }
    return rc;
}

#ifdef EMU_CUT_MAIN
// emu_cut_asan IN OUT.  IN: u64 stream_bytes, u64 seg_bytes, u64 max_unmapped, u64 max_bytes, u32 max_records, u32 final, the stream.
// OUT: u32 status, ended_by, n_reads, n_unmapped, u64 window_bytes, err_off, unmapped_bytes, n_rewalks, then (status 0) read_rec_off,
// unmapped_off[n_unmapped + 1], the unmapped bytes
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    uint64_t h[4];
    uint32_t g[2];
    if (fread(h, 8, 4, f) != 4 || fread(g, 4, 2, f) != 2) return 2;
    uint8_t *stream = (uint8_t *)malloc(h[0] ? h[0] : 1);  // exact size
    if (h[0] && fread(stream, 1, h[0], f) != h[0]) return 2;
    fclose(f);
    plo_window_cut_in in;
    memset(&in, 0, sizeof(in));
    in.stream = stream;
    in.stream_bytes = h[0];
    in.max_records = g[0];
    in.max_unmapped = h[2];
    in.max_bytes = h[3];
    in.final = (int32_t)g[1];
    plo_window_cut_out out;
    const int st = emu_window_cut(&in, h[1], 3u, 0, &out);
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    const uint32_t head[4] = {(uint32_t)st, (uint32_t)out.ended_by, out.n_reads, out.n_unmapped};
    const uint64_t head2[4] = {out.window_bytes, out.err_off, out.unmapped_bytes, out.n_rewalks};
    fwrite(head, 4, 4, o);
    fwrite(head2, 8, 4, o);
    if (st == PLO_OK) {
        fwrite(out.read_rec_off, 8, out.n_reads, o);
        fwrite(out.unmapped_off, 8, (size_t)out.n_unmapped + 1, o);
        fwrite(out.unmapped, 1, out.unmapped_bytes, o);
    }
    fclose(o);
    emu_cut_free();
    free(stream);
    return 0;
}
#endif
