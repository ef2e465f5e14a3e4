// tests/emu/emu_deflate.cpp -- deflate.hpp (the device code of plo_bgzf_compress_dev) executed on the host by an emulated wave
// (tests/emu/plo_wave.hpp).  TEST INFRASTRUCTURE ONLY.  Built as a shared library (tests/emu_deflate_lib.py) and, with -DEMU_DEFLATE_MAIN,
// as a program for the AddressSanitizer run: every payload, output slot and token buffer is a heap block of its exact size there.
#include <plo_wave.hpp>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../portello_amd/csrc/deflate.hpp"

using namespace plo;

namespace {
struct DefEmuWave {
    void gsync() const { wv::sync(); }
    uint32_t load_written(const uint16_t *p) const { return *p; }
};
}  // namespace

// One BGZF block of in[0, n) into out[0, cap) by the 64 lanes of an emulated wave, lanes shuffled when order_seed != 0.
// Returns the encoder's code (every lane must return the same, and the same size: -1000 otherwise).
extern "C" int emu_bgzf_deflate(const uint8_t *in, uint32_t n, uint8_t *out, uint32_t cap, int level, unsigned order_seed, uint32_t *size) {
    uint32_t tab[256];
    for (uint32_t e = 0; e < 256; ++e) tab[e] = crc32_table_entry(e);
    DefWork *ws = (DefWork *)malloc(sizeof(DefWork));
    uint16_t *tok = (uint16_t *)malloc((size_t)DEF_TOK_UNITS * 2);
    memset(ws, 0xC3, sizeof(DefWork));  // (the encoder initialises what it reads)
    int rc_all[64];
    uint32_t sz_all[64];
    wv::EmuWave w;
    w.order_seed = order_seed;
    w.run([&]() {
        DefEmuWave prim;
        uint32_t sz = 0;
        int rc = bgzf_deflate_block(prim, *ws, tab, in, n, out, cap, level, tok, &sz);
        rc_all[wv::lane()] = rc;
        sz_all[wv::lane()] = sz;
    });
    free(ws);
    free(tok);
    for (int l = 1; l < 64; ++l)
        if (rc_all[l] != rc_all[0] || sz_all[l] != sz_all[0]) return -1000;
    *size = sz_all[0];
    return rc_all[0];
}

extern "C" uint32_t emu_bgzf_slot(void) { return DEF_SLOT; }
extern "C" uint32_t emu_bgzf_work_bytes(void) { return (uint32_t)sizeof(DefWork); }

// ---- direct entries: the parts of the encoder that no payload steers freely ---------------------------------------------------------
// def_build_code over freq[0, nsym) with `limit`, run as a wave (lanes shuffled when order_seed != 0): lengths in len[nsym], the codes as
// they enter the stream (bit-reversed) in code[nsym].  freq, len and code are the caller's blocks of exactly nsym elements.
extern "C" int emu_def_build_code(const uint32_t *freq, int nsym, int limit, unsigned order_seed, uint8_t *len, uint16_t *code) {
    if (nsym < 2 || nsym > 288 || limit < 1 || limit > 15) return -1;  // (a code has two symbols at least: the encoder adds one)
    DefWork *ws = (DefWork *)malloc(sizeof(DefWork));
    memset(ws, 0xC3, sizeof(DefWork));
    memset(code, 0, (size_t)nsym * 2);  // (the encoder leaves the code of an unused symbol to its bit reversal, which writes 0)
    wv::EmuWave w;
    w.order_seed = order_seed;
    w.run([&]() {
        DefEmuWave prim;
        def_build_code(prim, *ws, freq, nsym, limit, len, code);
    });
    free(ws);
    return 0;
}

// ncalls wave-wide def_put calls, lane l of call k adding the low nb[64 k + l] bits of v[64 k + l], into out32[0, cap_words) from bit 0 on.
// res[0] = bits written, res[1] = the open word.
extern "C" int emu_def_put(const unsigned long long *v, const uint32_t *nb, uint32_t ncalls, uint32_t *out32, uint32_t cap_words, unsigned order_seed, uint32_t *res) {
    for (uint32_t i = 0; i < ncalls * 64; ++i)
        if (nb[i] > 48 || (nb[i] < 64 && (v[i] >> nb[i]))) return -1;
    DefWork *ws = (DefWork *)malloc(sizeof(DefWork));
    memset(ws, 0xC3, sizeof(DefWork));
    uint32_t bitpos[64], open_word = 0;
    wv::EmuWave w;
    w.order_seed = order_seed;
    w.run([&]() {
        const int lane = wv::lane();
        for (uint32_t k = (uint32_t)lane; k < DEF_OBUF_WORDS; k += 64) ws->obuf[k] = 0;  // as bgzf_deflate_block opens its stream
        wv::sync();
        DefBits st;
        st.out32 = out32;
        st.cap_words = cap_words;
        for (uint32_t k = 0; k < ncalls; ++k) def_put(*ws, st, v[64 * k + (uint32_t)lane], nb[64 * k + (uint32_t)lane]);
        bitpos[lane] = st.bitpos;
        if (lane == 0) open_word = ws->obuf[0];
    });
    free(ws);
    for (int l = 1; l < 64; ++l)
        if (bitpos[l] != bitpos[0]) return -1000;
    res[0] = bitpos[0];
    res[1] = open_word;
    return 0;
}

// the symbol tables: lens[256][3] = code, extra bits, extra value of the lengths 3 .. 258; dists[32768][3] of the distances 1 .. 32768;
// extra[29 + 30] = def_len_extra of the codes 0 .. 28, def_dist_extra of 0 .. 29
extern "C" void emu_def_symbols(uint32_t *lens, uint32_t *dists, uint32_t *extra) {
    for (uint32_t l = 3; l <= 258; ++l) def_len_code(l, lens[3 * (l - 3)], lens[3 * (l - 3) + 1], lens[3 * (l - 3) + 2]);
    for (uint32_t d = 1; d <= 32768; ++d) def_dist_code(d, dists[3 * (d - 1)], dists[3 * (d - 1) + 1], dists[3 * (d - 1) + 2]);
    for (uint32_t c = 0; c < 29; ++c) extra[c] = def_len_extra(c);
    for (uint32_t c = 0; c < 30; ++c) extra[29 + c] = def_dist_extra(c);
}


#ifdef EMU_DEFLATE_MAIN
namespace {
bool read_all(const char *path, std::vector<uint8_t> &all) {
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof(buf), f)) > 0) all.insert(all.end(), buf, buf + k);
    fclose(f);
    return true;
}
// one payload from a heap block of its exact size into slots of exactly 18 + 5 + n + 8 bytes, lane orders 0 and 7; a slot one byte short is refused
int one_payload(const uint8_t *src, uint32_t n, int level, FILE *o, bool prefix) {
    uint8_t *in = (uint8_t *)malloc(n ? n : 1);
    memcpy(in, src, n);
    const uint32_t cap = 18 + 5 + n + 8;
    uint8_t *a = (uint8_t *)malloc(cap), *b = (uint8_t *)malloc(cap);
    uint32_t sa = 0, sb = 0;
    if (emu_bgzf_deflate(in, n, a, cap, level, 0, &sa) != 0 || emu_bgzf_deflate(in, n, b, cap, level, 7, &sb) != 0) return 3;
    if (sa != sb || memcmp(a, b, sa) != 0) return 4;
    uint32_t sc = 0;
    if (emu_bgzf_deflate(in, n, b, cap - 1, level, 0, &sc) != DEF_ERR_SLOT) return 5;
    if (prefix) fwrite(&sa, 4, 1, o);
    fwrite(a, 1, sa, o);
    free(in);
    free(a);
    free(b);
    return 0;
}
// JOBS: records of 32-bit words and their data, every block of a record copied into a heap block of its exact size.
//   1, n, n bytes                                          a payload          -> its BGZF block
//   2, nsym, limit, nsym counts                            def_build_code     -> nsym lengths, nsym 16-bit codes
//   3, ncalls, cap_words, 64 ncalls x u64, 64 ncalls x u32 def_put calls      -> cap_words words, bits written, the open word
// OUT: for every record the length of its result in bytes, then the result.
int run_jobs(const std::vector<uint8_t> &all, int level, FILE *o) {
    size_t at = 0;
    auto word = [&](uint32_t &w) {
        if (at + 4 > all.size()) return false;
        memcpy(&w, all.data() + at, 4);
        at += 4;
        return true;
    };
    uint32_t kind;
    while (word(kind)) {
        if (kind == 1) {
            uint32_t n;
            if (!word(n) || at + n > all.size()) return 6;
            const int rc = one_payload(all.data() + at, n, level, o, true);
            if (rc) return rc;
            at += n;
        } else if (kind == 2) {
            uint32_t nsym, limit;
            if (!word(nsym) || !word(limit) || at + 4 * (size_t)nsym > all.size()) return 6;
            uint32_t *freq = (uint32_t *)malloc(4 * (size_t)nsym);
            memcpy(freq, all.data() + at, 4 * (size_t)nsym);
            at += 4 * (size_t)nsym;
            uint8_t *len = (uint8_t *)malloc(nsym);
            uint16_t *code = (uint16_t *)malloc(2 * (size_t)nsym);
            if (emu_def_build_code(freq, (int)nsym, (int)limit, 7, len, code) != 0) return 7;
            const uint32_t sz = 3 * nsym;
            fwrite(&sz, 4, 1, o);
            fwrite(len, 1, nsym, o);
            fwrite(code, 2, nsym, o);
            free(freq);
            free(len);
            free(code);
        } else if (kind == 3) {
            uint32_t ncalls, cap_words;
            if (!word(ncalls) || !word(cap_words) || at + 12 * 64 * (size_t)ncalls > all.size()) return 6;
            unsigned long long *v = (unsigned long long *)malloc(8 * 64 * (size_t)ncalls);
            uint32_t *nb = (uint32_t *)malloc(4 * 64 * (size_t)ncalls);
            memcpy(v, all.data() + at, 8 * 64 * (size_t)ncalls);
            memcpy(nb, all.data() + at + 8 * 64 * (size_t)ncalls, 4 * 64 * (size_t)ncalls);
            at += 12 * 64 * (size_t)ncalls;
            uint32_t *out32 = (uint32_t *)calloc(cap_words ? cap_words : 1, 4), res[2] = {0, 0};
            if (emu_def_put(v, nb, ncalls, out32, cap_words, 7, res) != 0) return 8;
            const uint32_t sz = 4 * cap_words + 8;
            fwrite(&sz, 4, 1, o);
            fwrite(out32, 4, cap_words, o);
            fwrite(res, 4, 2, o);
            free(v);
            free(nb);
            free(out32);
        } else {
            return 6;
        }
    }
    return at == all.size() ? 0 : 6;
}
}  // namespace

// emu_deflate_asan IN OUT LEVEL: IN is cut into 0xff00-byte payloads; every one is compressed twice (lane orders 0 and 7) from a heap block
// of its exact size into a slot of exactly 18 + 5 + len + 8 bytes; OUT receives the blocks.
// emu_deflate_asan --jobs JOBS OUT LEVEL: the records of JOBS (run_jobs above).
int main(int argc, char **argv) {
    const bool jobs = argc == 5 && strcmp(argv[1], "--jobs") == 0;
    if (argc != 4 && !jobs) return 2;
    if (jobs) ++argv;
    std::vector<uint8_t> all;
    if (!read_all(argv[1], all)) return 2;
    const int level = atoi(argv[3]);
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    if (jobs) {
        const int rc = run_jobs(all, level, o);
        fclose(o);
        return rc;
    }
    for (size_t at = 0; at < all.size() || at == 0; at += DEF_MAX_IN) {
        const uint32_t n = (uint32_t)(all.size() - at < DEF_MAX_IN ? all.size() - at : DEF_MAX_IN);
        const int rc = one_payload(all.data() + at, n, level, o, false);
        if (rc) return rc;
        if (all.empty()) break;
    }
    fclose(o);
    return 0;
}
#endif
