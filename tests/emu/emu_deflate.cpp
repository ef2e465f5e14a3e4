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

#ifdef EMU_DEFLATE_MAIN
// emu_deflate_asan IN OUT LEVEL: IN is cut into 0xff00-byte payloads; every one is compressed twice (lane orders 0 and 7) from a heap block
// of its exact size into a slot of exactly 18 + 5 + len + 8 bytes; OUT receives the blocks.
int main(int argc, char **argv) {
    if (argc != 4) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<uint8_t> all;
    uint8_t buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof(buf), f)) > 0) all.insert(all.end(), buf, buf + k);
    fclose(f);
    const int level = atoi(argv[3]);
    FILE *o = fopen(argv[2], "wb");
    if (!o) return 2;
    for (size_t at = 0; at < all.size() || at == 0; at += DEF_MAX_IN) {
        const uint32_t n = (uint32_t)(all.size() - at < DEF_MAX_IN ? all.size() - at : DEF_MAX_IN);
        uint8_t *in = (uint8_t *)malloc(n ? n : 1);
        memcpy(in, all.data() + at, n);
        const uint32_t cap = 18 + 5 + n + 8;
        uint8_t *a = (uint8_t *)malloc(cap), *b = (uint8_t *)malloc(cap);
        uint32_t sa = 0, sb = 0;
        if (emu_bgzf_deflate(in, n, a, cap, level, 0, &sa) != 0 || emu_bgzf_deflate(in, n, b, cap, level, 7, &sb) != 0) return 3;
        if (sa != sb || memcmp(a, b, sa) != 0) return 4;
        uint32_t sc = 0;
        if (emu_bgzf_deflate(in, n, b, cap - 1, level, 0, &sc) != DEF_ERR_SLOT) return 5;  // a slot one byte short is refused
        fwrite(a, 1, sa, o);
        free(in);
        free(a);
        free(b);
        if (all.empty()) break;
    }
    fclose(o);
    return 0;
}
#endif
