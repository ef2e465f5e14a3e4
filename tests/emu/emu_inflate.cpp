// tests/emu/emu_inflate.cpp -- inflate.hpp (the device code of k_bgzf_inflate) as a program for the AddressSanitizer + UBSan run
// (tests/emu_inflate_lib.py).  TEST INFRASTRUCTURE ONLY.
//   emu_inflate_asan IN OUT
// IN:  u32 n, then n cases of {u32 in_len, u32 cap, u32 wave, in_len bytes}
// OUT: per case the serial decode {i32 rc, u32 written, written bytes} and, where wave != 0, the same of the 64-lane decode (lane order
//      shuffled with seed `wave`)
// Every input and every output is a heap block of its exact size -- in_len is not rounded up to the words and windows the decoder loads --
// so that a read or write one byte outside [in, in + in_len) / [out, out + cap) ends the program.
#include <plo_wave.hpp>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "emu_inflate.hpp"

static bool rd32(FILE *f, uint32_t *v) { return fread(v, 4, 1, f) == 1; }

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    FILE *o = f ? fopen(argv[2], "wb") : nullptr;
    if (!f || !o) return 2;
    uint32_t n = 0;
    if (!rd32(f, &n)) return 2;
    for (uint32_t c = 0; c < n; ++c) {
        uint32_t in_len = 0, cap = 0, wave = 0;
        if (!rd32(f, &in_len) || !rd32(f, &cap) || !rd32(f, &wave)) return 2;
        uint8_t *in = (uint8_t *)malloc(in_len);  // (a block of no bytes is still a block of its own: any access is outside it)
        if (in_len && fread(in, 1, in_len, f) != in_len) return 2;
        for (int mode = 0; mode < (wave ? 2 : 1); ++mode) {
            uint8_t *out = (uint8_t *)malloc(cap);
            memset(out, 0xEE, cap);
            uint32_t written = 0;
            const int32_t rc = mode ? emu_inflate_wave(in, in_len, out, cap, &written, wave) : emu_inflate(in, in_len, out, cap, &written);
            if (rc != 0) written = 0;
            if (written > cap) return 3;
            fwrite(&rc, 4, 1, o);
            fwrite(&written, 4, 1, o);
            if (written) fwrite(out, 1, written, o);
            free(out);
        }
        free(in);
    }
    fclose(f);
    return fclose(o) == 0 ? 0 : 2;
}
