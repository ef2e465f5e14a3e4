// tests/emu/emu_inflate.hpp -- the device's DEFLATE decoder (inflate.hpp) executed on the host: serially, and by the 64 lanes of an emulated
// wave.  Shared by the emulator library (emu_harness.cpp) and the sanitizer program (emu_inflate.cpp).  TEST INFRASTRUCTURE ONLY.
// Include behind plo_wave.hpp.
#pragma once
#include "../../portello_amd/csrc/inflate.hpp"

extern "C" int emu_inflate(const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t out_len, uint32_t *written) {
    plo::InfWork ws;
    plo::InfSerial io;
    return plo::inflate_block(io, in, in_len, out, out_len, ws, written);
}
namespace {
struct InfEmuWave {
    int lane() const { return wv::lane(); }
    void sync() const { wv::sync(); }
    uint32_t uniform(uint32_t v) const { return (uint32_t)wv::bcast_first((int)v); }
    uint32_t scalar(uint32_t v) const { return v; }
    uint32_t read_lane(uint32_t v, uint32_t l) const { return (uint32_t)wv::shfl((int)v, (int)(l & 63)); }
    int popcount64(unsigned long long v) const { return __builtin_popcountll(v); }
    uint32_t rank_below(unsigned long long mask) const { return (uint32_t)__builtin_popcountll(mask & ((1ull << wv::lane()) - 1ull)); }
    uint8_t load_written(const uint8_t *p) const { return *p; }
};
}  // namespace
extern "C" int emu_inflate_wave(const uint8_t *in, uint32_t in_len, uint8_t *out, uint32_t out_len, uint32_t *written, unsigned order_seed) {
    plo::InfWork ws;
    plo::InfWaveMem mem;  // the wave's LDS windows
    int rc_all[64];
    uint32_t w_all[64];
    wv::EmuWave w;
    w.order_seed = order_seed;
    w.run([&]() {
        uint32_t wr = 0;
        plo::InfWaveIO<InfEmuWave> io;  // per lane, like the registers of the device code
        io.m = &mem;
        int rc = plo::inflate_block(io, in, in_len, out, out_len, ws, &wr);
        rc_all[wv::lane()] = rc;
        w_all[wv::lane()] = wr;
    });
    for (int l = 1; l < 64; ++l)
        if (rc_all[l] != rc_all[0] || (rc_all[0] == 0 && w_all[l] != w_all[0])) return -1000;  // the lanes must agree
    *written = w_all[0];
    return rc_all[0];
}
