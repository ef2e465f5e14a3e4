// tests/emu/emu_index.cpp -- index_core.hpp (the device code of plo_records_index_dev) executed on the host: every record by an emulated
// wave of 64 lanes (tests/emu/plo_wave.hpp), the records strided over n_waves waves as k_index strides them over its grid (the result does
// not depend on the number of waves, so the tests choose small ones).  Every accepted record is also given to the one-thread form of the
// rule, index_entry_scalar, which the host's merge uses: the two must agree.
// TEST INFRASTRUCTURE ONLY.  Built as a shared library (tests/emu_index_lib.py) and, with -DEMU_INDEX_MAIN, as a program for the
// AddressSanitizer run: every array, the records and the entries too, sits in a heap block of its exact size there.
#include <plo_wave.hpp>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../portello_amd/csrc/index_core.hpp"

using namespace plo;

namespace {
template <class T>
T *exact(size_t n) {  // a heap block of exactly n elements (one byte when n == 0: no access to it is in range)
    return (T *)malloc(n ? n * sizeof(T) : 1);
}

// the call as engine.hip issues it -> PLO_OK, PLO_ERR_INVALID_ARG, or -4 when the wave's entry of a record and the one-thread rule's differ
int run_index(const uint8_t *bytes, uint64_t n_bytes, uint32_t n, const uint64_t *record_off, uint32_t n_ref, unsigned order_seed, uint32_t n_waves, IndexEntry *entry,
              uint32_t *n_placed, uint32_t *err_record, uint32_t *err_kind) {
    *n_placed = 0;
    *err_record = UINT32_MAX;
    *err_kind = 0;
    if (!n) return PLO_OK;
    memset(entry, 0xA5, (size_t)n * sizeof(IndexEntry));
    int err = INDEX_NO_RECORD;
    unsigned placed = 0;
    DevBai d;
    memset(&d, 0, sizeof(d));
    d.s.bytes = bytes;
    d.s.n_bytes = n_bytes;
    d.s.n = n;
    d.s.record_off = record_off;
    d.s.n_ref = n_ref;
    d.entry = entry;
    d.err = &err;
    d.n_placed = &placed;
    if (!n_waves) n_waves = 1;
    wv::EmuWave ew;
    ew.order_seed = order_seed;
    for (uint32_t k = 0; k < n_waves; ++k) {
        const uint32_t w = order_seed & 1u ? n_waves - 1 - k : k;
        ew.run([&]() { index_records(d, w, n_waves); });
    }
    if (err != INDEX_NO_RECORD) {
        *err_record = (uint32_t)err >> 4;
        *err_kind = (uint32_t)err & 15u;
        return PLO_ERR_INVALID_ARG;
    }
    *n_placed = placed;
    for (uint32_t i = 0; i < n; ++i) {
        IndexEntry e;
        memset(&e, 0, sizeof(e));
        if (index_entry_scalar(bytes + record_off[i], record_off[i + 1] - record_off[i], record_off[i], e) != 0 || memcmp(&e, &entry[i], sizeof(e)) != 0) return -4;
    }
    return PLO_OK;
}
}  // namespace

extern "C" int emu_index(const uint8_t *bytes, uint64_t n_bytes, uint32_t n, const uint64_t *record_off, uint32_t n_ref, unsigned order_seed, uint32_t n_waves,
                         uint8_t *entry, uint32_t *n_placed, uint32_t *err_record, uint32_t *err_kind) {
    return run_index(bytes, n_bytes, n, record_off, n_ref, order_seed, n_waves, (IndexEntry *)entry, n_placed, err_record, err_kind);
}

#ifdef EMU_INDEX_MAIN
// emu_index_asan IN OUT.  IN: u32 n_cases, then per case u32 n, u32 n_ref, u32 order_seed, u32 n_waves, u64 n_bytes, record_off [n + 1], the
// bytes.  Every array goes into a heap block of its exact size.  OUT per case: i32 status, u32 err_record, u32 err_kind, u32 n_placed, and
// for status 0 the entries [n].
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    FILE *o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    uint32_t n_cases = 0;
    if (fread(&n_cases, 4, 1, f) != 1) return 2;
    for (uint32_t k = 0; k < n_cases; ++k) {
        uint32_t h[4];
        uint64_t n_bytes;
        if (fread(h, 4, 4, f) != 4 || fread(&n_bytes, 8, 1, f) != 1) return 2;
        const uint32_t n = h[0];
        uint64_t *off = exact<uint64_t>((size_t)n + 1);
        uint8_t *bytes = exact<uint8_t>((size_t)n_bytes);
        if (fread(off, 8, (size_t)n + 1, f) != (size_t)n + 1 || (n_bytes && fread(bytes, 1, (size_t)n_bytes, f) != n_bytes)) return 2;
        IndexEntry *entry = exact<IndexEntry>(n);
        uint32_t np = 0, er = 0, ek = 0;
        const int32_t st = run_index(bytes, n_bytes, n, off, h[1], h[2], h[3], entry, &np, &er, &ek);
        fwrite(&st, 4, 1, o);
        fwrite(&er, 4, 1, o);
        fwrite(&ek, 4, 1, o);
        fwrite(&np, 4, 1, o);
        if (st == 0 && n) fwrite(entry, sizeof(IndexEntry), n, o);
        free(off);
        free(bytes);
        free(entry);
    }
    fclose(f);
    fclose(o);
    return 0;
}
#endif
