// tests/emu/emu_sort.cpp -- sort_core.hpp (the device code of plo_records_sort_dev) executed on the host: the tile sort by an emulated
// workgroup of four waves (tests/emu/plo_wave.hpp), the 64-bit scan of records_core.hpp by emulated waves, the merge, gather and copy
// functions (no wave primitives) by plain loops over their threads.
// TEST INFRASTRUCTURE ONLY.  Built as a shared library (tests/emu_sort_lib.py) and, with -DEMU_SORT_MAIN, as a program for the
// AddressSanitizer run: every array, the records and the output too, sits in a heap block of its exact size there.
// The copy is watched store by store: the output starts as the complement of the expected bytes, and after every thread of every chunk
// the bytes that now hold the expected value are counted and set back.  Every byte must be counted exactly once.
#include <plo_wave.hpp>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../portello_amd/csrc/sort_core.hpp"

using namespace plo;

namespace {
constexpr uint8_t SORT_CANARY = 0xA5;

template <class T>
T *exact(size_t n) {  // a heap block of exactly n elements (one byte when n == 0: no access to it is in range)
    return (T *)malloc(n ? n * sizeof(T) : 1);
}

struct SortResult {
    uint32_t n = 0;
    unsigned long long *key[2] = {nullptr, nullptr}, *len = nullptr, *slen = nullptr, *off = nullptr;
    uint32_t *idx[2] = {nullptr, nullptr};
    uint8_t *block = nullptr;  // guard + n_bytes + guard
    size_t guard = 0;
    int cur = 0;  // which of key / idx holds the result
    int status = PLO_OK, check = 0;  // check 2: a store outside the output or far from its chunk, 3: a byte not stored exactly once
    uint32_t err_record = UINT32_MAX, err_kind = 0, n_mapped = 0;
    std::vector<uint8_t> out;
    ~SortResult() {
        for (int i = 0; i < 2; ++i) {
            free(key[i]);
            free(idx[i]);
        }
        free(len);
        free(slen);
        free(off);
        free(block);
    }
};

void scan64(const unsigned long long *in, uint32_t n, unsigned long long *out, unsigned order_seed) {
    const uint32_t nb = (n + REC_SCAN_CHUNK - 1) / REC_SCAN_CHUNK;
    unsigned long long *partial = exact<unsigned long long>(nb);
    wv::EmuWave ew;
    ew.order_seed = order_seed;
    for (uint32_t w = 0; w < nb; ++w) ew.run([&]() { rec_scan_sums(in, n, w, partial); });
    ew.run([&]() { rec_scan_partials(partial, nb, out + n); });
    for (uint32_t w = 0; w < nb; ++w) ew.run([&]() { rec_scan_apply(in, n, w, partial, out); });
    free(partial);
}

// the call as engine.hip issues it.  expect: the n_bytes the output must hold (not looked at for a refused input)
void run_sort(const uint8_t *bytes, uint64_t n_bytes, uint32_t n, const uint64_t *record_off, uint32_t n_ref, unsigned order_seed, size_t guard, const uint8_t *expect,
              SortResult &r) {
    r.n = n;
    if (!n) return;
    for (int i = 0; i < 2; ++i) {
        r.key[i] = exact<unsigned long long>(n);
        r.idx[i] = exact<uint32_t>(n);
    }
    r.len = exact<unsigned long long>(n);
    r.slen = exact<unsigned long long>(n);
    r.off = exact<unsigned long long>((size_t)n + 1);
    int err = SORT_NO_RECORD;
    unsigned n_mapped = 0;
    DevSort d;
    memset(&d, 0, sizeof(d));
    d.bytes = bytes;
    d.n_bytes = n_bytes;
    d.n = n;
    d.record_off = record_off;
    d.n_ref = n_ref;
    for (int i = 0; i < 2; ++i) {
        d.key[i] = r.key[i];
        d.idx[i] = r.idx[i];
    }
    d.len = r.len;
    d.slen = r.slen;
    d.new_off = r.off;
    d.err = &err;
    d.n_mapped = &n_mapped;
    {
        unsigned long long *lk = exact<unsigned long long>(SORT_TILE);
        uint32_t *li = exact<uint32_t>(SORT_TILE);
        wv::EmuWave ew;
        ew.nw = SORT_THREADS / 64;
        ew.order_seed = order_seed;
        const uint32_t n_tiles = (n + SORT_TILE - 1) / SORT_TILE;
        for (uint32_t k = 0; k < n_tiles; ++k) {
            const uint32_t t = order_seed & 1u ? n_tiles - 1 - k : k;
            ew.run([&]() { sort_tile(d, t, lk, li); });
        }
        free(lk);
        free(li);
    }
    int cur = 0;
    for (uint64_t run = SORT_TILE; run < n; run <<= 1, cur ^= 1)
        for (uint32_t k = 0; k < n; ++k) sort_merge_pair(d.key[cur], d.idx[cur], d.key[cur ^ 1], d.idx[cur ^ 1], n, (uint32_t)run, order_seed & 1u ? n - 1 - k : k);
    r.cur = cur;
    const uint32_t *perm = d.idx[cur];
    for (uint32_t j = 0; j < n; ++j) d.slen[j] = d.len[perm[j]];
    scan64(d.slen, n, r.off, order_seed);
    if (err != SORT_NO_RECORD) {  // k_sort_copy's gate: a refused window moves no byte
        r.status = PLO_ERR_INVALID_ARG;
        r.err_record = (uint32_t)err;
        r.err_kind = (uint32_t)r.len[err];
        return;
    }
    r.n_mapped = n_mapped;
    r.guard = guard;
    r.block = exact<uint8_t>(guard + (size_t)n_bytes + guard);
    memset(r.block, SORT_CANARY, guard + (size_t)n_bytes + guard);
    uint8_t *o = r.block + guard;
    for (size_t k = 0; k < n_bytes; ++k) o[k] = (uint8_t)~expect[k];
    d.out = o;
    std::vector<uint8_t> cnt((size_t)n_bytes, 0);
    const unsigned long long n_chunks = (n_bytes + SORT_COPY_CHUNK - 1) / SORT_COPY_CHUNK;
    for (unsigned long long c0 = 0; c0 < n_chunks; ++c0) {
        const unsigned long long c = order_seed & 1u ? n_chunks - 1 - c0 : c0;
        const size_t lo = (size_t)(c * SORT_COPY_CHUNK), hi = (size_t)std::min<unsigned long long>(n_bytes, lo + SORT_COPY_CHUNK);
        const size_t w0 = lo > 256 ? lo - 256 : 0, w1 = std::min<size_t>((size_t)n_bytes, hi + 256);
        for (int tid = 0; tid < 64; ++tid) {
            sort_copy_chunk(d, perm, c, tid, 64);
            for (size_t k = w0; k < w1; ++k)
                if (o[k] == expect[k]) {
                    if (k < lo || k >= hi) r.check = 2;
                    if (cnt[k] < 255) ++cnt[k];
                    o[k] = (uint8_t)~expect[k];
                }
        }
    }
    for (size_t k = 0; k < guard; ++k)
        if (r.block[k] != SORT_CANARY || r.block[guard + n_bytes + k] != SORT_CANARY) r.check = 2;
    r.out.resize((size_t)n_bytes);
    for (size_t k = 0; k < n_bytes; ++k) {
        if (o[k] != (uint8_t)~expect[k]) r.check = 2;  // a wrong value, or a store far from its chunk
        else if (cnt[k] != 1 && !r.check) r.check = 3;
        r.out[k] = cnt[k] ? expect[k] : o[k];
    }
}

int finish(const SortResult &r, uint64_t n_bytes, uint8_t *out_bytes, uint64_t *out_off, uint32_t *perm, uint64_t *key, uint32_t *n_mapped, uint32_t *err_record,
           uint32_t *err_kind) {
    *err_record = r.err_record;
    *err_kind = r.err_kind;
    *n_mapped = r.n_mapped;
    if (r.status != PLO_OK) return r.status;
    if (!r.n) {
        out_off[0] = 0;
        return PLO_OK;
    }
    memcpy(perm, r.idx[r.cur], (size_t)r.n * 4);
    memcpy(key, r.key[r.cur], (size_t)r.n * 8);
    memcpy(out_off, r.off, ((size_t)r.n + 1) * 8);
    if (n_bytes) memcpy(out_bytes, r.out.data(), (size_t)n_bytes);
    return r.check ? -r.check : PLO_OK;
}
}  // namespace

// -> PLO_OK, PLO_ERR_INVALID_ARG (*err_record the lowest offending record, *err_kind its SORT_ERR_*), or -2 / -3 when the copy stored
// outside the output (or far from the storing chunk) / did not store every byte exactly once.  The output lies between 64 canary bytes.
extern "C" int emu_sort(const uint8_t *bytes, uint64_t n_bytes, uint32_t n, const uint64_t *record_off, uint32_t n_ref, unsigned order_seed, const uint8_t *expect,
                        uint8_t *out_bytes, uint64_t *out_off, uint32_t *perm, uint64_t *key, uint32_t *n_mapped, uint32_t *err_record, uint32_t *err_kind) {
    SortResult r;
    run_sort(bytes, n_bytes, n, record_off, n_ref, order_seed, 64, expect, r);
    return finish(r, n_bytes, out_bytes, out_off, perm, key, n_mapped, err_record, err_kind);
}
extern "C" uint32_t emu_sort_tile(void) { return SORT_TILE; }

#ifdef EMU_SORT_MAIN
// emu_sort_asan IN OUT.  IN: u32 n_cases, then per case u32 n, u32 n_ref, u32 order_seed, u32 has_expect, u64 n_bytes, record_off [n + 1],
// the bytes, the expected bytes (has_expect).  Every array goes into a heap block of its exact size, the output too (no guard bytes).
// OUT per case: i32 status, u32 err_record, u32 err_kind, u32 n_mapped, and for status 0: perm [n], key [n], record_off [n + 1], bytes.
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
        uint8_t *bytes = exact<uint8_t>((size_t)n_bytes), *expect = exact<uint8_t>(h[3] ? (size_t)n_bytes : 0);
        if (fread(off, 8, (size_t)n + 1, f) != (size_t)n + 1 || (n_bytes && fread(bytes, 1, (size_t)n_bytes, f) != n_bytes) ||
            (h[3] && n_bytes && fread(expect, 1, (size_t)n_bytes, f) != n_bytes))
            return 2;
        SortResult r;
        run_sort(bytes, n_bytes, n, off, h[1], h[2], 0, expect, r);
        uint8_t *ob = exact<uint8_t>((size_t)n_bytes);
        uint64_t *oo = exact<uint64_t>((size_t)n + 1), *ok = exact<uint64_t>(n);
        uint32_t *op = exact<uint32_t>(n), nm = 0, er = 0, ek = 0;
        const int32_t st = finish(r, n_bytes, ob, oo, op, ok, &nm, &er, &ek);
        fwrite(&st, 4, 1, o);
        fwrite(&er, 4, 1, o);
        fwrite(&ek, 4, 1, o);
        fwrite(&nm, 4, 1, o);
        if (st == 0) {
            fwrite(op, 4, n, o);
            fwrite(ok, 8, n, o);
            fwrite(oo, 8, (size_t)n + 1, o);
            if (n_bytes) fwrite(ob, 1, (size_t)n_bytes, o);
        }
        free(off);
        free(bytes);
        free(expect);
        free(ob);
        free(oo);
        free(ok);
        free(op);
    }
    fclose(f);
    fclose(o);
    return 0;
}
#endif
