// tests/emu/emu_merge.cpp -- merge_core.hpp (the device code of plo_runs_merge_plan_dev / plo_runs_merge_emit_dev) executed on the host, the
// two calls issued as engine.hip issues them, its host-side refusals included: the 64-bit scan of records_core.hpp by emulated waves
// (tests/emu/plo_wave.hpp), the key, rank, gather, chunk, copy and rebase functions (no wave primitives) by plain loops over their threads.
// TEST INFRASTRUCTURE ONLY.  Built as a shared library (tests/emu_merge_lib.py) and, with -DEMU_MERGE_MAIN, as a program for the
// AddressSanitizer run.  Both take one blob of cases and give one blob of results (formats below); every array -- each run's bytes and
// offsets, the workspace, every chunk's output -- sits in a heap block of its exact size.
// Every emit is watched store by store: the chunk's output lies between canary bytes and starts as the complement of the expected bytes,
// and after every thread of every piece the bytes that now hold the expected value are counted and set back.  Every byte must be counted
// exactly once.
#include <plo_wave.hpp>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../portello_amd/csrc/merge_core.hpp"

using namespace plo;

namespace {
constexpr uint8_t MERGE_CANARY = 0xA5;
enum { ST_OK = 0, ST_INVALID_ARG = 1, ST_RANGE = 5, ST_INTERNAL = 6 };  // plo_status

template <class T>
T *exact(size_t n) {  // a heap block of exactly n elements (one byte when n == 0: no access to it is in range)
    return (T *)malloc(n ? n * sizeof(T) : 1);
}

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

struct PlanOut {
    int status = ST_OK;
    uint32_t n = 0, n_mapped = 0, n_chunks = 0, err_run = UINT32_MAX, err_record = UINT32_MAX, err_kind = 0;
    unsigned long long n_bytes = 0;
};

struct ChunkOut {
    int status = ST_OK, check = 0;  // check 2: a store outside the output or far from its piece, 3: a byte not stored exactly once
    uint32_t n = 0, first = 0;
    std::vector<unsigned long long> off;
    std::vector<uint8_t> bytes;
};

// the context's side of the two calls
struct EmuCtx {
    bool have_plan = false;
    uint32_t n = 0, n_runs = 0, n_chunks = 0;
    int cur = 0;
    MergeRun *runs = nullptr;
    uint32_t *run_first = nullptr;
    unsigned long long *key[2] = {nullptr, nullptr}, *len = nullptr, *mlen = nullptr, *off = nullptr, *chunk_off = nullptr;
    uint32_t *src[2] = {nullptr, nullptr}, *chunk_first = nullptr;
    uint16_t *run_of = nullptr;
    void drop() {
        for (int i = 0; i < 2; ++i) {
            free(key[i]);
            free(src[i]);
            key[i] = nullptr;
            src[i] = nullptr;
        }
        free(runs);
        free(run_first);
        free(len);
        free(mlen);
        free(off);
        free(chunk_off);
        free(chunk_first);
        free(run_of);
        runs = nullptr;
        run_first = chunk_first = nullptr;
        len = mlen = off = chunk_off = nullptr;
        run_of = nullptr;
        have_plan = false;
    }
    ~EmuCtx() { drop(); }

    void plan(const MergeRun *in_runs, uint32_t in_n_runs, uint32_t n_ref, unsigned long long chunk_bytes, unsigned order_seed, PlanOut &o) {
        drop();
        if (in_n_runs > MERGE_MAX_RUNS || chunk_bytes == 0 || (in_n_runs && !in_runs) || n_ref > 0x7fffffffu) {
            o.status = ST_INVALID_ARG;
            return;
        }
        unsigned long long n64 = 0, n_bytes = 0;
        for (uint32_t r = 0; r < in_n_runs; ++r) {
            if (in_runs[r].n_records ? (!in_runs[r].bytes || !in_runs[r].record_off) : in_runs[r].n_bytes != 0) {
                o.status = ST_INVALID_ARG;
                return;
            }
            n64 += in_runs[r].n_records;
            n_bytes += in_runs[r].n_bytes;
        }
        if (n64 > 0xfffffffeull) {
            o.status = ST_RANGE;
            return;
        }
        n = (uint32_t)n64;
        n_runs = in_n_runs;
        n_chunks = 0;
        cur = 0;
        off = exact<unsigned long long>((size_t)n + 1);
        if (!n) {
            off[0] = 0;
            have_plan = true;
            return;
        }
        const uint32_t cap = (uint32_t)std::min<unsigned long long>(n, 2 * (n_bytes / chunk_bytes) + 2);
        runs = exact<MergeRun>(n_runs);
        memcpy(runs, in_runs, (size_t)n_runs * sizeof(MergeRun));
        run_first = exact<uint32_t>((size_t)n_runs + 1);
        run_first[0] = 0;
        for (uint32_t r = 0; r < n_runs; ++r) run_first[r + 1] = run_first[r] + runs[r].n_records;
        for (int i = 0; i < 2; ++i) {
            key[i] = exact<unsigned long long>(n);
            src[i] = exact<uint32_t>(n);
        }
        len = exact<unsigned long long>(n);
        mlen = exact<unsigned long long>(n);
        run_of = exact<uint16_t>(n);
        chunk_first = exact<uint32_t>((size_t)cap + 1);
        chunk_off = exact<unsigned long long>((size_t)cap + 1);
        int err = merge_err_word(MERGE_NO_RECORD);
        uint32_t res[2] = {0, 0};
        DevMerge d;
        memset(&d, 0, sizeof(d));
        d.runs = runs;
        d.run_first = run_first;
        d.n_runs = n_runs;
        d.n = n;
        d.n_ref = n_ref;
        d.chunk_bytes = chunk_bytes;
        for (int i = 0; i < 2; ++i) {
            d.key[i] = key[i];
            d.src[i] = src[i];
        }
        d.run_of = run_of;
        d.len = len;
        d.mlen = mlen;
        d.off = off;
        d.err = &err;
        d.res = res;
        d.chunk_first = chunk_first;
        d.chunk_off = chunk_off;
        d.chunk_cap = cap;
        const bool back = (order_seed & 1u) != 0;
        for (uint32_t k = 0; k < n; ++k) merge_key_record(d, back ? n - 1 - k : k);
        for (uint32_t t = 0; (1u << t) < n_runs; ++t, cur ^= 1)
            for (uint32_t k = 0; k < n; ++k) merge_rank_pair(d, key[cur], src[cur], key[cur ^ 1], src[cur ^ 1], t, back ? n - 1 - k : k);
        for (uint32_t j = 0; j < n; ++j) merge_gather(d, src[cur], j);
        scan64(mlen, n, off, order_seed);
        merge_chunks(d, key[cur]);
        if (err != merge_err_word(MERGE_NO_RECORD)) {
            const uint32_t g = (uint32_t)err ^ 0x80000000u;
            uint32_t r = 0;
            while (r + 1 < n_runs && run_first[r + 1] <= g) ++r;
            o.status = ST_INVALID_ARG;
            o.err_run = r;
            o.err_record = g - run_first[r];
            o.err_kind = (uint32_t)len[g];
            return;
        }
        if (res[1] == 0 || res[1] > cap) {
            o.status = ST_INTERNAL;
            return;
        }
        n_chunks = res[1];
        have_plan = true;
        o.n = n;
        o.n_mapped = res[0];
        o.n_chunks = n_chunks;
        o.n_bytes = chunk_off[n_chunks];
    }

    // expect: the merged stream's bytes (the chunk's stand at chunk_off[chunk])
    void emit(uint32_t chunk, unsigned order_seed, size_t guard, const uint8_t *expect, size_t expect_len, ChunkOut &o) {
        if (!have_plan || chunk >= n_chunks) {
            o.status = ST_INVALID_ARG;
            return;
        }
        const uint32_t first = chunk_first[chunk], nrec = chunk_first[chunk + 1] - first;
        const size_t nbytes = (size_t)(chunk_off[chunk + 1] - chunk_off[chunk]);
        if (chunk_off[chunk + 1] > expect_len) {  // (the plan disagrees with the expectation: the caller's comparison shows where)
            o.status = -4;
            return;
        }
        const uint8_t *want = expect + chunk_off[chunk];
        uint8_t *block = exact<uint8_t>(guard + nbytes + guard);
        memset(block, MERGE_CANARY, guard + nbytes + guard);
        uint8_t *out = block + guard;
        for (size_t k = 0; k < nbytes; ++k) out[k] = (uint8_t)~want[k];
        unsigned long long *ooff = exact<unsigned long long>((size_t)nrec + 1);
        DevMergeEmit d;
        memset(&d, 0, sizeof(d));
        d.runs = runs;
        d.run_first = run_first;
        d.run_of = run_of;
        d.src = src[cur];
        d.off = off;
        d.first = first;
        d.n = nrec;
        d.out = out;
        d.out_off = ooff;
        std::vector<uint8_t> cnt(nbytes, 0);
        const unsigned long long n_pieces = (nbytes + MERGE_COPY_PIECE - 1) / MERGE_COPY_PIECE, nw = ((n_pieces + 3) / 4) * 4;
        for (unsigned long long p0 = 0; p0 < nw; ++p0) {
            const unsigned long long p = order_seed & 1u ? nw - 1 - p0 : p0;
            const size_t lo = (size_t)std::min<unsigned long long>(nbytes, p * MERGE_COPY_PIECE), hi = (size_t)std::min<unsigned long long>(nbytes, lo + MERGE_COPY_PIECE);
            const size_t w0 = lo > 256 ? lo - 256 : 0, w1 = std::min<size_t>(nbytes, hi + 256);
            for (int tid = 0; tid < 64; ++tid) {
                if (p < n_pieces) merge_copy_piece(d, p, tid, 64);
                merge_rebase(d, p * 64u + (unsigned long long)tid, nw * 64u);
                for (size_t k = w0; k < w1; ++k)
                    if (out[k] == want[k]) {
                        if (k < lo || k >= hi) o.check = 2;
                        if (cnt[k] < 255) ++cnt[k];
                        out[k] = (uint8_t)~want[k];
                    }
            }
        }
        for (size_t k = 0; k < guard; ++k)
            if (block[k] != MERGE_CANARY || block[guard + nbytes + k] != MERGE_CANARY) o.check = 2;
        o.bytes.resize(nbytes);
        for (size_t k = 0; k < nbytes; ++k) {
            if (out[k] != (uint8_t)~want[k]) o.check = 2;  // a wrong value, or a store far from its piece
            else if (cnt[k] != 1 && !o.check) o.check = 3;
            o.bytes[k] = cnt[k] ? want[k] : out[k];
        }
        o.n = nrec;
        o.first = first;
        o.off.assign(ooff, ooff + nrec + 1);
        free(ooff);
        free(block);
    }
};

struct Reader {
    const uint8_t *p;
    size_t n, at = 0;
    bool ok = true;
    void get(void *dst, size_t k) {
        if (at + k > n) {
            ok = false;
            memset(dst, 0, k);
            return;
        }
        memcpy(dst, p + at, k);
        at += k;
    }
    uint32_t u32() {
        uint32_t v;
        get(&v, 4);
        return v;
    }
    uint64_t u64() {
        uint64_t v;
        get(&v, 8);
        return v;
    }
};

void put(std::string &o, const void *p, size_t k) { o.append((const char *)p, k); }
void put32(std::string &o, uint32_t v) { put(o, &v, 4); }
void put64(std::string &o, uint64_t v) { put(o, &v, 8); }

// IN:  u32 n_cases, then per case
//        u32 n_runs, u32 n_ref, u64 chunk_bytes, u32 order_seed, u32 n_emit, u32 guard, u32 flags (1: an empty run gets NULL pointers, 2: no plan is made,
//        4: the run table itself is NULL)
//        per run: u32 n_records, u32 n_off, u64 n_bytes (what the descriptor says), u64 data_len, record_off [n_off], the data
//        u32 emit [n_emit] (chunks, in the order to emit them)
//        u64 expect_len, the merged stream's expected bytes
// OUT: per case
//        i32 status, u32 err_run, err_record, err_kind, u32 n, u32 n_mapped, u32 n_chunks, u32 0, u64 n_bytes
//        status 0: src [n], key [n], record_off [n + 1], chunk_first [n_chunks + 1], chunk_off [n_chunks + 1]
//        per emit: i32 status (-4: the plan's chunk leaves the expected bytes), and for status 0: i32 check, u32 n, u32 first, u64 n_bytes,
//        record_off [n + 1], the bytes
bool run_blob(const uint8_t *in, size_t in_len, std::string &out) {
    Reader rd{in, in_len};
    const uint32_t n_cases = rd.u32();
    for (uint32_t cs = 0; cs < n_cases && rd.ok; ++cs) {
        const uint32_t n_runs = rd.u32(), n_ref = rd.u32();
        const uint64_t chunk_bytes = rd.u64();
        const uint32_t seed = rd.u32(), n_emit = rd.u32(), guard = rd.u32(), flags = rd.u32();
        if (!rd.ok || n_runs > (1u << 20)) return false;
        MergeRun *runs = exact<MergeRun>(n_runs);
        std::vector<void *> owned;
        for (uint32_t r = 0; r < n_runs; ++r) {
            const uint32_t nrec = rd.u32(), n_off = rd.u32();
            const uint64_t nb = rd.u64(), data_len = rd.u64();
            if (!rd.ok || n_off > in_len || data_len > in_len) return false;
            uint64_t *off = exact<uint64_t>(n_off);
            uint8_t *data = exact<uint8_t>((size_t)data_len);
            rd.get(off, (size_t)n_off * 8);
            rd.get(data, (size_t)data_len);
            owned.push_back(off);
            owned.push_back(data);
            const bool null = (flags & 1u) && !nrec;
            runs[r] = MergeRun{null ? nullptr : data, nb, nrec, null ? nullptr : off};
        }
        std::vector<uint32_t> emits(n_emit);
        for (uint32_t k = 0; k < n_emit; ++k) emits[k] = rd.u32();
        const uint64_t expect_len = rd.u64();
        if (!rd.ok || expect_len > in_len) return false;
        uint8_t *expect = exact<uint8_t>((size_t)expect_len);
        rd.get(expect, (size_t)expect_len);
        if (!rd.ok) return false;
        EmuCtx ctx;
        PlanOut po;
        if (flags & 2u) po.status = -1;
        else ctx.plan((flags & 4u) ? nullptr : runs, n_runs, n_ref, chunk_bytes, seed, po);
        put32(out, (uint32_t)po.status);
        put32(out, po.err_run);
        put32(out, po.err_record);
        put32(out, po.err_kind);
        put32(out, po.n);
        put32(out, po.n_mapped);
        put32(out, po.n_chunks);
        put32(out, 0);
        put64(out, po.n_bytes);
        if (po.status == ST_OK) {
            const uint32_t n = po.n;
            if (n) {
                put(out, ctx.src[ctx.cur], (size_t)n * 4);
                put(out, ctx.key[ctx.cur], (size_t)n * 8);
            }
            put(out, ctx.off, ((size_t)n + 1) * 8);
            if (n) {
                put(out, ctx.chunk_first, ((size_t)po.n_chunks + 1) * 4);
                put(out, ctx.chunk_off, ((size_t)po.n_chunks + 1) * 8);
            } else {
                put32(out, 0);
                put64(out, 0);
            }
        }
        for (uint32_t k = 0; k < n_emit; ++k) {
            ChunkOut co;
            ctx.emit(emits[k], seed + k, guard, expect, (size_t)expect_len, co);
            put32(out, (uint32_t)co.status);
            if (co.status != ST_OK) continue;
            put32(out, (uint32_t)co.check);
            put32(out, co.n);
            put32(out, co.first);
            put64(out, co.bytes.size());
            put(out, co.off.data(), co.off.size() * 8);
            put(out, co.bytes.data(), co.bytes.size());
        }
        for (void *p : owned) free(p);
        free(runs);
        free(expect);
    }
    return rd.ok;
}
}  // namespace

// -> 0 and *out / *out_len (a malloc block: emu_merge_free), or 2 for a malformed blob
extern "C" int emu_merge_blob(const uint8_t *in, uint64_t in_len, uint8_t **out, uint64_t *out_len) {
    std::string o;
    if (!run_blob(in, (size_t)in_len, o)) return 2;
    *out = (uint8_t *)malloc(o.size() ? o.size() : 1);
    memcpy(*out, o.data(), o.size());
    *out_len = o.size();
    return 0;
}
extern "C" void emu_merge_free(uint8_t *p) { free(p); }
extern "C" uint32_t emu_merge_threads(void) { return MERGE_THREADS; }
extern "C" uint32_t emu_merge_max_runs(void) { return MERGE_MAX_RUNS; }

#ifdef EMU_MERGE_MAIN
// emu_merge_asan IN OUT: the blobs above as files
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    const long len = ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t *in = exact<uint8_t>((size_t)len);
    if (len < 0 || fread(in, 1, (size_t)len, f) != (size_t)len) return 2;
    fclose(f);
    std::string o;
    const bool ok = run_blob(in, (size_t)len, o);
    free(in);
    if (!ok) return 2;
    FILE *g = fopen(argv[2], "wb");
    if (!g || fwrite(o.data(), 1, o.size(), g) != o.size()) return 2;
    fclose(g);
    return 0;
}
#endif
