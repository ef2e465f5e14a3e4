// tests/emu/emu_fasta.cpp -- fasta_core.hpp (the device code and the host's carry of plo_fasta_*) executed on the host: every tile by an
// emulated wave of 64 lanes (tests/emu/plo_wave.hpp), the tiles strided over n_waves waves as the k_fa_* kernels stride them over their
// grids, the pieces handled one after the other as engine.hip's fasta_piece handles them (the 64-bit scans of the tiles' counts, which the
// engine takes from records_core.hpp, are plain loops here).  The result must not depend on the pieces' cuts, the number of waves or the
// order of the lanes.
// TEST INFRASTRUCTURE ONLY.  Built as a shared library (tests/emu_fasta_lib.py) and, with -DEMU_FASTA_MAIN, as a program for the
// AddressSanitizer run.  Every array, the piece's text and the output allocation too, sits in a heap block of its exact size (the output
// between two canaries of 64 bytes, which are checked at the end).
#include <plo_wave.hpp>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#define PLO_FA_HOST 1
#include "../../portello_amd/csrc/fasta_core.hpp"

using namespace plo;

namespace {
constexpr size_t CANARY = 64;

template <class T>
T *exact(size_t n) {  // a heap block of exactly n elements (one byte when n == 0: no access to it is in range)
    return (T *)malloc(n ? n * sizeof(T) : 1);
}

struct Case {
    const uint8_t *text = nullptr;
    uint64_t n = 0;
    std::vector<uint64_t> piece_len;
    bool has_want = false;
    std::vector<std::string> names;
    std::vector<int64_t> lens;
    unsigned order_seed = 0;
    uint32_t n_waves = 1;
    bool vec = true;
};

struct Result {
    int status = 0;  // 0, 8 (PLO_ERR_DATA), 1 (a bad wanted list)
    FaHost h;
    uint32_t canary_ok = 1;
    std::vector<uint8_t> alloc;  // the output allocation
    std::vector<long long> chrom_dst, chrom_len;
};

struct Out {  // the output allocation between its canaries
    uint8_t *block = nullptr;
    size_t cap = 0;
    uint8_t *p() const { return block + CANARY; }
    void ensure(size_t need) {
        if (block && need <= cap) return;
        uint8_t *b = exact<uint8_t>(need + 2 * CANARY);
        memset(b, 0xA5, CANARY);
        memset(b + CANARY, 0, need);
        memset(b + CANARY + need, 0xA5, CANARY);
        if (block) {
            memcpy(b + CANARY, p(), cap);
            free(block);
        }
        block = b;
        cap = need;
    }
    bool canaries() const {
        for (size_t i = 0; i < CANARY; ++i)
            if (block[i] != 0xA5 || block[CANARY + cap + i] != 0xA5) return false;
        return true;
    }
};

// a piece of a job between its passes
struct Piece {
    bool live = false, emit = false;
    uint32_t n = 0, nt = 0, n_hdr = 0;
    unsigned long long n_bases = 0;
    uint8_t *text = nullptr;
    unsigned *tile_fn = nullptr, *tile_state = nullptr;
    unsigned long long *cnt = nullptr, *start = nullptr;
    FaHeader *hdr = nullptr;
    FaDest *dest = nullptr;
    int err[2] = {FA_NONE, FA_NONE};
    DevFasta d;
};

struct Job {
    Case c;
    Result r;
    Out out;
    size_t next = 0;
    uint64_t at = 0;
    Piece p;
};

template <class F>
void each_wave(const Case &c, F body) {
    for (uint32_t k = 0; k < c.n_waves; ++k) body(c.order_seed & 1u ? c.n_waves - 1 - k : k);
}

// The jobs (all of one order_seed) piece by piece, as fasta_piece of engine.hip issues a piece: k_fa_lines, k_fa_states, k_fa_count | the
// scans | k_fa_headers | the host's part | k_fa_emit.  One emulator run executes a pass of EVERY job's current piece (setting up the 64
// fibers costs more than these small pieces do); wv::sync() stands where one launch ends and the next begins.
void run_jobs(std::vector<Job *> &jobs, unsigned order_seed) {
    wv::EmuWave ew;
    ew.order_seed = order_seed;
    for (Job *j : jobs) {
        if (j->c.has_want) {
            std::vector<const char *> np;
            for (const std::string &s : j->c.names) np.push_back(s.c_str());
            if (!j->r.h.init((uint32_t)np.size(), np.data(), j->c.lens.data())) j->r.status = 1;
        }
        j->out.ensure(j->c.has_want ? (size_t)j->r.h.out_bytes : 0);
    }
    for (;;) {
        bool any = false, any_hdr = false, any_emit = false;
        for (Job *j : jobs) {
            Piece &p = j->p;
            p = Piece();
            FaHost &h = j->r.h;
            while (j->r.status == 0 && !h.err_kind && j->next < j->c.piece_len.size() && j->c.piece_len[j->next] == 0) ++j->next;
            if (j->r.status != 0 || h.err_kind || j->next >= j->c.piece_len.size()) continue;
            p.live = any = true;
            p.n = (uint32_t)j->c.piece_len[j->next++];
            p.nt = (p.n + FA_TILE - 1) / FA_TILE;
            p.text = exact<uint8_t>(p.n);
            memcpy(p.text, j->c.text + j->at, p.n);
            j->at += p.n;
            p.tile_fn = exact<unsigned>(p.nt);
            p.tile_state = exact<unsigned>((size_t)p.nt + 1);
            p.cnt = exact<unsigned long long>((size_t)p.nt * 2);
            p.start = exact<unsigned long long>(((size_t)p.nt + 1) * 2);
            memset(&p.d, 0, sizeof(p.d));
            p.d.text = p.text;
            p.d.n = p.n;
            p.d.n_tiles = p.nt;
            p.d.in_state = h.state;
            p.d.tile_fn = p.tile_fn;
            p.d.tile_state = p.tile_state;
            p.d.cnt = p.cnt;
            p.d.start = p.start;
            p.d.err = p.err;
            p.d.want_first_base = h.recs.empty() ? 1 : 0;
        }
        if (!any) break;
        ew.run([&]() {
            for (Job *j : jobs) {
                if (!j->p.live) continue;
                const DevFasta &d = j->p.d;
                each_wave(j->c, [&](uint32_t w) { fa_lines_tiles(d, w, j->c.n_waves); });
                wv::sync();
                fa_states(d);
                wv::sync();
                each_wave(j->c, [&](uint32_t w) { fa_tiles<0, false>(d, w, j->c.n_waves); });
            }
        });
        for (Job *j : jobs) {
            Piece &p = j->p;
            if (!p.live) continue;
            for (int y = 0; y < 2; ++y) {
                unsigned long long run = 0;
                for (uint32_t t = 0; t < p.nt; ++t) {
                    p.start[(size_t)y * (p.nt + 1) + t] = run;
                    run += p.cnt[(size_t)y * p.nt + t];
                }
                p.start[(size_t)y * (p.nt + 1) + p.nt] = run;
            }
            p.n_bases = p.start[p.nt];
            p.n_hdr = (uint32_t)p.start[(size_t)p.nt + 1 + p.nt];
            p.hdr = exact<FaHeader>(p.n_hdr);
            p.d.hdr = p.hdr;
            any_hdr |= p.n_hdr != 0;
        }
        if (any_hdr)
            ew.run([&]() {
                for (Job *j : jobs)
                    if (j->p.live && j->p.n_hdr) each_wave(j->c, [&](uint32_t w) { fa_tiles<1, false>(j->p.d, w, j->c.n_waves); });
            });
        for (Job *j : jobs) {
            Piece &p = j->p;
            if (!p.live) continue;
            FaHost &h = j->r.h;
            std::vector<FaDest> dest;
            p.emit = h.piece(p.text, p.n, p.hdr, p.n_hdr, p.n_bases, p.tile_state[p.nt], p.err[0], p.err[1], dest) && !h.err_kind;
            if (!p.emit) continue;
            any_emit = true;
            j->out.ensure((size_t)h.out_bytes);
            p.dest = exact<FaDest>(dest.size());
            memcpy(p.dest, dest.data(), dest.size() * sizeof(FaDest));
            p.d.dest = p.dest;
            p.d.out = j->out.p();
        }
        if (any_emit)
            ew.run([&]() {
                for (Job *j : jobs) {
                    if (!j->p.live || !j->p.emit) continue;
                    if (j->c.vec) each_wave(j->c, [&](uint32_t w) { fa_tiles<2, true>(j->p.d, w, j->c.n_waves); });
                    else each_wave(j->c, [&](uint32_t w) { fa_tiles<2, false>(j->p.d, w, j->c.n_waves); });
                }
            });
        for (Job *j : jobs) {
            Piece &p = j->p;
            free(p.dest);
            free(p.hdr);
            free(p.start);
            free(p.cnt);
            free(p.tile_state);
            free(p.tile_fn);
            free(p.text);
            p = Piece();
        }
    }
    for (Job *j : jobs) {
        Result &r = j->r;
        FaHost &h = r.h;
        if (r.status == 1) {
            free(j->out.block);
            continue;
        }
        const int refused = h.finish();
        j->out.ensure((size_t)h.out_bytes);
        r.alloc.assign(j->out.p(), j->out.p() + j->out.cap);  // (of a refused load too: the tests look at what a record longer than its slot left)
        if (refused) {
            r.status = 8;
        } else if (h.has_want) {
            r.chrom_dst = h.want_dst;
            r.chrom_len = h.want_len;
        } else {
            for (const FaRec &rec : h.recs) {
                r.chrom_dst.push_back(rec.dst);
                r.chrom_len.push_back(rec.len);
            }
        }
        r.canary_ok = j->out.canaries() ? 1u : 0u;
        free(j->out.block);
    }
}

template <class T>
void put(std::vector<uint8_t> &b, T v) {
    const uint8_t *p = (const uint8_t *)&v;
    b.insert(b.end(), p, p + sizeof(T));
}

// i32 status, i32 err_kind, u64 err_offset, u32 err_chrom, u32 canary_ok, i64 err_len, u64 n_records, u64 n_bases, u64 text_bytes; per
// record u32 id length, the id, i64 len, i32 want; u32 n_chroms, per chromosome i64 dst, i64 len; u64 bytes of the allocation, the bytes
void serialise(const Result &r, std::vector<uint8_t> &b) {
    put<int32_t>(b, r.status);
    put<int32_t>(b, r.h.err_kind);
    put<uint64_t>(b, r.h.err_offset);
    put<uint32_t>(b, r.h.err_chrom);
    put<uint32_t>(b, r.canary_ok);
    put<int64_t>(b, r.h.err_len);
    put<uint64_t>(b, r.h.recs.size());
    put<uint64_t>(b, r.h.n_bases);
    put<uint64_t>(b, r.h.file_off);
    for (const FaRec &rec : r.h.recs) {
        put<uint32_t>(b, (uint32_t)rec.id.size());
        b.insert(b.end(), rec.id.begin(), rec.id.end());
        put<int64_t>(b, rec.len);
        put<int32_t>(b, rec.want);
    }
    put<uint32_t>(b, (uint32_t)r.chrom_dst.size());
    for (size_t i = 0; i < r.chrom_dst.size(); ++i) {
        put<int64_t>(b, r.chrom_dst[i]);
        put<int64_t>(b, r.chrom_len[i]);
    }
    put<uint64_t>(b, r.alloc.size());
    b.insert(b.end(), r.alloc.begin(), r.alloc.end());
}

// IN: u32 n_cases, then per case u64 n, u32 n_pieces, u32 has_want, u32 n_want, u32 order_seed, u32 n_waves, u32 vec, the pieces' lengths
// [n_pieces] u64, the text, and per wanted name u32 its length, its bytes, i64 the length wanted.  OUT per case: u64 the bytes of its result,
// the result as serialise() writes it.  The texts are copied into heap blocks of their exact size.  -> false: IN is cut short
bool run_all(const uint8_t *in, uint64_t in_bytes, std::vector<uint8_t> &out) {
    uint64_t at = 0;
    auto take = [&](void *dst, uint64_t n) {
        if (at + n > in_bytes) return false;
        memcpy(dst, in + at, (size_t)n);
        at += n;
        return true;
    };
    uint32_t n_cases = 0;
    if (!take(&n_cases, 4)) return false;
    std::vector<Job> jobs(n_cases);
    std::vector<uint8_t *> texts;
    for (Job &j : jobs) {
        Case &c = j.c;
        uint32_t h[6];
        if (!take(&c.n, 8) || !take(h, 24)) return false;
        c.piece_len.resize(h[0]);
        if (h[0] && !take(c.piece_len.data(), 8ull * h[0])) return false;
        uint8_t *t = exact<uint8_t>((size_t)c.n);
        texts.push_back(t);
        if (c.n && !take(t, c.n)) return false;
        c.text = t;
        c.has_want = h[1] != 0;
        for (uint32_t i = 0; i < h[2]; ++i) {
            uint32_t ln;
            int64_t wl;
            if (!take(&ln, 4)) return false;
            std::string s(ln, '\0');
            if (ln && !take(&s[0], ln)) return false;
            if (!take(&wl, 8)) return false;
            c.names.push_back(s);
            c.lens.push_back(wl);
        }
        c.order_seed = h[3];
        c.n_waves = h[4] ? h[4] : 1;
        c.vec = h[5] != 0;
    }
    std::vector<char> done(jobs.size(), 0);
    for (size_t a = 0; a < jobs.size(); ++a) {  // the jobs of one order_seed together
        if (done[a]) continue;
        std::vector<Job *> group;
        for (size_t b = a; b < jobs.size(); ++b)
            if (!done[b] && jobs[b].c.order_seed == jobs[a].c.order_seed) {
                group.push_back(&jobs[b]);
                done[b] = 1;
            }
        run_jobs(group, jobs[a].c.order_seed);
    }
    for (Job &j : jobs) {
        std::vector<uint8_t> b;
        serialise(j.r, b);
        put<uint64_t>(out, b.size());
        out.insert(out.end(), b.begin(), b.end());
    }
    for (uint8_t *t : texts) free(t);
    return true;
}
}  // namespace

extern "C" uint32_t emu_fasta_tile(void) { return FA_TILE; }

// -> the bytes of OUT written to `out`, -1: IN is cut short, -2: out_cap is too small
extern "C" long long emu_fasta_many(const uint8_t *in, uint64_t in_bytes, uint8_t *out, uint64_t out_cap) {
    std::vector<uint8_t> b;
    if (!run_all(in, in_bytes, b)) return -1;
    if (b.size() > out_cap) return -2;
    memcpy(out, b.data(), b.size());
    return (long long)b.size();
}

#ifdef EMU_FASTA_MAIN
// emu_fasta_asan IN OUT: the files of run_all
int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb");
    FILE *o = fopen(argv[2], "wb");
    if (!f || !o) return 2;
    fseek(f, 0, SEEK_END);
    const long size = ftell(f);
    fseek(f, 0, SEEK_SET);
    uint8_t *in = exact<uint8_t>((size_t)size);
    if (size && fread(in, 1, (size_t)size, f) != (size_t)size) return 2;
    std::vector<uint8_t> b;
    const bool ok = run_all(in, (uint64_t)size, b);
    free(in);
    if (!ok) return 2;
    fwrite(b.data(), 1, b.size(), o);
    fclose(f);
    fclose(o);
    return 0;
}
#endif
