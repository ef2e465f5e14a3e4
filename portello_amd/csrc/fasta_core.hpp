// fasta_core.hpp -- the reference FASTA as upper-cased ASCII arrays in device memory (plo_fasta_*, portello_liftover.h states the rule).
// The text arrives in pieces.  A piece is cut into tiles of FA_TILE bytes, a wave each: FA_TRIPS trips in which lane l reads the 16 bytes
// at tile + 1024 trip + 16 l, neighbouring lanes neighbouring words.  What a byte is depends on the LINE STATE in front of it:
//   FA_LS  at a line start     FA_H  inside a header line     FA_Q  inside a sequence line
// and a stretch of bytes acts on that state as a function {LS, H, Q} -> {LS, H, Q}, six bits; functions compose associatively, so
//   fa_lines    reduces every tile to its function,
//   fa_states   (one wave) scans the tiles' functions from the state the previous piece left: the state in front of every tile,
//   fa_tile<0>  classifies every byte: bases and header lines per tile, the lowest refused byte and the lowest base by atomic min,
//   (the 64-bit scan of records_core.hpp turns the counts into offsets)
//   fa_tile<1>  writes the table of the piece's header lines: where the '>' stands and how many bases of the piece precede it,
//   (the host reads the ids at those offsets from its own copy of the piece and gives every record a destination: FaHost below)
//   fa_tile<2>  stores every base upper-cased at destination + its rank inside its record, guarded by the slot's length.
// A '\n' as the last byte of a tile leaves FA_LS, and the '>' that opens the next tile is a header line's: no kernel looks at a
// neighbouring tile's bytes.  No LDS; every store is an ordinary vector store of bytes that belong to the storing lane alone.
// The second part (FaHost, behind PLO_FA_HOST) is plain C++: the carry between pieces, the ids, the wanted list and the refusals.  The
// engine and the CPU emulator (tests/emu/emu_fasta.cpp) compile both parts, so the tests run the code the library runs.
#pragma once
#include <stdint.h>

#ifndef PLO_HD
#define PLO_HD inline
#endif

namespace plo {

#ifndef PLO_FA_TILE
#define PLO_FA_TILE 4096
#endif
constexpr uint32_t FA_TILE = PLO_FA_TILE;  // a multiple of 1024 (EXPERIMENTS 17.1)
constexpr int FA_TRIPS = (int)(FA_TILE / 1024u);
static_assert(FA_TILE % 1024u == 0 && FA_TILE >= 1024u && FA_TILE <= 16384u, "a tile is 1 .. 16 trips of 64 lanes x 16 bytes (its counts share a word, 16 bits each)");
constexpr int FA_NONE = 0x7fffffff;
constexpr uint32_t FA_MAX_PIECE = 1u << 30;  // offsets inside a piece travel by a 32-bit atomic min
constexpr long long FA_NO_CAP = 1ll << 62;

enum { FA_LS = 0, FA_H = 1, FA_Q = 2 };
constexpr unsigned FA_IDENT = FA_LS | (FA_H << 2) | (FA_Q << 4);
// plo_fasta_out::err_kind (PLO_FA_ERR_*)
enum { FA_ERR_BAD_BYTE = 1, FA_ERR_NO_HEADER = 2, FA_ERR_MISSING = 3, FA_ERR_LENGTH = 4, FA_ERR_DUPLICATE = 5 };

struct FaHeader {  // a header line of the piece
    unsigned long long off;    // where its '>' stands in the piece
    unsigned long long bases;  // bases of the piece in front of it
};
struct FaDest {  // where the bases of a record of the piece go ([0]: the record the piece starts in)
    long long base0;  // bases of the piece in front of the record's first base (negative: the record began in an earlier piece)
    long long dst;    // byte offset of its slot in the output allocation, < 0: the record is not stored
    long long cap;    // the slot's length
};

PLO_HD unsigned fa_apply(unsigned f, unsigned s) { return (f >> (2u * s)) & 3u; }
// first, then `then`
PLO_HD unsigned fa_compose(unsigned first, unsigned then) {
    return fa_apply(then, fa_apply(first, FA_LS)) | (fa_apply(then, fa_apply(first, FA_H)) << 2) | (fa_apply(then, fa_apply(first, FA_Q)) << 4);
}
PLO_HD unsigned fa_step(unsigned s, unsigned b) { return b == '\n' ? (unsigned)FA_LS : (s == FA_LS ? (b == '>' ? (unsigned)FA_H : (unsigned)FA_Q) : s); }
// a byte of a sequence line: 0 dropped, 1 a base, 2 refused
PLO_HD unsigned fa_seq_class(unsigned b) {
    if (b == '\n' || b == '\r' || b == ' ' || b == '\t') return 0u;
    return ((b | 0x20u) - 'a') < 26u ? 1u : 2u;
}
PLO_HD bool fa_id_ends(unsigned b) { return b == ' ' || b == '\t' || b == '\r' || b == '\n'; }
PLO_HD unsigned long long fa_slot_bytes(long long len) { return ((unsigned long long)(len < 16 ? 16 : len) + 255ull) & ~255ull; }

}  // namespace plo

#ifdef PLO_WAVE
namespace plo {

struct DevFasta {
    const uint8_t *text;  // the piece, at a 16-byte boundary
    uint32_t n, n_tiles;
    unsigned in_state;           // the line state in front of byte 0
    unsigned *tile_fn;           // [n_tiles]
    unsigned *tile_state;        // [n_tiles + 1] the state in front of every tile, and behind the last
    unsigned long long *cnt;     // [2][n_tiles] bases, header lines
    unsigned long long *start;   // [2][n_tiles + 1] their exclusive scans
    int *err;                    // [2] the lowest refused byte, the lowest base (FA_NONE: none)
    int want_first_base;         // no header line has been seen yet: err[1] is wanted
    FaHeader *hdr;               // [header lines of the piece]
    const FaDest *dest;          // [header lines + 1]
    uint8_t *out;
};

struct alignas(16) FaWord {
    unsigned w[4];
};

// the 16 bytes at off as four words, zero behind the piece's end -> how many of them are the piece's.  Nothing at or behind text + n is read.
PLO_DEV unsigned fa_load16(const uint8_t *text, unsigned long long off, unsigned long long n, unsigned w[4]) {
    if (off + 16ull <= n) {
        const FaWord v = *(const FaWord *)(text + off);
        w[0] = v.w[0];
        w[1] = v.w[1];
        w[2] = v.w[2];
        w[3] = v.w[3];
        return 16u;
    }
    w[0] = w[1] = w[2] = w[3] = 0u;
    const unsigned nv = off < n ? (unsigned)(n - off) : 0u;
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if ((unsigned)i < nv) w[i >> 2] |= (unsigned)text[off + (unsigned)i] << (8 * (i & 3));
    return nv;
}
PLO_DEV unsigned fa_byte(const unsigned w[4], int i) { return (w[i >> 2] >> (8 * (i & 3))) & 0xffu; }

// what the lane's bytes do to the line state: with a '\n' among them whatever stood in front is forgotten
PLO_DEV unsigned fa_chunk_fn(const unsigned w[4], unsigned nv) {
    unsigned s = FA_LS;
    bool nl = false;
#pragma unroll
    for (int i = 0; i < 16; ++i)
        if ((unsigned)i < nv) {
            const unsigned b = fa_byte(w, i);
            nl |= b == '\n';
            s = fa_step(s, b);
        }
    return nl ? (s | (s << 2) | (s << 4)) : (s | (FA_H << 2) | (FA_Q << 4));
}

// inclusive scan of the lanes' functions, lane 0 first
PLO_DEV unsigned fa_wave_scan_fn(unsigned x) {
    const int l = wv::lane();
    for (int s = 1; s < 64; s <<= 1) {
        const unsigned t = wv::shfl(x, (l - s) & 63);
        if (l >= s) x = fa_compose(t, x);
    }
    return x;
}

PLO_DEV int fa_wave_min(int v) { return -wv::reduce_max(-v); }  // (v >= 0 or FA_NONE)

// tile -> its function
PLO_DEV void fa_lines(const DevFasta &d, uint32_t tile) {
    unsigned f = FA_IDENT;
    for (int trip = 0; trip < FA_TRIPS; ++trip) {
        const unsigned long long trip_off = (unsigned long long)tile * FA_TILE + (unsigned)trip * 1024u;
        if (trip_off >= d.n) break;  // (wave-uniform: the piece ends inside the tile)
        const unsigned long long off = trip_off + (unsigned)wv::lane() * 16u;
        unsigned w[4];
        const unsigned nv = fa_load16(d.text, off, d.n, w);
        f = fa_compose(f, (unsigned)wv::bcast_last((int)fa_wave_scan_fn(fa_chunk_fn(w, nv))));
    }
    if (wv::lane() == 0) d.tile_fn[tile] = f;
}

// one wave: the state in front of every tile.  A lane takes FA_STATE_RUN neighbouring tiles, so a trip of the wave covers 512 of them: with
// one tile a lane the 16 384 tiles of a 64 MiB piece were 256 dependent trips, 135 us, a third of the piece's kernel time (EXPERIMENTS 17.4)
constexpr uint32_t FA_STATE_RUN = 8;
PLO_DEV void fa_states(const DevFasta &d) {
    unsigned st = d.in_state;
    for (uint32_t b0 = 0; b0 < d.n_tiles; b0 += 64u * FA_STATE_RUN) {
        const uint32_t i0 = b0 + (uint32_t)wv::lane() * FA_STATE_RUN;
        unsigned f[FA_STATE_RUN], run = FA_IDENT;
#pragma unroll
        for (uint32_t k = 0; k < FA_STATE_RUN; ++k) f[k] = i0 + k < d.n_tiles ? d.tile_fn[i0 + k] : FA_IDENT;
#pragma unroll
        for (uint32_t k = 0; k < FA_STATE_RUN; ++k) run = fa_compose(run, f[k]);
        const unsigned incl = fa_wave_scan_fn(run);
        unsigned s = fa_apply((unsigned)wv::shfl_up1((int)incl, (int)FA_IDENT), st);  // in front of the lane's first tile
#pragma unroll
        for (uint32_t k = 0; k < FA_STATE_RUN; ++k) {
            if (i0 + k < d.n_tiles) d.tile_state[i0 + k] = s;
            s = fa_apply(f[k], s);
        }
        st = fa_apply((unsigned)wv::bcast_last((int)incl), st);
    }
    if (wv::lane() == 0) d.tile_state[d.n_tiles] = st;
}

// MODE 0: count, 1: the header table, 2: emit (VEC: a lane whose 16 bytes are 16 bases of one record stores them at once)
template <int MODE, bool VEC>
PLO_DEV void fa_tile(const DevFasta &d, uint32_t tile) {
    const uint32_t nt = d.n_tiles;
    if (MODE == 1 && d.cnt[(size_t)nt + tile] == 0) return;  // (wave-uniform)
    if (MODE == 2 && d.cnt[tile] == 0) return;
    unsigned st = d.tile_state[tile];
    unsigned long long base_run = MODE ? d.start[tile] : 0ull, hdr_run = MODE ? d.start[(size_t)nt + 1 + tile] : 0ull;
    unsigned tot = 0;
    int bad = FA_NONE, fbase = FA_NONE;
    for (int trip = 0; trip < FA_TRIPS; ++trip) {
        const unsigned long long trip_off = (unsigned long long)tile * FA_TILE + (unsigned)trip * 1024u;
        if (trip_off >= d.n) break;  // (wave-uniform: the piece ends inside the tile)
        const unsigned long long off = trip_off + (unsigned)wv::lane() * 16u;
        unsigned w[4];
        const unsigned nv = fa_load16(d.text, off, d.n, w);
        const unsigned incl = fa_wave_scan_fn(fa_chunk_fn(w, nv));
        const unsigned s0 = fa_apply((unsigned)wv::shfl_up1((int)incl, (int)FA_IDENT), st);
        st = fa_apply((unsigned)wv::bcast_last((int)incl), st);
        unsigned s = s0, nb = 0, nh = 0;
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if ((unsigned)i < nv) {
                const unsigned b = fa_byte(w, i);
                if (b == '\n') {
                    s = FA_LS;
                } else {
                    if (s == FA_LS) {
                        if (b == '>') {
                            s = FA_H;
                            ++nh;
                        } else {
                            s = FA_Q;
                        }
                    }
                    if (s == FA_Q) {
                        const unsigned cl = fa_seq_class(b);
                        if (cl == 1u) {
                            if (MODE == 0 && fbase == FA_NONE) fbase = (int)(off + (unsigned)i);
                            ++nb;
                        } else if (cl == 2u) {
                            if (MODE == 0 && bad == FA_NONE) bad = (int)(off + (unsigned)i);
                        }
                    }
                }
            }
        const unsigned packed = (nh << 16) | nb;  // a trip has at most 1024 bases and 512 header lines
        const unsigned inc = (unsigned)wv::scan_add((int)packed);
        const unsigned trip_tot = (unsigned)wv::bcast_last((int)inc);
        if (MODE == 0) {
            tot += trip_tot;
            continue;
        }
        unsigned long long my_base = base_run + ((inc - packed) & 0xffffu), my_hdr = hdr_run + ((inc - packed) >> 16);
        base_run += trip_tot & 0xffffu;
        hdr_run += trip_tot >> 16;
        if (MODE == 1 && nh == 0) continue;
        if (MODE == 2 && nb == 0) continue;
        FaDest to = {0, -1, 0};
        if (MODE == 2) {
            to = d.dest[my_hdr];
            if (VEC && nb == 16u && to.dst >= 0) {  // 16 bases: no header line, nothing dropped
                const long long rank = (long long)my_base - to.base0;
                if (rank + 16 <= to.cap) {
                    FaWord v;
                    v.w[0] = w[0] & 0xdfdfdfdfu;
                    v.w[1] = w[1] & 0xdfdfdfdfu;
                    v.w[2] = w[2] & 0xdfdfdfdfu;
                    v.w[3] = w[3] & 0xdfdfdfdfu;
                    __builtin_memcpy(d.out + to.dst + rank, &v, 16);
                    continue;
                }
            }
        }
        s = s0;
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if ((unsigned)i < nv) {
                const unsigned b = fa_byte(w, i);
                if (b == '\n') {
                    s = FA_LS;
                } else {
                    if (s == FA_LS) {
                        if (b == '>') {
                            s = FA_H;
                            if (MODE == 1) {
                                FaHeader h;
                                h.off = off + (unsigned)i;
                                h.bases = my_base;
                                d.hdr[my_hdr] = h;
                            }
                            ++my_hdr;
                            if (MODE == 2) to = d.dest[my_hdr];
                        } else {
                            s = FA_Q;
                        }
                    }
                    if (s == FA_Q && fa_seq_class(b) == 1u) {
                        if (MODE == 2) {
                            const long long rank = (long long)my_base - to.base0;
                            if (to.dst >= 0 && rank < to.cap) d.out[to.dst + rank] = (uint8_t)(b & 0xdfu);
                        }
                        ++my_base;
                    }
                }
            }
    }
    if (MODE == 0) {
        bad = fa_wave_min(bad);
        fbase = fa_wave_min(fbase);
        if (wv::lane() == 0) {
            d.cnt[tile] = tot & 0xffffu;
            d.cnt[(size_t)nt + tile] = tot >> 16;
            if (bad != FA_NONE) wv::atomic_min(d.err, bad);
            if (d.want_first_base && fbase != FA_NONE) wv::atomic_min(d.err + 1, fbase);
        }
    }
}

// the tiles w, w + nw, ... by wave w of nw
template <int MODE, bool VEC>
PLO_DEV void fa_tiles(const DevFasta &d, uint32_t w, uint32_t nw) {
    for (uint32_t t = w; t < d.n_tiles; t += nw) fa_tile<MODE, VEC>(d, t);
}
PLO_DEV void fa_lines_tiles(const DevFasta &d, uint32_t w, uint32_t nw) {
    for (uint32_t t = w; t < d.n_tiles; t += nw) fa_lines(d, t);
}

}  // namespace plo
#endif

#ifdef PLO_FA_HOST
#include <string>
#include <unordered_map>
#include <vector>

namespace plo {

struct FaRec {
    std::string id;
    long long len = 0;
    int want = -1;               // its place in the wanted list, -1: none (without a list: its own number)
    unsigned long long off = 0;  // file offset of its '>'
    long long dst = -1, cap = 0;
};

// What the host keeps between the pieces, and decides for them.  No HIP in here.
struct FaHost {
    bool has_want = false;
    std::vector<std::string> want_name;
    std::vector<long long> want_len, want_dst, want_rec;
    std::unordered_map<std::string, uint32_t> want_map;
    unsigned long long out_bytes = 0;  // bytes of the output allocation (without a list: what the records so far need)
    unsigned long long next_dst = 0;
    unsigned state = FA_LS;  // the carry: line state, whether the last header line's id goes on, the open record (recs.back()) and its bases
    bool id_open = false;
    long long open_bases = 0;
    std::vector<FaRec> recs;
    unsigned long long file_off = 0, n_bases = 0;
    int err_kind = 0;
    unsigned long long err_offset = 0;
    uint32_t err_chrom = 0;
    long long err_len = 0;
    bool dup = false;
    unsigned long long dup_off = 0;
    uint32_t dup_chrom = 0;

    // -> false: a name twice, or a negative length
    bool init(uint32_t n, const char *const *names, const int64_t *lens) {
        has_want = true;
        for (uint32_t i = 0; i < n; ++i) {
            if (!names[i] || lens[i] < 0 || !want_map.emplace(names[i], i).second) return false;
            want_name.emplace_back(names[i]);
            want_len.push_back(lens[i]);
            want_dst.push_back((long long)out_bytes);
            want_rec.push_back(-1);
            out_bytes += fa_slot_bytes(lens[i]);
        }
        return true;
    }
    void resolve(FaRec &r) {
        if (!has_want) {
            r.want = (int)(recs.size() - 1);
            r.dst = (long long)next_dst;
            r.cap = FA_NO_CAP;
            return;
        }
        auto it = want_map.find(r.id);
        if (it == want_map.end()) return;
        r.want = (int)it->second;
        if (want_rec[it->second] >= 0) {
            if (!dup) {
                dup = true;
                dup_off = r.off;
                dup_chrom = it->second;
            }
            return;
        }
        want_rec[it->second] = (long long)recs.size() - 1;
        r.dst = want_dst[it->second];
        r.cap = want_len[it->second];
    }
    void close_open() {
        FaRec &r = recs.back();
        r.len = open_bases;
        if (!has_want) {
            next_dst = (unsigned long long)r.dst + fa_slot_bytes(r.len);
            if (next_dst > out_bytes) out_bytes = next_dst;
        }
    }
    // A piece behind its count pass: text[0, n), its header table, its bases, the state behind it, the lowest refused byte and the lowest
    // base (FA_NONE: none).  Fills dest [n_hdr + 1] -> true: the piece has bases to store
    bool piece(const uint8_t *text, uint32_t n, const FaHeader *hdr, uint32_t n_hdr, unsigned long long n_bases_piece, unsigned out_state, int bad, int first_base,
               std::vector<FaDest> &dest) {
        long long e = FA_NONE;
        int kind = 0;
        if (bad != FA_NONE) {
            e = bad;
            kind = FA_ERR_BAD_BYTE;
        }
        if (recs.empty() && first_base != FA_NONE && (!n_hdr || (unsigned long long)first_base < hdr[0].off) && first_base < e) {
            e = first_base;
            kind = FA_ERR_NO_HEADER;
        }
        if (kind) {
            err_kind = kind;
            err_offset = file_off + (unsigned long long)e;
            return false;
        }
        dest.assign((size_t)n_hdr + 1, FaDest{0, -1, 0});
        if (id_open) {
            FaRec &r = recs.back();
            uint32_t p = 0;
            while (p < n && !fa_id_ends(text[p])) r.id.push_back((char)text[p++]);
            if (p < n) {
                id_open = false;
                resolve(r);
            }
        }
        if (!recs.empty() && !id_open) dest[0] = FaDest{-open_bases, recs.back().dst, recs.back().cap};
        unsigned long long prev = 0;
        for (uint32_t k = 0; k < n_hdr; ++k) {
            if (!recs.empty()) {
                open_bases += (long long)(hdr[k].bases - prev);
                close_open();
            }
            prev = hdr[k].bases;
            open_bases = 0;
            recs.emplace_back();
            FaRec &r = recs.back();
            r.off = file_off + hdr[k].off;
            uint32_t p = (uint32_t)hdr[k].off + 1u;
            while (p < n && !fa_id_ends(text[p])) r.id.push_back((char)text[p++]);
            if (p < n) {
                resolve(r);
                dest[(size_t)k + 1] = FaDest{(long long)hdr[k].bases, r.dst, r.cap};
            } else {
                id_open = true;  // the line goes on in the next piece: none of its record's bases is in this one
            }
        }
        if (!recs.empty()) open_bases += (long long)(n_bases_piece - prev);
        n_bases += n_bases_piece;
        file_off += n;
        state = out_state;
        if (!has_want && !recs.empty() && !id_open) {
            const unsigned long long need = (unsigned long long)recs.back().dst + fa_slot_bytes(open_bases);
            if (need > out_bytes) out_bytes = need;
        }
        return !dup && n_bases_piece > 0;
    }
    // the end of the text -> 0 or the refusal (err_* are set)
    int finish() {
        if (id_open) {
            id_open = false;
            resolve(recs.back());
        }
        if (!recs.empty()) close_open();
        if (err_kind) return err_kind;
        if (dup) {
            err_kind = FA_ERR_DUPLICATE;
            err_offset = dup_off;
            err_chrom = dup_chrom;
            err_len = recs[(size_t)want_rec[dup_chrom]].len;
            return err_kind;
        }
        for (size_t w = 0; has_want && w < want_name.size(); ++w) {
            if (want_rec[w] < 0) {
                err_kind = FA_ERR_MISSING;
                err_chrom = (uint32_t)w;
                return err_kind;
            }
            if (recs[(size_t)want_rec[w]].len != want_len[w]) {
                err_kind = FA_ERR_LENGTH;
                err_chrom = (uint32_t)w;
                err_len = recs[(size_t)want_rec[w]].len;
                err_offset = recs[(size_t)want_rec[w]].off;
                return err_kind;
            }
        }
        return 0;
    }
};

}  // namespace plo
#endif
