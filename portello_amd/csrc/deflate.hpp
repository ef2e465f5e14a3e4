// deflate.hpp -- DEFLATE (RFC 1951) encoder for one BGZF payload of at most 0xff00 bytes, written for ONE WAVEFRONT per block
// (k_bgzf_deflate, engine.hip) and compiled for the CPU wave emulator as well (tests/emu/emu_deflate.cpp).  The counterpart of
// inflate.hpp: the output of bgzf_deflate_block is a complete BGZF block -- the 18-byte gzip / `BC` header the host writer emits
// (plo_bam_writer::emit, bam_host.cpp) with BSIZE filled in, deflate data ending in a BFINAL block, CRC-32, ISIZE.
//
// Level 1, the one deflate level of the device:
//   * LZ77, 64 positions per round, one per lane.  Lane i hashes the three bytes at cur + i into a table of 16-bit positions in LDS
//     (DEF_HASH_BITS), verifies the candidate it finds there against the payload (8 bytes per compare) and also tries distance 1, so that
//     runs collapse whatever the table holds.  All lanes read the table first; then they insert their own positions, and where several
//     lanes hash alike the HIGHEST position stays (write, read back, the losers that are higher write again): the table does not depend
//     on which lane the hardware lets win a colliding store.
//   * the parse is greedy: the scalar unit walks from the round's first position to its last, literal by literal up to the next lane
//     that holds a match (one ballot, a count of trailing zeros), takes the match and skips its length (one v_readlane).  A match may
//     run past the round's 64 positions; the next round starts behind it.
//   * tokens go to a buffer of 16-bit units in global memory that belongs to the wave (a literal: its byte; a match: 0x8000 | len - 3,
//     then dist - 1); their symbols are counted in LDS as they are chosen.
//   * dynamic Huffman codes from those counts: symbols ranked by (count, symbol) by all lanes, the tree built from the sorted leaves with
//     two queues by lane 0, the leaves' depths found by the lanes again.  A code longer than the limit (15 bits; 7 for the code-length
//     code) halves the counts (rounding up) and builds again -- at most a handful of times, and only for block-sized Fibonacci-like counts.
//   * the size of the block is known before a bit of it is written: a deflate form that is not smaller than the stored one (5 + len
//     bytes) is dropped for a stored block, so a block never exceeds 18 + 5 + len + 8 bytes and level 1 is never worse than level 0.
//   * bits are written 64 tokens at a time: every lane builds the up to 48 bits of its token, an exclusive scan of the bit counts
//     places them, LDS atomic ORs merge them into a window of 32-bit words, the complete words are stored with one instruction per 64.
// Level 0: the stored block and the CRC only -- byte for byte what plo_bam_writer::emit writes for the same payload.
//
// The bytes of a block depend on the payload alone: table inserts have a defined winner, counts and ORs commute, everything else
// is a function of the lane index.  The encoder reads [in, in + n) only and writes [out, out + size) only, size <= 18 + 5 + n + 8; an
// output slot smaller than that bound is refused before anything is written.
#pragma once
#include <stdint.h>

#include "inflate.hpp"  // crc32_wave

namespace plo {

enum { DEF_OK = 0, DEF_ERR_SLOT = -1, DEF_ERR_LENGTH = -2, DEF_ERR_ALIGN = -3, DEF_ERR_INTERNAL = -4 };
constexpr uint32_t DEF_MAX_IN = 0xff00;                       // htslib's BGZF_BLOCK_SIZE
constexpr uint32_t DEF_MAX_BLOCK = 18 + 5 + DEF_MAX_IN + 8;   // header, stored-block header, payload, CRC-32 + ISIZE
constexpr uint32_t DEF_SLOT = (DEF_MAX_BLOCK + 15u) & ~15u;   // stride of the output slots (16-byte aligned for k_bgzf_pack)
constexpr uint32_t DEF_TOK_UNITS = DEF_MAX_IN;                // 16-bit units of a wave's token buffer: a literal takes one per byte, a match two per >= 3
constexpr int DEF_HASH_BITS = 12;
constexpr uint32_t DEF_MAX_DIST = 32768, DEF_MAX_MATCH = 258, DEF_TOO_FAR = 4096;  // (a 3-byte match farther than DEF_TOO_FAR costs more than its literals)
constexpr uint32_t DEF_OBUF_WORDS = 104;                      // bit window: 64 tokens x 48 bits + 31 carried bits, and two words of spill

// per-block workspace: LDS of the wave on the device (10.8 KB), a stack object under the emulator
struct DefTree {
    uint32_t weight[2 * 288];  // Huffman tree: leaves in ascending order, internal nodes behind them
    uint16_t parent[2 * 288];
    uint16_t sorted[288];      // symbols in ascending (count, symbol) order
    uint16_t hseq[320];        // the run-length coded code lengths: code-length symbol | extra bits value << 8
};
struct DefWork {
    union {  // the hash table is done with when the codes are built
        uint16_t head[1 << DEF_HASH_BITS];  // position + 1 of the latest string with this hash, 0 = none
        DefTree t;
    };
    uint32_t lfreq[288], dfreq[32], cfreq[20];
    uint16_t lcode[288], dcode[32], ccode[20];  // codes as they enter the stream (bit-reversed)
    uint8_t llen[288], dlen[32], clen[20];
    uint16_t blcount[16], nextcode[16];
    uint32_t obuf[DEF_OBUF_WORDS];
};
static_assert(sizeof(DefTree) <= sizeof(uint16_t) << DEF_HASH_BITS, "the tree workspace lies over the hash table");

// `Prim` supplies what differs between the device and the emulator beyond plo_wave.hpp: gsync() (LDS and the wave's own global stores
// ordered for all its lanes) and load_written(p) (a token this wave stored earlier and has waited for with gsync(): never from a stale
// line of the CU's vector cache).

PLO_HD unsigned long long def_ld64(const uint8_t *p) {
    unsigned long long v;
    __builtin_memcpy(&v, p, 8);
    return v;
}
PLO_HD uint32_t def_ld32(const uint8_t *p) {
    uint32_t v;
    __builtin_memcpy(&v, p, 4);
    return v;
}
// common prefix of in[a ..] and in[b ..], a < b, at most maxl <= n - b bytes
PLO_HD uint32_t def_match(const uint8_t *in, uint32_t a, uint32_t b, uint32_t maxl) {
    uint32_t k = 0;
    while (k + 8 <= maxl) {
        const unsigned long long x = def_ld64(in + a + k) ^ def_ld64(in + b + k);
        if (x) return k + ((uint32_t)__builtin_ctzll(x) >> 3);
        k += 8;
    }
    while (k < maxl && in[a + k] == in[b + k]) ++k;
    return k;
}
PLO_HD unsigned long long def_range(uint32_t a, uint32_t b) {  // bits [a, b), a <= b <= 64, a < 64
    const unsigned long long hi = b >= 64 ? ~0ull : (1ull << b) - 1ull;
    return hi & ~((1ull << a) - 1ull);
}
PLO_HD uint32_t def_rank(unsigned long long mask, int lane) { return (uint32_t)__builtin_popcountll(mask & ((1ull << lane) - 1ull)); }
// length 3 .. 258 -> code 0 .. 28 (symbol 257 + code), extra bits and their value (RFC 1951, 3.2.5; the inverse of inflate_block's formula)
PLO_HD void def_len_code(uint32_t len, uint32_t &c, uint32_t &eb, uint32_t &ev) {
    const uint32_t x = len - 3;
    if (x < 8) {
        c = x, eb = 0, ev = 0;
    } else if (x == 255) {
        c = 28, eb = 0, ev = 0;
    } else {
        eb = (uint32_t)(31 - __builtin_clz(x)) - 2;
        c = 4 * (eb + 1) + ((x >> eb) & 3u);
        ev = x & ((1u << eb) - 1u);
    }
}
PLO_HD void def_dist_code(uint32_t dist, uint32_t &c, uint32_t &eb, uint32_t &ev) {  // distance 1 .. 32768 -> code 0 .. 29
    const uint32_t y = dist - 1;
    if (y < 4) {
        c = y, eb = 0, ev = 0;
    } else {
        const uint32_t hb = (uint32_t)(31 - __builtin_clz(y));
        eb = hb - 1;
        c = 2 * hb + ((y >> eb) & 1u);
        ev = y & ((1u << eb) - 1u);
    }
}
PLO_HD uint32_t def_len_extra(uint32_t c) { return c < 8 || c == 28 ? 0u : (c - 4) >> 2; }
PLO_HD uint32_t def_dist_extra(uint32_t c) { return c < 4 ? 0u : (c >> 1) - 1; }

// ---- LZ77: tokens of in[0, n) into tok[], their symbols counted in ws.lfreq / ws.dfreq; returns the number of 16-bit units ----------
template <class Prim>
PLO_DEV uint32_t def_tokenize(const Prim &prim, DefWork &ws, const uint8_t *in, uint32_t n, uint16_t *tok) {
    const int lane = wv::lane();
    for (int i = lane; i < (1 << DEF_HASH_BITS); i += 64) ws.head[i] = 0;
    for (int i = lane; i < 288; i += 64) ws.lfreq[i] = 0;
    if (lane < 32) ws.dfreq[lane] = 0;
    wv::sync();
    uint32_t cur = 0, tc = 0;
    while (cur < n) {
        const uint32_t p = cur + (uint32_t)lane;
        const bool hashed = p + 3 <= n;
        uint32_t h = 0, cand = 0;
        if (hashed) {
            const uint32_t v = p + 4 <= n ? def_ld32(in + p) & 0xffffffu : (uint32_t)in[p] | ((uint32_t)in[p + 1] << 8) | ((uint32_t)in[p + 2] << 16);
            h = (v * 0x9E3779B1u) >> (32 - DEF_HASH_BITS);
            cand = ws.head[h];
        }
        wv::sync();  // every lane has read the table
        bool pending = hashed;
        for (;;) {  // the highest position of a hash stays, whichever lane the hardware lets win
            if (pending) ws.head[h] = (uint16_t)(p + 1);
            wv::sync();
            if (pending) pending = ws.head[h] < p + 1;  // (a higher one: it will stay or be replaced by one higher still)
            if (!wv::ballot(pending)) break;
            wv::sync();
        }
        uint32_t mlen = 0, mdist = 0;
        if (p < n) {
            const uint32_t maxl = n - p < DEF_MAX_MATCH ? n - p : DEF_MAX_MATCH;
            if (cand && maxl >= 3) {
                const uint32_t c = cand - 1, d = p - c;  // (inserted in an earlier round: c < cur)
                if (d <= DEF_MAX_DIST) {
                    const uint32_t l = def_match(in, c, p, maxl);
                    if (l >= 3 && !(l == 3 && d > DEF_TOO_FAR)) mlen = l, mdist = d;
                }
            }
            if (p >= 1 && maxl >= 3 && in[p - 1] == in[p]) {
                const uint32_t l = def_match(in, p - 1, p, maxl);
                if (l >= 3 && l >= mlen) mlen = l, mdist = 1;
            }
        }
        // greedy parse of the round's positions: S = lanes at which a token starts, T = those of them that are matches
        const unsigned long long M = wv::ballot(mlen >= 3);
        const uint32_t nvalid = n - cur < 64 ? n - cur : 64;
        unsigned long long S = 0, T = 0;
        uint32_t c = 0;
        while (c < nvalid) {
            const unsigned long long rest = M >> c;
            if (!rest) {
                S |= def_range(c, nvalid);
                c = nvalid;
                break;
            }
            const uint32_t m = c + (uint32_t)__builtin_ctzll(rest);
            S |= def_range(c, m) | (1ull << m);
            T |= 1ull << m;
            c = m + (uint32_t)wv::read_lane((int)mlen, (int)m);
        }
        if ((S >> lane) & 1ull) {
            const uint32_t at = tc + def_rank(S, lane) + def_rank(T, lane);
            if ((T >> lane) & 1ull) {
                uint32_t lc, dc, eb, ev;
                def_len_code(mlen, lc, eb, ev);
                def_dist_code(mdist, dc, eb, ev);
                tok[at] = (uint16_t)(0x8000u | (mlen - 3));
                tok[at + 1] = (uint16_t)(mdist - 1);
                wv::atomic_add(&ws.lfreq[257 + lc], 1u);
                wv::atomic_add(&ws.dfreq[dc], 1u);
            } else {
                const uint32_t b = in[p];
                tok[at] = (uint16_t)b;
                wv::atomic_add(&ws.lfreq[b], 1u);
            }
        }
        tc += (uint32_t)__builtin_popcountll(S) + (uint32_t)__builtin_popcountll(T);
        cur += c;
    }
    if (lane == 0) ws.lfreq[256] = 1;  // end of block
    prim.gsync();
    return tc;
}

// ---- Huffman code of at most `limit` bits for freq[0, nsym): lengths in len[], bit-reversed canonical codes in code[] ------------------
template <class Prim>
PLO_DEV void def_build_code(const Prim &, DefWork &ws, const uint32_t *freq, int nsym, int limit, uint8_t *len, uint16_t *code) {
    const int lane = wv::lane();
    // rank of every used symbol among the used ones, by (count, symbol)
    int used = 0;
    for (int s = lane; s < nsym; s += 64) {
        len[s] = 0;
        const uint32_t f = freq[s];
        if (!f) continue;
        ++used;
        const uint32_t key = (f << 9) | (uint32_t)s;
        int r = 0;
        for (int t = 0; t < nsym; ++t) {
            const uint32_t ft = freq[t];
            r += (ft != 0 && ((ft << 9) | (uint32_t)t) < key) ? 1 : 0;
        }
        ws.t.sorted[r] = (uint16_t)s;
    }
    int m = wv::reduce_add(used);
    wv::sync();
    for (int i = lane; i < m; i += 64) ws.t.weight[i] = freq[ws.t.sorted[i]];
    wv::sync();
    if (m < 2 && lane == 0) {  // a code needs two symbols (zlib's rule: symbol 0, or 1 where 0 is the one in use)
        if (m == 0) {
            ws.t.sorted[0] = 0, ws.t.sorted[1] = 1;
            ws.t.weight[0] = ws.t.weight[1] = 1;
        } else {  // the added symbol weighs 1 and comes first
            const uint16_t s = ws.t.sorted[0];
            ws.t.sorted[1] = s;
            ws.t.weight[1] = ws.t.weight[0];
            ws.t.sorted[0] = s == 0 ? 1 : 0;
            ws.t.weight[0] = 1;
        }
    }
    if (m < 2) m = 2;
    wv::sync();
    for (;;) {
        if (lane == 0) {  // two queues: the sorted leaves [0, m) and the internal nodes [m, 2m - 1) in the order they are made
            int a = 0, b = m, next = m;
            while (next < 2 * m - 1) {
                uint32_t w = 0;
                for (int k = 0; k < 2; ++k) {
                    const bool leaf = a < m && (b >= next || ws.t.weight[a] <= ws.t.weight[b]);
                    const int pick = leaf ? a++ : b++;
                    w += ws.t.weight[pick];
                    ws.t.parent[pick] = (uint16_t)next;
                }
                ws.t.weight[next++] = w;
            }
        }
        wv::sync();
        int deepest = 0;
        for (int i = lane; i < m; i += 64) {
            int d = 0;
            for (int node = i; node != 2 * m - 2; node = ws.t.parent[node]) ++d;
            len[ws.t.sorted[i]] = (uint8_t)d;  // (a tree that is too deep: overwritten by the next one)
            deepest = d > deepest ? d : deepest;
        }
        deepest = wv::reduce_max(deepest);
        wv::sync();
        if (deepest <= limit) break;
        for (int i = lane; i < m; i += 64) ws.t.weight[i] = (ws.t.weight[i] + 1) >> 1;  // (monotone: the leaves stay sorted)
        wv::sync();
    }
    if (lane == 0) {  // canonical codes (RFC 1951, 3.2.2)
        for (int l = 0; l < 16; ++l) ws.blcount[l] = 0;
        for (int s = 0; s < nsym; ++s) ws.blcount[len[s]]++;
        unsigned c = 0;
        ws.blcount[0] = 0;
        for (int l = 1; l < 16; ++l) {
            c = (c + ws.blcount[l - 1]) << 1;
            ws.nextcode[l] = (uint16_t)c;
        }
        for (int s = 0; s < nsym; ++s)
            if (len[s]) code[s] = ws.nextcode[len[s]]++;
    }
    wv::sync();
    for (int s = lane; s < nsym; s += 64) {
        const unsigned l = len[s], cv = code[s];
        unsigned rev = 0;
        for (unsigned b = 0; b < l; ++b) rev |= ((cv >> b) & 1u) << (l - 1 - b);
        code[s] = (uint16_t)(l ? rev : 0);
    }
    wv::sync();
}

// ---- bit writer: a stream of 32-bit words at out32 (the block's byte 16 on), `bitpos` bits of it written so far ---------------------
struct DefBits {
    uint32_t *out32 = nullptr;
    uint32_t cap_words = 0;
    uint32_t bitpos = 0;  // the bits of the open word are in ws.obuf[0]
};
// every lane adds nb <= 48 bits (v, low bit first), lane 0's first; wave-uniform call
PLO_DEV void def_put(DefWork &ws, DefBits &st, unsigned long long v, uint32_t nb) {
    const int lane = wv::lane();
    const int incl = wv::scan_add((int)nb);
    const uint32_t total = (uint32_t)wv::bcast_last(incl);
    if (nb) {
        const uint32_t rel = (st.bitpos & 31u) + (uint32_t)incl - nb, idx = rel >> 5, sh = rel & 31u;
        const unsigned long long lo = v << sh;
        const uint32_t top = sh ? (uint32_t)(v >> (64 - sh)) : 0u;
        if ((uint32_t)lo) wv::atomic_or((int *)&ws.obuf[idx], (int)(uint32_t)lo);
        if ((uint32_t)(lo >> 32)) wv::atomic_or((int *)&ws.obuf[idx + 1], (int)(uint32_t)(lo >> 32));
        if (top) wv::atomic_or((int *)&ws.obuf[idx + 2], (int)top);
    }
    wv::sync();
    const uint32_t w0 = st.bitpos >> 5, nfull = ((st.bitpos + total) >> 5) - w0;
    for (uint32_t k = (uint32_t)lane; k < nfull; k += 64)
        if (w0 + k < st.cap_words) st.out32[w0 + k] = ws.obuf[k];
    const uint32_t carry = ws.obuf[nfull];
    wv::sync();
    for (uint32_t k = (uint32_t)lane; k < nfull + 3 && k < DEF_OBUF_WORDS; k += 64) ws.obuf[k] = k ? 0u : carry;
    wv::sync();
    st.bitpos += total;
}

PLO_DEV void def_copy(uint8_t *dst, const uint8_t *src, uint32_t n) {  // dst[0, n) = src[0, n): aligned 32-bit stores between a bytewise head and tail
    const uint32_t lane = (uint32_t)wv::lane();
    uint32_t head = (4u - (uint32_t)((uintptr_t)dst & 3u)) & 3u;
    if (head > n) head = n;
    const uint32_t nw = (n - head) >> 2;
    if (lane < head) dst[lane] = src[lane];
    for (uint32_t k = lane; k < nw; k += 64) *(uint32_t *)(dst + head + 4 * k) = def_ld32(src + head + 4 * k);
    for (uint32_t k = head + 4 * nw + lane; k < n; k += 64) dst[k] = src[k];
}

// One BGZF block of in[0, n), n <= 0xff00, into out[0, cap): level 0 a stored block, level 1 LZ77 + dynamic Huffman codes unless the
// stored form is not larger.  `out` 4-byte aligned, cap >= 18 + 5 + n + 8 (anything less is DEF_ERR_SLOT, nothing written).
// tok: DEF_TOK_UNITS 16-bit units of global memory of this wave's own (level 1); crc_tab: crc32_table_entry[256] in LDS.
// Wave-uniform call; every lane returns the same code and *size.
template <class Prim>
PLO_DEV int bgzf_deflate_block(const Prim &prim, DefWork &ws, const uint32_t *crc_tab, const uint8_t *in, uint32_t n, uint8_t *out, uint32_t cap, int level,
                               uint16_t *tok, uint32_t *size) {
    constexpr unsigned long long CLO_LO = 16ull | (17ull << 5) | (18ull << 10) | (0ull << 15) | (8ull << 20) | (7ull << 25) | (9ull << 30) | (6ull << 35) |
                                          (10ull << 40) | (5ull << 45) | (11ull << 50) | (4ull << 55);
    constexpr unsigned long long CLO_HI = 12ull | (3ull << 5) | (13ull << 10) | (2ull << 15) | (14ull << 20) | (1ull << 25) | (15ull << 30);
    const int lane = wv::lane();
    *size = 0;
    if (n > DEF_MAX_IN) return DEF_ERR_LENGTH;
    if ((uintptr_t)out & 3u) return DEF_ERR_ALIGN;
    if (cap < 18 + 5 + n + 8) return DEF_ERR_SLOT;
    const uint32_t crc = n ? crc32_wave(in, n, crc_tab) : 0u;

    uint32_t tc = 0, hlit = 257, hdist = 1, hclen = 4, nh = 0, bits = 0;
    bool stored = level == 0;
    if (!stored) {
        tc = def_tokenize(prim, ws, in, n, tok);
        def_build_code(prim, ws, ws.lfreq, 286, 15, ws.llen, ws.lcode);
        def_build_code(prim, ws, ws.dfreq, 30, 15, ws.dlen, ws.dcode);
        // the code lengths, run-length coded (RFC 1951, 3.2.7)
        if (lane < 20) ws.cfreq[lane] = 0;
        wv::sync();
        uint32_t hdr[3] = {0, 0, 0};
        if (lane == 0) {
            uint32_t nl = 286, nd = 30;
            while (nl > 257 && ws.llen[nl - 1] == 0) --nl;
            while (nd > 1 && ws.dlen[nd - 1] == 0) --nd;
            const uint32_t N = nl + nd;
            auto L = [&](uint32_t i) -> uint32_t { return i < nl ? ws.llen[i] : ws.dlen[i - nl]; };
            uint32_t i = 0, k = 0;
            while (i < N) {
                const uint32_t v = L(i);
                uint32_t run = 1;
                while (i + run < N && run < 138 && L(i + run) == v) ++run;
                uint32_t sym, ev = 0, adv;
                if (v == 0 && run >= 11) sym = 18, ev = run - 11, adv = run;
                else if (v == 0 && run >= 3) sym = 17, ev = run - 3, adv = run;
                else sym = v, adv = 1;
                ws.t.hseq[k++] = (uint16_t)(sym | (ev << 8));
                ws.cfreq[sym]++;
                i += adv;
                if (v != 0 && run >= 4) {  // the length just written, 3 .. 6 more times
                    const uint32_t r = run - 1 < 6 ? run - 1 : 6;
                    ws.t.hseq[k++] = (uint16_t)(16u | ((r - 3) << 8));
                    ws.cfreq[16]++;
                    i += r;
                }
            }
            hdr[0] = nl, hdr[1] = nd, hdr[2] = k;
        }
        hlit = (uint32_t)wv::bcast_first((int)hdr[0]);
        hdist = (uint32_t)wv::bcast_first((int)hdr[1]);
        nh = (uint32_t)wv::bcast_first((int)hdr[2]);
        wv::sync();
        def_build_code(prim, ws, ws.cfreq, 19, 7, ws.clen, ws.ccode);
        hclen = 19;
        while (hclen > 4) {
            const uint32_t at = (uint32_t)(((hclen - 1 < 12 ? CLO_LO >> (5 * (hclen - 1)) : CLO_HI >> (5 * (hclen - 1 - 12)))) & 31ull);
            if (ws.clen[at]) break;
            --hclen;
        }
        // the size of the dynamic block
        int part = 0;
        for (uint32_t s = (uint32_t)lane; s < 286; s += 64) part += (int)(ws.lfreq[s] * (ws.llen[s] + (s > 256 ? def_len_extra(s - 257) : 0u)));
        if (lane < 30) part += (int)(ws.dfreq[lane] * (ws.dlen[lane] + def_dist_extra((uint32_t)lane)));
        if (lane < 19) part += (int)(ws.cfreq[lane] * (ws.clen[lane] + (lane == 16 ? 2u : (lane == 17 ? 3u : (lane == 18 ? 7u : 0u)))));
        bits = 3 + 14 + 3 * hclen + (uint32_t)wv::reduce_add(part);
        if ((bits + 7) / 8 >= 5 + n) stored = true;
    }

    if (stored) {
        const uint32_t bsize = 18 + 5 + n + 8 - 1;
        if (lane < 23) {
            const unsigned long long h0 = 0x0000000004088b1full, h1 = 0x000243420006ff00ull;  // 1f 8b 08 04 00 00 00 00 | 00 ff 06 00 'B' 'C' 02 00
            uint32_t b;
            if (lane < 8) b = (uint32_t)(h0 >> (8 * lane));
            else if (lane < 16) b = (uint32_t)(h1 >> (8 * (lane - 8)));
            else if (lane < 18) b = bsize >> (8 * (lane - 16));
            else if (lane == 18) b = 1;  // final stored block
            else if (lane < 21) b = n >> (8 * (lane - 19));
            else b = (~n) >> (8 * (lane - 21));
            out[lane] = (uint8_t)b;
        }
        def_copy(out + 23, in, n);
        if (lane < 8) out[23 + n + (uint32_t)lane] = (uint8_t)((lane < 4 ? crc : n) >> (8 * (lane & 3)));
        *size = bsize + 1;
        return DEF_OK;
    }

    const uint32_t clen = (bits + 7) / 8, total = 18 + clen + 8;  // < 18 + 5 + n + 8 <= cap
    if (lane < 16) {
        const unsigned long long h0 = 0x0000000004088b1full, h1 = 0x000243420006ff00ull;
        out[lane] = (uint8_t)((lane < 8 ? h0 >> (8 * lane) : h1 >> (8 * (lane - 8))));
    }
    for (uint32_t k = (uint32_t)lane; k < DEF_OBUF_WORDS; k += 64) ws.obuf[k] = 0;
    wv::sync();
    DefBits st;
    st.out32 = (uint32_t *)(out + 16);
    st.cap_words = (cap - 16) / 4;
    {   // BSIZE, the block header, the code lengths of the code-length code in their order
        unsigned long long v = 0;
        uint32_t nb = 0;
        if (lane == 0) v = total - 1, nb = 16;
        else if (lane == 1) v = 1u | (2u << 1), nb = 3;  // BFINAL, BTYPE = dynamic
        else if (lane == 2) v = hlit - 257, nb = 5;
        else if (lane == 3) v = hdist - 1, nb = 5;
        else if (lane == 4) v = hclen - 4, nb = 4;
        else if ((uint32_t)lane < 5 + hclen) {
            const uint32_t i = (uint32_t)lane - 5;
            v = ws.clen[(uint32_t)(((i < 12 ? CLO_LO >> (5 * i) : CLO_HI >> (5 * (i - 12)))) & 31ull)];
            nb = 3;
        }
        def_put(ws, st, v, nb);
    }
    for (uint32_t b0 = 0; b0 < nh; b0 += 64) {
        unsigned long long v = 0;
        uint32_t nb = 0;
        const uint32_t i = b0 + (uint32_t)lane;
        if (i < nh) {
            const uint32_t e = ws.t.hseq[i], sym = e & 0xffu, l = ws.clen[sym];
            v = (unsigned long long)ws.ccode[sym] | ((unsigned long long)(e >> 8) << l);
            nb = l + (sym == 16 ? 2u : (sym == 17 ? 3u : (sym == 18 ? 7u : 0u)));
        }
        def_put(ws, st, v, nb);
    }
    uint32_t prev_last = 0;  // the unit in front of the round's first: a match's first unit has bit 15, its second never
    for (uint32_t b0 = 0; b0 < tc; b0 += 64) {
        const uint32_t i = b0 + (uint32_t)lane;
        const uint32_t u = i < tc ? prim.load_written(tok + i) : 0u;
        const uint32_t before = (uint32_t)wv::shfl_up1((int)u, (int)prev_last);
        prev_last = (uint32_t)wv::bcast_last((int)u);
        unsigned long long v = 0;
        uint32_t nb = 0;
        if (i < tc && !(before & 0x8000u)) {
            if (u & 0x8000u) {
                const uint32_t len = (u & 0xffu) + 3, dist = (i + 1 < tc ? prim.load_written(tok + i + 1) : 0u) + 1;
                uint32_t lc, le, lv, dc, de, dv;
                def_len_code(len, lc, le, lv);
                def_dist_code(dist, dc, de, dv);
                const uint32_t ll = ws.llen[257 + lc], dl = ws.dlen[dc];
                v = (unsigned long long)ws.lcode[257 + lc] | ((unsigned long long)lv << ll) | ((unsigned long long)ws.dcode[dc] << (ll + le)) |
                    ((unsigned long long)dv << (ll + le + dl));
                nb = ll + le + dl + de;
            } else {
                v = ws.lcode[u];
                nb = ws.llen[u];
            }
        }
        def_put(ws, st, v, nb);
    }
    def_put(ws, st, lane == 0 ? ws.lcode[256] : 0u, lane == 0 ? ws.llen[256] : 0u);
    if (st.bitpos != 16 + bits) return DEF_ERR_INTERNAL;  // (the size was computed from the same counts and lengths)
    // the bytes of the open word, CRC-32, ISIZE
    const uint32_t done = (st.bitpos >> 5) * 4, rem = 18 + clen - (16 + done);
    if ((uint32_t)lane < rem) out[16 + done + (uint32_t)lane] = (uint8_t)(ws.obuf[0] >> (8 * lane));
    if (lane < 8) out[18 + clen + (uint32_t)lane] = (uint8_t)((lane < 4 ? crc : n) >> (8 * (lane & 3)));
    wv::sync();
    *size = total;
    return DEF_OK;
}

}  // namespace plo
