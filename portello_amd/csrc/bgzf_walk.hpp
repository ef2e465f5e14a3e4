// bgzf_walk.hpp -- the host's walk over the BGZF block headers of plo_bgzf_inflate_dev: the rules of BgzfIn::bgzf_block_at / BgzfIn::fill
// (bam_internal.hpp: gzip magic with FEXTRA, the `BC` subfield, BSIZE, the ISIZE trailer, ISIZE <= 65536).  Host code without a device
// part: the engine and the test harness (tests/emu/emu_cut.cpp) both include it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace plo {

struct BgzfWalkBlk {
    uint64_t off;         // the block's first byte inside the buffer
    uint64_t coff, clen;  // its deflate data
    uint64_t uoff, ulen;  // its inflated bytes inside the packed output
    uint32_t crc;
};
enum { BGZF_WALK_OK = 0, BGZF_WALK_NOT_A_HEADER = 1, BGZF_WALK_CORRUPT = 2, BGZF_WALK_TOO_LARGE = 3 };

// Every whole block of b[0, n) whose inflated bytes still fit into `cap`.  *consumed: where the first block that was not taken starts (a
// partial one, or one that no longer fits).  A failure's *consumed is the offset of the offending block.
// A part of a file (plo_bgzf_inflate_part_dev): b[0] lies at `file_off` of its file and the part ends at `range_end`; *own_bytes is the
// inflated offset of the first block taken whose file offset is >= range_end, *n_bytes when there is none (BgzfIn::block_file_off: a byte
// belongs to the last block that starts at or before it, so a block with ISIZE 0 at the border changes nothing).
inline int bgzf_walk(const uint8_t *b, size_t n, uint64_t cap, std::vector<BgzfWalkBlk> &out, uint64_t *consumed, uint64_t *n_bytes, uint64_t file_off = 0,
                     uint64_t range_end = UINT64_MAX, uint64_t *own_bytes = nullptr) {
    auto rd16 = [](const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); };
    auto rd32 = [](const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); };
    size_t c = 0;
    uint64_t u = 0, own = UINT64_MAX;
    out.clear();
    int rc = BGZF_WALK_OK;
    while (c < n) {
        const uint8_t *h = b + c;
        const size_t left = n - c;
        // (what is there of the magic is checked even where the block is cut short: garbage is an error, not a partial block)
        static const uint8_t magic[3] = {0x1f, 0x8b, 8};
        bool bad = false;
        for (size_t k = 0; k < 3 && k < left; ++k) bad = bad || h[k] != magic[k];
        if (left > 3 && !(h[3] & 4)) bad = true;
        if (bad) {
            rc = BGZF_WALK_NOT_A_HEADER;
            break;
        }
        if (left < 28) break;  // a partial block
        const uint32_t xlen = rd16(h + 10);
        if (12 + (size_t)xlen > left) break;
        uint32_t bsize = 0;
        for (uint32_t x = 0; x + 4 <= xlen;) {
            const uint8_t *e = h + 12 + x;
            const uint32_t slen = rd16(e + 2);
            if (e[0] == 'B' && e[1] == 'C' && slen == 2 && x + 6 <= xlen) bsize = rd16(e + 4) + 1;
            x += 4 + slen;
        }
        if (bsize < 12 + xlen + 8) {
            rc = BGZF_WALK_CORRUPT;
            break;
        }
        if (bsize > left) break;  // a partial block
        BgzfWalkBlk k;
        k.off = c;
        k.coff = c + 12 + xlen;
        k.clen = bsize - 12 - xlen - 8;
        k.crc = rd32(h + bsize - 8);
        k.ulen = rd32(h + bsize - 4);
        k.uoff = u;
        if (k.ulen > 65536) {
            rc = BGZF_WALK_TOO_LARGE;
            break;
        }
        if (u + k.ulen > cap) break;  // no longer fits
        if (own == UINT64_MAX && range_end != UINT64_MAX && (file_off > range_end || c >= range_end - file_off)) own = u;
        u += k.ulen;
        c += bsize;
        out.push_back(k);
    }
    *consumed = c;
    *n_bytes = u;
    if (own_bytes) *own_bytes = own == UINT64_MAX ? u : own;
    return rc;
}

}  // namespace plo
