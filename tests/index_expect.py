"""What plo_records_index_dev, the writer's index and plo_bam_merge_runs_indexed must produce, restated from the definitions in
include/portello_liftover.h and include/portello_bam.h (and SAMv1 5.2 / 5.3) in plain Python -- not derived from the code under test:
the entry of a record, the lowest record the device refuses, the .bai bytes from entries and a block table, a BAI parser, and a region
query through an index (reg2bins, the linear index's lower bound, records read from virtual offsets with zlib).
TEST INFRASTRUCTURE ONLY."""
import struct
import zlib

import numpy as np

ERR_OFFSET, ERR_SHORT, ERR_BLOCK, ERR_REFID, ERR_POS, ERR_CIGAR, ERR_END, ERR_ORDER = 1, 2, 3, 4, 5, 6, 7, 8
POS_MAX = (1 << 31) - 2
MAX_END = 1 << 29
BIN_UNPLACED, BIN_META = 4680, 37450
REF_OPS = (0, 2, 3, 7, 8)  # M D N = X
ENTRY = np.dtype([("off", "<u8"), ("ref_id", "<i4"), ("beg", "<i4"), ("end", "<i4"), ("flags", "<u4")])
assert ENTRY.itemsize == 24


def op(length, code):
    return (length << 4) | code


def make_record(ref, pos, flag=0, name=b"", cigar=(), payload=b"", n_cigar=None, block_size=None):
    """block_size + the fixed fields + name + the CIGAR words + payload; n_cigar / block_size: the fields, when they shall lie"""
    body = struct.pack("<iiBBHHHIiii", ref, pos, len(name), 0, 0, len(cigar) if n_cigar is None else n_cigar, flag, 0, -1, -1, 0) + name
    body += struct.pack("<%dI" % len(cigar), *cigar) + payload
    return struct.pack("<I", len(body) if block_size is None else block_size) + body


def concat(records):
    off = np.zeros(len(records) + 1, np.uint64)
    if records:
        off[1:] = np.cumsum([len(r) for r in records], dtype=np.uint64)
    return b"".join(records), off


def reg2bin(beg, end):
    end -= 1
    for shift, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
        if beg >> shift == end >> shift:
            return base + (beg >> shift)
    return 0


def reg2bins(beg, end):
    end -= 1
    out = [0]
    for shift, base in ((26, 1), (23, 9), (20, 73), (17, 585), (14, 4681)):
        out += list(range(base + (beg >> shift), base + (end >> shift) + 1))
    return out


def fields(rec):
    ref, pos, lrn, _mapq, _bin, ncig, flag = struct.unpack_from("<iiBBHHH", rec, 4)
    return ref, pos, lrn, ncig, flag


def interval(rec):
    """(ref, beg, end, unmapped flag) by the rule; end may pass 2^29.  The CIGAR must lie inside rec."""
    ref, pos, lrn, ncig, flag = fields(rec)
    unm = (flag >> 2) & 1
    if ref < 0:
        return -1, -1, 0, unm
    ops = struct.unpack_from("<%dI" % ncig, rec, 36 + lrn)
    rlen = sum(o >> 4 for o in ops if (o & 15) in REF_OPS)
    beg = max(pos, 0)
    return ref, beg, (beg + 1 if unm or rlen == 0 else beg + rlen), unm


def entry_of(rec, off):
    ref, beg, end, unm = interval(rec)
    return (off, ref, beg, end, unm | ((BIN_UNPLACED if ref < 0 else reg2bin(beg, end)) << 16))


def first_offender(data, off, n_ref):
    """(record, kind) of the lowest record plo_records_index_dev refuses, or None"""
    n, n_bytes = len(off) - 1, len(data)
    prev = None  # (ref', pos) of the record in front when that record's fixed fields could be trusted
    for i in range(n):
        a, b = int(off[i]), int(off[i + 1])
        if (i == 0 and a != 0) or b < a or b > n_bytes or (i == n - 1 and b != n_bytes):
            return i, ERR_OFFSET
        if b - a < 36:
            return i, ERR_SHORT
        rec = data[a:b]
        if struct.unpack_from("<I", rec, 0)[0] + 4 != b - a:
            return i, ERR_BLOCK
        ref, pos, lrn, ncig, flag = fields(rec)
        if not -1 <= ref < n_ref:
            return i, ERR_REFID
        if not -1 <= pos <= POS_MAX:
            return i, ERR_POS
        if 36 + lrn + 4 * ncig > b - a:
            return i, ERR_CIGAR
        if interval(rec)[2] > MAX_END:
            return i, ERR_END
        cur = (n_ref if ref < 0 else ref, pos)
        if prev is not None and cur < prev:
            return i, ERR_ORDER
        prev = cur
    return None


def entries(data, off):
    """the entries of a buffer every record of which is accepted, as an ENTRY array"""
    n = len(off) - 1
    out = np.zeros(n, ENTRY)
    for i in range(n):
        out[i] = entry_of(data[int(off[i]):int(off[i + 1])], int(off[i]))
    return out


def split_records(data):
    out, at = [], 0
    while at < len(data):
        bs = struct.unpack_from("<I", data, at)[0]
        out.append(data[at:at + 4 + bs])
        at += 4 + bs
    assert at == len(data)
    return out


# ---- the file ---------------------------------------------------------------------------------------------------------------------------

def bgzf_blocks(blob):
    """[(file offset, block size, inflated bytes)] of a BGZF file, the EOF block included"""
    out, at = [], 0
    while at < len(blob):
        assert blob[at:at + 4] == b"\x1f\x8b\x08\x04" and blob[at + 12:at + 16] == b"BC\x02\x00"
        bs = struct.unpack_from("<H", blob, at + 16)[0] + 1
        raw = zlib.decompressobj(-15).decompress(blob[at + 18:at + bs - 8])
        assert len(raw) == struct.unpack_from("<I", blob, at + bs - 4)[0] and zlib.crc32(raw) == struct.unpack_from("<I", blob, at + bs - 8)[0]
        out.append((at, bs, raw))
        at += bs
    return out


def bam_layout(blob):
    """a BAM file whose header ends its own block(s) -> (records, block table [(record-stream offset, file offset)], file offset of the EOF
    block, n_ref).  The record stream is what follows the header; the EOF block is no entry of the table."""
    blocks = bgzf_blocks(blob)
    assert blocks and blocks[-1][1] == 28 and blocks[-1][2] == b""
    head = b""
    k = 0
    while True:  # the header's blocks
        head += blocks[k][2]
        k += 1
        if len(head) >= 12:
            lt = struct.unpack_from("<I", head, 4)[0]
            if len(head) >= 12 + lt:
                n_ref = struct.unpack_from("<I", head, 8 + lt)[0]
                at, ok = 12 + lt, True
                for _ in range(n_ref):
                    if len(head) < at + 4:
                        ok = False
                        break
                    at += 4 + struct.unpack_from("<I", head, at)[0] + 4
                if ok and len(head) >= at:
                    assert len(head) == at, "the header does not end its block"
                    break
    table, stream = [], b""
    for fo, _bs, raw in blocks[k:-1]:
        table.append((len(stream), fo))
        stream += raw
    return split_records(stream), table, blocks[-1][0], n_ref


def bai_bytes(ents, stream_len, table, eof_off, n_ref):
    """the .bai of records with the entries `ents` (offsets in the record stream) written in the blocks of `table`"""
    starts = [t[0] for t in table]

    def voff(o):
        if o >= stream_len:
            return eof_off << 16
        k = max(j for j in range(len(starts)) if starts[j] <= o)  # the last block that starts at or before o
        return (table[k][1] << 16) | (o - starts[k])

    n = len(ents)
    nxt = [int(ents[i + 1]["off"]) if i + 1 < n else stream_len for i in range(n)]
    out = b"BAI\x01" + struct.pack("<I", n_ref)
    for r in range(n_ref):
        mine = [i for i in range(n) if int(ents[i]["ref_id"]) == r]
        if not mine:
            out += struct.pack("<II", 0, 0)
            continue
        bins, lin, last_bin, counts = {}, {}, None, [0, 0]
        for i in mine:
            e = ents[i]
            beg, end = int(e["beg"]), int(e["end"])
            b = reg2bin(beg, end)
            v0, v1 = voff(int(e["off"])), voff(nxt[i])
            if b == last_bin:
                bins[b][-1][1] = v1
            else:
                bins.setdefault(b, []).append([v0, v1])
            last_bin = b
            counts[int(e["flags"]) & 1] += 1
            for w in range(beg >> 14, ((end - 1) >> 14) + 1):
                lin.setdefault(w, v0)
        out += struct.pack("<I", len(bins) + 1)
        for b in sorted(bins):
            out += struct.pack("<II", b, len(bins[b])) + b"".join(struct.pack("<QQ", *c) for c in bins[b])
        out += struct.pack("<IIQQQQ", BIN_META, 2, voff(int(ents[mine[0]]["off"])), voff(nxt[mine[-1]]), counts[0], counts[1])
        n_intv = max(lin) + 1
        vals, fill = [0] * n_intv, None
        for w in range(n_intv - 1, -1, -1):
            fill = lin.get(w, fill)
            vals[w] = fill
        out += struct.pack("<I", n_intv) + struct.pack("<%dQ" % n_intv, *vals)
    return out + struct.pack("<Q", sum(1 for i in range(n) if int(ents[i]["ref_id"]) < 0))


def expected_bai(blob):
    """the .bai of a BAM file, from its bytes alone"""
    recs, table, eof_off, n_ref = bam_layout(blob)
    data, off = concat(recs)
    assert first_offender(data, off, n_ref) is None
    return bai_bytes(entries(data, off), len(data), table, eof_off, n_ref)


def parse_bai(b):
    """-> (refs [dict(bins {bin: [(beg, end)]}, meta [(..), (..)] or None, linear [..])], n_no_coor); every byte is consumed"""
    assert b[:4] == b"BAI\x01"
    n_ref, at, refs = struct.unpack_from("<I", b, 4)[0], 8, []
    for _ in range(n_ref):
        n_bin = struct.unpack_from("<I", b, at)[0]
        at += 4
        bins, meta = {}, None
        for _ in range(n_bin):
            bn, nc = struct.unpack_from("<II", b, at)
            at += 8
            ch = [struct.unpack_from("<QQ", b, at + 16 * c) for c in range(nc)]
            at += 16 * nc
            if bn == BIN_META:
                meta = ch
            else:
                assert bn not in bins
                bins[bn] = ch
        n_intv = struct.unpack_from("<I", b, at)[0]
        lin = list(struct.unpack_from("<%dQ" % n_intv, b, at + 4))
        at += 4 + 8 * n_intv
        refs.append({"bins": bins, "meta": meta, "linear": lin})
    n_no_coor = struct.unpack_from("<Q", b, at)[0]
    assert at + 8 == len(b)
    return refs, n_no_coor


class BgzfFile:
    """records of a BAM file from a virtual offset on"""

    def __init__(self, blob):
        self.blob, self.cache = blob, {}

    def block(self, fo):
        if fo not in self.cache:
            bs = struct.unpack_from("<H", self.blob, fo + 16)[0] + 1
            self.cache[fo] = (zlib.decompressobj(-15).decompress(self.blob[fo + 18:fo + bs - 8]), fo + bs)
        return self.cache[fo]

    def read(self, v, n):
        """n bytes from virtual offset v -> (bytes, the virtual offset behind them)"""
        fo, uo, out = v >> 16, v & 0xffff, b""
        while True:
            raw, nxt = self.block(fo)
            take = raw[uo:uo + n - len(out)]
            out += take
            uo += len(take)
            if len(out) == n:
                if uo == len(raw):  # (the reader's tell() at a block's end is the next block's start)
                    fo, uo = nxt, 0
                return out, (fo << 16) | uo
            assert nxt < len(self.blob), "read past the end of the file"
            fo, uo = nxt, 0

    def records(self, v0, v1):
        """the records that START in [v0, v1) -> [(virtual offset, record)]"""
        out, v = [], v0
        if v & 0xffff == len(self.block(v >> 16)[0]) and v < v1:  # a chunk that begins at a block's very end
            v = self.block(v >> 16)[1] << 16
        while v < v1:
            head, _ = self.read(v, 4)
            rec, nv = self.read(v, 4 + struct.unpack("<I", head)[0])
            out.append((v, rec))
            v = nv
        return out


def query(blob, bai, ref, beg, end):
    """the records of the BAM `blob` that overlap [beg, end) on ref, found through the parsed index `bai`, in file order"""
    refs, _ = bai
    ix = refs[ref]
    if beg >= end or not ix["linear"]:
        return []
    w = beg >> 14
    min_off = ix["linear"][w] if w < len(ix["linear"]) else ix["linear"][-1]
    if w >= len(ix["linear"]):
        return []  # behind the last window a record of this reference touches
    chunks = sorted(c for b in reg2bins(beg, end) for c in ix["bins"].get(b, []) if c[1] > min_off)
    f, seen, out = BgzfFile(blob), set(), []
    for c0, c1 in chunks:
        for v, rec in f.records(c0, c1):
            r, rb, re_, _ = interval(rec)
            if v not in seen and r == ref and rb < end and re_ > beg:
                seen.add(v)
                out.append((v, rec))
    return [rec for _, rec in sorted(out)]


def brute(recs, ref, beg, end):
    """the same set by looking at every record"""
    if beg >= end:
        return []
    return [r for r in recs if interval(r)[0] == ref and interval(r)[1] < end and interval(r)[2] > beg]
