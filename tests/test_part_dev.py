"""Parts of a BAM file on the device (API 11): plo_part_start_dev, plo_bgzf_inflate_part_dev's own_bytes, plo_window_cut_part_dev and
devreader.DeviceBamReader(part, n_parts).  The oracle is the host reader, bam.BamReader(part=, n_parts=) / plo_bam_open_range.  CPU: the
device code under the wave emulator (tests/emu/emu_part.cpp) against part_start_ref / host_loop below, restatements of the host's loops that
first prove themselves against the host reader on files of tiny BGZF blocks (payloads cut at 20-400 bytes, ISIZE-0 blocks in the middle);
the reader's own logic with zlib and the emulator standing in for the device.  GPU: the calls and the reader against the host reader, and
run_bam_to_bam(device_input=True, part=i, n_parts=3)."""
import contextlib
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

import emu_cut_lib as ecl
import emu_part_lib as epl
from emu_cut_lib import Cut
from portello_amd import abi, api, bam, bamsynth, devreader, synth

NAMES = ["ctgA", "ctgB"]
OK, IO, DATA = abi.PLO_OK, abi.PLO_ERR_IO, abi.PLO_ERR_DATA
FOUND, NEED_MORE, NONE = abi.PART_FOUND, abi.PART_NEED_MORE, abi.PART_NONE
NO_END = abi.NO_RANGE_END


# ---- records and streams (the helpers of test_window_cut_dev.py) ------------------------------------------------------------------------------

def rec(total, cls="p", k=0, qual=None, l_seq=None, tid=None):
    """a record of exactly `total` bytes (block_size word included, total >= 39): cls p(rimary) / u(nmapped) / s(upplementary)"""
    name = b"r%d" % (k % 10) + b"\0"
    body = total - 4 - 32 - len(name)
    if l_seq is None:
        l_seq = (2 * body) // 3
        while (l_seq + 1) // 2 + l_seq > body:
            l_seq -= 1
    pad = body - (l_seq + 1) // 2 - l_seq
    assert pad >= 0
    flag, t = {"p": (0, 0), "u": (4, -1), "s": (0x800, 1)}[cls]
    t = t if tid is None else tid
    q = bytes([k % 40] * l_seq) if qual is None else qual
    b = struct.pack("<iiBBHHHIiii", t, 100 + k, len(name), 30, 4680, 0, flag, l_seq, -1, -1, 0) + name + bytes([0x12] * ((l_seq + 1) // 2)) + q + b"\x00" * pad
    assert len(b) == total - 4
    return struct.pack("<I", len(b)) + b


def mixed(n, seed, lo=39, hi=300, classes="pppppus", k0=0):
    rng = np.random.default_rng(seed)
    return b"".join(rec(int(rng.integers(lo, hi)), classes[int(rng.integers(0, len(classes)))], k0 + k) for k in range(n))


def rec_starts(stream):
    at, out = 0, []
    while at < len(stream):
        out.append(at)
        at += 4 + struct.unpack_from("<I", stream, at)[0]
    assert at == len(stream)
    return out


def host_loop(stream, max_records, final, max_unmapped=0, max_bytes=0, own_bytes=NO_END):
    """plo_bam_read_window's loop (bam_host.cpp:257-297) over bytes in memory, the range test (:268) included"""
    n, at, reads, unm = len(stream), 0, [], []
    max_unmapped = max_unmapped or 4 * max_records + 1024
    max_bytes = max_bytes or max(1 << 30, min(8 << 30, max_records << 16))
    ended = abi.CUT_MAX_RECORDS
    while len(reads) < max_records:
        if len(unm) >= max_unmapped:
            ended = abi.CUT_MAX_UNMAPPED
            break
        if at >= max_bytes and reads + unm:
            ended = abi.CUT_MAX_BYTES
            break
        if at == n:
            ended = abi.CUT_EOF if final else abi.CUT_END_OF_BYTES
            break
        if n - at < 4:
            if final:
                return Cut(IO, err_off=at)
            ended = abi.CUT_END_OF_BYTES
            break
        if at >= own_bytes:
            ended = abi.CUT_PART_END
            break
        bs = struct.unpack_from("<I", stream, at)[0]
        if bs < 32:
            return Cut(IO, err_off=at)
        if n - at < 4 + bs:
            if final:
                return Cut(IO, err_off=at)
            ended = abi.CUT_END_OF_BYTES
            break
        tid, _, lq, _, _, ncg, flag, lseq = struct.unpack_from("<iiBBHHHI", stream, at + 4)
        if 32 + lq + 4 * ncg + ((lseq + 1) & 0xFFFFFFFF) // 2 + lseq > bs:
            return Cut(IO, err_off=at)
        if flag & 4 and tid >= 0:
            return Cut(DATA, err_off=at)
        if flag & 4:
            unm.append(at)
        elif not flag & 0x800:
            reads.append(at)
        at += 4 + bs
    ub = b"".join(stream[u:u + 4 + struct.unpack_from("<I", stream, u)[0]] for u in unm)
    return Cut(OK, len(reads), reads, len(unm), ub, None, at, ended)


def plausible(b, q, n_ref):
    """plausible_record (bam_host.cpp:113-130) at b[q:]: the record's length or None"""
    left = len(b) - q
    if left < 36:
        return None
    bs = struct.unpack_from("<I", b, q)[0]
    if bs < 32 or 4 + bs > left:
        return None
    tid, _, lq, _, _, ncg, _, lseq, mtid = struct.unpack_from("<iiBBHHHIi", b, q + 4)
    nr = n_ref if n_ref < (1 << 31) else n_ref - (1 << 32)
    if tid < -1 or tid >= nr or mtid < -1 or mtid >= nr:
        return None
    if lq < 1 or 32 + lq + 4 * ncg + ((lseq + 1) & 0xFFFFFFFF) // 2 + lseq > bs:
        return None
    if b[q + 36 + lq - 1] != 0:
        return None
    for i in range(ncg):
        if b[q + 36 + lq + 4 * i] & 15 > 8:
            return None
    return 4 + bs


def part_start_ref(b, n_ref, final):
    """the loop of plo_bam_open_range (bam_host.cpp:183-202) with have = len(b) and eof = final -> (kind, first_off or None)"""
    have = len(b)
    for p in range(0, have - 35):
        q, ok, ran_out = p, 0, False
        while ok < 8:
            if q == have and final:
                break
            ln = plausible(b, q, n_ref)
            if ln is None:
                ran_out = q + 36 > have or (q + 4 <= have and 4 + struct.unpack_from("<I", b, q)[0] > have - q and struct.unpack_from("<I", b, q)[0] >= 32)
                break
            q += ln
            ok += 1
        if ok == 8 or (ok > 0 and q == have and final):
            return FOUND, p
        if ran_out and not final and ok > 0:
            return NEED_MORE, None
    return NONE, None


# ---- files of tiny BGZF blocks ----------------------------------------------------------------------------------------------------------------

def bgzf_block(payload: bytes) -> bytes:
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    d = co.compress(payload) + co.flush()
    return (b"\x1f\x8b\x08\x04" + bytes(6) + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, len(d) + 25) + d +
            struct.pack("<II", zlib.crc32(payload) & 0xFFFFFFFF, len(payload)))


def bam_header(names=NAMES, text=b"@HD\tVN:1.6\n"):
    h = b"BAM\x01" + struct.pack("<I", len(text)) + text + struct.pack("<I", len(names))
    for n in names:
        h += struct.pack("<I", len(n) + 1) + n.encode() + b"\0" + struct.pack("<I", 500000)
    return h


class TinyBam:
    """a BAM file written block by block: payloads of 20-400 bytes cut anywhere (the header's last block holds the first records' bytes),
    ISIZE-0 blocks in the middle with probability p_empty, the EOF block at the end.  blocks: (file offset, size, inflated offset, ISIZE)"""

    def __init__(self, path, stream, seed, p_empty=0.15, lo=20, hi=401):
        rng = np.random.default_rng(seed)
        self.path, self.stream, self.hdr = path, stream, bam_header()
        plain, at, data, self.blocks = self.hdr + stream, 0, b"", []
        while at < len(plain):
            if rng.random() < p_empty:
                self.blocks.append((len(data), 28, at, 0))
                data += bgzf_block(b"")
            n = min(int(rng.integers(lo, hi)), len(plain) - at)
            blk = bgzf_block(plain[at:at + n])
            self.blocks.append((len(data), len(blk), at, n))
            data += blk
            at += n
        self.blocks.append((len(data), 28, at, 0))
        data += bgzf_block(b"")
        self.plain, self.data = plain, data
        with open(path, "wb") as fh:
            fh.write(data)

    def own_ref(self, range_end, first=0):
        """inflated offset (from block `first`'s) of the first block at or behind `first` whose file offset is >= range_end, the end otherwise"""
        for off, _, uoff, _ in self.blocks[first:]:
            if off >= range_end:
                return uoff - self.blocks[first][2]
        return len(self.plain) - self.blocks[first][2]

    def part_ref(self, part, n_parts):
        """[a, b) of the record stream that the part owns by the restatements: plo_bam_open_range's decisions over the known blocks,
        part_start_ref for the first record, own_ref for the end"""
        size, H = len(self.data), len(self.hdr)
        lo, hi = size * part // n_parts, size * (part + 1) // n_parts
        range_end = NO_END if part + 1 == n_parts else hi
        u = k = 0
        while k < len(self.blocks) and u + self.blocks[k][3] <= H:  # (the host's walk over the ISIZE trailers)
            u += self.blocks[k][3]
            k += 1
        if k == len(self.blocks) or hi <= self.blocks[k][0]:
            return None
        if lo <= self.blocks[k][0]:
            a = H
        else:
            k = next((j for j, b in enumerate(self.blocks) if b[0] >= lo), None)
            if k is None or self.blocks[k][0] >= hi:
                return None
            kind, off = part_start_ref(self.plain[self.blocks[k][2]:], len(NAMES), True)
            assert kind != NEED_MORE
            if kind == NONE:
                return None
            a = self.blocks[k][2] + off
        own = self.blocks[0][2] + self.own_ref(range_end)
        starts = [H + s for s in rec_starts(self.stream)]
        b = next((s for s in starts if s >= own), len(self.plain))
        return (a - H, b - H) if a < b else None


def host_part(path, part, n_parts, max_records, keep_empty=False):
    """the windows of bam.BamReader(part, n_parts): (Cut (ended_by: EOF or not), the window's bytes) per window; keep_empty: also a window
    of supplementary records only, which bam.BamReader.read_window does not hand out"""
    rd = bam.BamReader(path, 2, part=part, n_parts=n_parts)
    out = []
    while True:
        h = C.c_void_p()
        st = bam.lib().plo_bam_read_window(rd.handle, max_records, C.byref(h))
        assert st == OK
        w = bam.Window(h)
        raw = w.raw()
        ub, nu = w.unmapped_bytes()
        nr, nb = int(raw.n_reads), int(raw.raw_bytes)
        if nr or nu or (keep_empty and nb):
            out.append((Cut(OK, nr, [int(raw.read_rec_off[i]) for i in range(nr)], nu, ub, None, nb, abi.CUT_EOF if w.eof else -1),
                        bytes(bytearray(raw.raw[:nb]))))
        eof = w.eof
        w.close()
        if eof:
            break
    rd.close()
    return out


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("partdev")
    out = []
    for k, (n, seed) in enumerate(((60, 11), (25, 12), (9, 13), (1, 14))):
        out.append(TinyBam(str(d / f"t{k}.bam"), mixed(n, seed), seed + 100))
    return out


def part_counts(tb):
    return (1, 2, 3, 7, 4 * len(tb.blocks))


# ---- CPU: the restatements against the host reader ----------------------------------------------------------------------------------------------

def test_restatements_equal_the_host_reader_on_files(files):
    """part_start_ref, own_ref and the decisions of plo_bam_open_range as part_ref restates them: for every part of every split, the
    stretch of records they give is the stretch the host reader reads, and the parts tile the file"""
    n_later = 0
    for tb in files:
        assert any(b[3] == 0 for b in tb.blocks[:-1]) or len(tb.blocks) < 6
        for n_parts in part_counts(tb):
            at = 0
            for part in range(n_parts):
                want = tb.part_ref(part, n_parts)
                got = b"".join(raw for _, raw in host_part(tb.path, part, n_parts, 1000, keep_empty=True))
                if want is None:
                    assert got == b"", (n_parts, part)
                    continue
                assert got == tb.stream[want[0]:want[1]] and want[0] == at, (n_parts, part, want, at)
                n_later += part > 0
                at = want[1]
            assert at == len(tb.stream)
    assert n_later > 30


# ---- CPU: plo_part_start_dev under the emulator ---------------------------------------------------------------------------------------------------

def start_same(s, n_ref, final, what="", quick=False):
    want = part_start_ref(s, n_ref, final)
    for tile, oseed, tseed in ((128, 5, 0), (64, 3, 9)) if quick else ((64, 0, 0), (128, 5, 0), (64, 3, 9), (192, 7, 21)):
        assert epl.part_start(s, n_ref, final, tile, oseed, tseed) == want, (what, tile, oseed, tseed, want)
    return want


def in_quals(fakes, total, k=0):
    """a primary record of `total` bytes whose quality bytes begin with `fakes`, zeros behind them -> (record, offset of the fakes in it)"""
    body = total - 4 - 32 - 3
    l_seq = (2 * body) // 3
    while (l_seq + 1) // 2 + l_seq > body:
        l_seq -= 1
    assert len(fakes) <= l_seq
    r = rec(total, "p", k, qual=fakes + bytes(l_seq - len(fakes)))
    return r, 4 + 32 + 3 + (l_seq + 1) // 2


def test_part_start_inside_a_record():
    """streams that begin 1 .. len - 1 bytes into a record: the next record is the first one"""
    tail = mixed(10, 5, hi=120, k0=1)
    for first, step in ((rec(61, "p", 0), 1), (rec(147, "u", 0), 9)):
        for cut in range(1, len(first), step):
            s = first[cut:] + tail
            assert start_same(s, 2, True, cut, quick=True) == (FOUND, len(first) - cut)
    assert start_same(rec(140)[70:] + tail, 2, False) == (FOUND, 70)


def test_part_start_short_chains_and_the_end_of_the_bytes():
    first = rec(80)
    for n in range(0, 8):  # fewer than eight records left
        s = first[33:] + mixed(n, 20 + n, hi=90, k0=1)
        want = start_same(s, 2, True, n)
        assert want == ((FOUND, 47) if n else (NONE, None))
        # without `final` the chain is cut by the end of the bytes: the host buffers more
        assert start_same(s, 2, False, n) == ((NEED_MORE, None) if n else (NONE, None))
    s = first[33:] + mixed(8, 30, hi=90, k0=1)
    assert start_same(s, 2, False) == (FOUND, 47)
    full = first[33:] + mixed(3, 31, hi=90, k0=1)
    for drop in (1, 3, 4, 20, 36, 40):  # the last record cut short: inside its block_size word, its fixed fields, its body
        assert start_same(full[:-drop], 2, False, drop) == (NEED_MORE, None)
        assert start_same(full[:-drop], 2, True, drop)[0] == NONE  # (nothing follows: no chain ends at the end of the bytes)
    for n in (0, 1, 35, 36, 37):
        s = rec(60)[:n]
        assert start_same(s, 2, True, n) == (NONE, None) and start_same(s, 2, False, n) == (NONE, None)
    # one whole record and nothing else: a chain of one to the end with `final`, a cut without
    assert start_same(rec(36 + 3), 2, True) == (FOUND, 0) and start_same(rec(36 + 3), 2, False) == (NEED_MORE, None)


def test_part_start_decoys():
    tail = mixed(9, 40, hi=100, k0=3)
    # seven links pass, the eighth (the zeros behind them: block_size 0) fails
    big, fo = in_quals(b"".join(rec(40, "p", k) for k in range(7)), 600)
    s = big[10:] + tail
    assert part_start_ref(s[fo - 10:], 2, True)[1] != 0 and plausible(s, fo - 10, 2) == 40
    for final in (True, False):
        assert start_same(s, 2, final) == (FOUND, len(big) - 10)
    # eight links pass but for tid >= n_ref: what cut_plausible (the cut's guess) lets through and plausible_record does not
    big, fo = in_quals(b"".join(rec(40, "p", k, tid=2) for k in range(8)), 600)
    s = big[10:] + tail
    assert start_same(s, 2, True) == (FOUND, len(big) - 10)
    assert start_same(s, 3, True) == (FOUND, fo - 10)  # (with a third reference the same bytes ARE a chain)
    big, fo = in_quals(b"".join(rec(40, "p", k) for k in range(7)) + struct.pack("<IiiBBHHHIi", 36, 0, 0, 2, 0, 0, 0, 0, 0, 2) + b"x\0\0\0", 600)
    assert start_same(big[10:] + tail, 2, True) == (FOUND, len(big) - 10)  # (the eighth fails on its mate's reference id alone)
    assert start_same(big[10:] + tail, 3, True) == (FOUND, fo - 10)
    # a first candidate whose block_size runs beyond the bytes is a reject, not a cut: the chain behind it is found, `final` or not
    bogus = bytearray(rec(40))
    bogus[0:4] = struct.pack("<I", 0x7FFFFF00)
    s = bytes(bogus) + tail
    for final in (True, False):
        assert start_same(s, 2, final) == (FOUND, 40)
    bogus[0:4] = struct.pack("<I", 0xFFFFFFFF)
    assert start_same(bytes(bogus) + tail, 2, False) == (FOUND, 40)


def test_part_start_fuzz_with_shuffled_tiles():
    rng = np.random.default_rng(20261018)
    kinds = {FOUND: 0, NEED_MORE: 0, NONE: 0}
    for it in range(320):
        n = int(rng.integers(1, 13))
        s = bytearray(mixed(n, int(rng.integers(1 << 30)), hi=int(rng.choice([70, 160, 300]))))
        s = s[int(rng.integers(0, min(len(s), 200))):]
        roll = rng.random()
        if roll < 0.3 and len(s):
            for _ in range(int(rng.integers(1, 4))):
                s[int(rng.integers(0, len(s)))] = int(rng.integers(0, 256))
        elif roll < 0.55:
            s = s[:int(rng.integers(0, len(s) + 1))]
        s, final, n_ref = bytes(s), bool(rng.random() < 0.5), int(rng.choice([1, 2, 2, 5]))
        want = part_start_ref(s, n_ref, final)
        tile = int(rng.choice([64, 128, 256]))
        assert epl.part_start(s, n_ref, final, tile, it + 1, it + 1) == want, (it, tile, final, n_ref, want)
        if it % 4 == 0:
            assert epl.part_start(s, n_ref, final, tile, it + 1, 0) == want, (it, tile, final, n_ref, want)
        kinds[want[0]] += 1
    assert min(kinds.values()) > 25, kinds


# ---- CPU: own_bytes of the header walk -----------------------------------------------------------------------------------------------------------

def test_own_bytes_of_the_header_walk(tmp_path):
    """files of 1-40 blocks, every range_end at, just before and just behind each block's offset, the walk from the file's start and from a
    block in the middle; own_ref is what part_ref (proven against the host reader above) takes for the part's end"""
    n_empty_border = 0
    for nb_, seed in ((0, 1), (1, 2), (4, 3), (17, 4), (38, 5)):
        tb = TinyBam(str(tmp_path / f"o{nb_}.bam"), mixed(max(1, nb_ * 2), seed, hi=150)[:max(1, nb_ * 90)], seed, p_empty=0.3 if nb_ else 0.0, lo=60, hi=200)
        if nb_ == 0:
            tb.blocks, tb.data = tb.blocks[:1], tb.data[:tb.blocks[0][1]]
            tb.plain = tb.plain[:tb.blocks[0][3]]
        assert 1 <= len(tb.blocks) <= 40
        for first in sorted({0, len(tb.blocks) // 2}):
            f0 = tb.blocks[first][0]
            buf = tb.data[f0:]
            total = len(tb.plain) - tb.blocks[first][2]
            ends = sorted({max(0, off + dd) for off, _, _, _ in tb.blocks for dd in (-1, 0, 1)} | {len(tb.data), len(tb.data) + 1, NO_END})
            for re_ in ends:
                rc, used, nbytes, own, nblk = epl.bgzf_walk_part(buf, 1 << 30, f0, re_)
                assert (rc, used, nbytes, nblk) == (0, len(buf), total, len(tb.blocks) - first)
                assert own == tb.own_ref(re_, first), (nb_, first, re_)
                n_empty_border += any(b[0] == re_ and b[3] == 0 for b in tb.blocks[first:])
            # a buffer that ends inside a block, and a dst that ends early: own_bytes is n_bytes when the border was not reached
            k = (first + len(tb.blocks)) // 2
            if k > first:
                cut = tb.blocks[k][0] - f0 + 5
                rc, used, nbytes, own, nblk = epl.bgzf_walk_part(buf[:cut], 1 << 30, f0, tb.blocks[k][0])
                assert (rc, used, nblk, own) == (0, cut - 5, k - first, nbytes)
                rc, used, nbytes, own, nblk = epl.bgzf_walk_part(buf, tb.blocks[k][2] - tb.blocks[first][2], f0, tb.blocks[k][0])
                assert rc == 0 and own == nbytes <= tb.blocks[k][2] - tb.blocks[first][2]
        # the plain walk is unchanged by the new arguments
        assert ecl.bgzf_walk(tb.data, 1 << 30)[:3] == epl.bgzf_walk_part(tb.data, 1 << 30, 0, NO_END)[:3]
    assert n_empty_border > 5


# ---- CPU: plo_window_cut_part_dev under the emulator -------------------------------------------------------------------------------------------------

def emu(stream, seg, max_records, final, own_bytes, **kw):
    return epl.window_cut_part(stream, seg, max_records, final, own_bytes, order_seed=kw.pop("order_seed", 7), **kw)


def same(got: Cut, want: Cut, what=""):
    assert got.key() == want.key(), (what, got, want)
    if got.status == OK:
        assert got.unmapped_off[-1] == len(got.unmapped) and len(got.unmapped_off) == got.n_unmapped + 1


def cut_same(s, seg, mr, final, own, what="", **kw):
    want = host_loop(s, mr, final, own_bytes=own, **kw)
    same(emu(s, seg, mr, final, own, **kw), want, what)
    same(emu(s, seg, mr, final, own, no_guess=True, **kw), want, what)
    return want


def test_cut_part_range_test():
    seg = 128
    recs = [rec(60 + 7 * k, "ppus"[k % 4], k) for k in range(14)]
    s, starts = b"".join(recs), rec_starts(b"".join(recs))
    for final in (True, False):
        for k in (1, 5, 9, 13):
            # at a record boundary: that record is the next part's
            w = cut_same(s, seg, 100, final, starts[k], k)
            assert (w.status, w.ended_by, w.window_bytes) == (OK, abi.CUT_PART_END, starts[k])
            # inside a record: it belongs to the part, the next one does not
            for inside in (1, 4, 40):
                w = cut_same(s, seg, 100, final, starts[k] + inside, k)
                assert (w.ended_by, w.window_bytes) == (abi.CUT_PART_END, starts[k + 1]) if k + 1 < len(starts) else w.ended_by != abi.CUT_PART_END
        w = cut_same(s, seg, 100, final, 0)
        assert (w.n_reads, w.n_unmapped, w.window_bytes, w.ended_by) == (0, 0, 0, abi.CUT_PART_END)
        # beyond the stream, and no end at all: the plain cut
        for own in (len(s) + 1, len(s) + 1000, NO_END):
            w = cut_same(s, seg, 100, final, own)
            assert w.key() == ecl.window_cut(s, seg, 100, final, order_seed=7).key() and w.ended_by != abi.CUT_PART_END
        # own_bytes at the end of the bytes: the end of the bytes comes first (the host sees "no byte left" before the range test)
        assert cut_same(s, seg, 100, final, len(s)).ended_by == (abi.CUT_EOF if final else abi.CUT_END_OF_BYTES)
    # fewer than 4 bytes left at own_bytes: the host's "truncated" test stands in front of the range test
    assert cut_same(s + b"\x01\x02", seg, 100, True, len(s)).key() == (IO, len(s))
    assert cut_same(s + b"\x01\x02", seg, 100, False, len(s)).ended_by == abi.CUT_END_OF_BYTES
    assert cut_same(b"", seg, 5, True, 0).ended_by == abi.CUT_EOF


def _bad(kind):
    r = bytearray(rec(100, "p", 5))
    if kind == "bs0":
        r[0:4] = struct.pack("<I", 0)
    elif kind == "bs31":
        r[0:4] = struct.pack("<I", 31)
    elif kind == "layout":
        r[20:24] = struct.pack("<I", 90)
    elif kind == "unm_tid":
        r[18:20] = struct.pack("<H", 4)
    return bytes(r)


@pytest.mark.parametrize("kind,status", [("bs0", IO), ("bs31", IO), ("layout", IO), ("unm_tid", DATA), ("trunc", IO)])
def test_cut_part_refusals_behind_own_bytes(kind, status):
    """a refused record at or behind own_bytes never fails the part; one in front of it does"""
    seg = 128
    good = [rec(60 + 3 * k, "ppu"[k % 3], k) for k in range(9)]
    for where in (0, 4, 9):
        bad = rec(100, "p", 5)[:57] if kind == "trunc" else _bad(kind)
        s = b"".join(good[:where]) + bad + (b"" if kind == "trunc" else b"".join(good[where:]))
        off = sum(len(g) for g in good[:where])
        w = cut_same(s, seg, 100, True, off, (kind, where))  # AT own_bytes
        assert (w.status, w.ended_by, w.window_bytes) == (OK, abi.CUT_PART_END, off)
        if where:
            w = cut_same(s, seg, 100, True, off - 5, (kind, where))  # BEHIND it (own_bytes inside the record in front)
            assert (w.status, w.ended_by, w.window_bytes) == (OK, abi.CUT_PART_END, off)
            w = cut_same(s, seg, 100, True, sum(len(g) for g in good[:where - 1]), (kind, where))
            assert w.status == OK and w.window_bytes < off
        w = cut_same(s, seg, 100, True, off + 1, (kind, where))  # IN FRONT of own_bytes: the record is the part's and fails it
        assert (w.status, w.err_off) == (status, off)
        assert cut_same(s, seg, 100, True, NO_END, (kind, where)).key() == (status, off)


def test_cut_part_with_the_stop_rules():
    """MAX_RECORDS / MAX_UNMAPPED / MAX_BYTES come first, in the host's order"""
    seg = 128
    s = b"".join(rec(60 + k, "pppu"[k % 4], k) for k in range(24))
    starts = rec_starts(s)
    n_part_end = 0
    for own in (starts[4], starts[7] + 9, starts[23], len(s) + 5):
        for kw in ({}, {"max_unmapped": 1}, {"max_bytes": 1}, {"max_bytes": starts[12]}):
            for mr in (3, 4, 100):
                at = 0
                while True:  # window after window, own_bytes moving with the stream
                    w = host_loop(s[at:], mr, True, own_bytes=max(0, own - at), **kw)
                    same(emu(s[at:], seg, mr, True, max(0, own - at), **kw), w, (own, kw, mr, at))
                    assert w.status == OK
                    n_part_end += w.ended_by == abi.CUT_PART_END
                    if w.ended_by in (abi.CUT_PART_END, abi.CUT_EOF) or not (w.window_bytes or w.n_reads or w.n_unmapped):
                        break
                    at += w.window_bytes
                assert at + w.window_bytes == (min(x for x in starts + [len(s)] if x >= own) if w.ended_by == abi.CUT_PART_END else at + w.window_bytes)
    assert n_part_end > 30
    # the record count is tested first: a full window whose next record is the next part's ends with MAX_RECORDS
    only_p = b"".join(rec(50 + k, "p", k) for k in range(6))
    assert cut_same(only_p, seg, 3, True, rec_starts(only_p)[3]).ended_by == abi.CUT_MAX_RECORDS
    assert cut_same(only_p[rec_starts(only_p)[3]:], seg, 3, True, 0).ended_by == abi.CUT_PART_END


def test_cut_fuzz_without_an_end_equals_the_plain_cut():
    """every case of test_window_cut_dev.py's fuzz (the same generator and seed) with own_bytes = UINT64_MAX: the plain emulator cut; and
    with an end somewhere in the stream: the host loop with the range test"""
    rng = np.random.default_rng(20261017)
    rng2 = np.random.default_rng(5)
    n_err = 0
    for it in range(240):
        seg = int(rng.choice([128, 192, 256, 512]))
        n = int(rng.integers(1, 14))
        s = bytearray(mixed(n, int(rng.integers(1 << 30)), hi=int(rng.choice([80, 300, 700]))))
        roll = rng.random()
        if roll < 0.15:
            at = int(rng.integers(0, len(s)))
            s[at] = int(rng.integers(0, 256))
        elif roll < 0.3:
            s = s[:int(rng.integers(0, len(s) + 1))]
        s = bytes(s)
        kw = {}
        if rng.random() < 0.3:
            kw["max_unmapped"] = int(rng.integers(1, 4))
        if rng.random() < 0.3:
            kw["max_bytes"] = int(rng.integers(1, 600))
        mr, final = int(rng.integers(1, 8)), bool(rng.random() < 0.6)
        plain = ecl.window_cut(s, seg, mr, final, order_seed=it + 1, **kw)
        got = emu(s, seg, mr, final, NO_END, order_seed=it + 1, **kw)
        same(got, plain, it)
        same(got, host_loop(s, mr, final, **kw), it)
        own = int(rng2.integers(0, len(s) + 2))
        if it % 2 == 0:
            same(emu(s, seg, mr, final, own, order_seed=it + 1, **kw), host_loop(s, mr, final, own_bytes=own, **kw), (it, own))
        n_err += plain.status != OK
    assert n_err > 10


# ---- CPU: the sanitizer build ----------------------------------------------------------------------------------------------------------------------

def test_nothing_outside_the_stretch_is_read(tmp_path):
    """the emulator cases above again in a stand-alone ASan + UBSan program, every stream in a heap block of its exact size"""
    cases, want = [], []

    def start(s, n_ref, final, tile=64, oseed=3, tseed=0):
        cases.append(("start", s, n_ref, final, tile, oseed, tseed))
        want.append(part_start_ref(s, n_ref, final))

    def cut(s, seg, mr, final, own, mu=0, mb=0):
        cases.append(("cut", s, seg, mr, final, own, mu, mb))
        want.append(host_loop(s, mr, final, mu, mb, own_bytes=own))

    tail = mixed(9, 40, hi=100, k0=3)
    first = rec(61)
    for c in range(1, len(first), 7):
        start(first[c:] + tail, 2, True)
    for n in range(0, 8):
        for final in (True, False):
            start(rec(80)[33:] + mixed(n, 20 + n, hi=90, k0=1), 2, final, 128, 5, n)
    full = rec(80)[33:] + mixed(3, 31, hi=90, k0=1)
    for drop in (1, 3, 4, 20, 36, 40):
        for final in (True, False):
            start(full[:-drop], 2, final)
    for n in (0, 1, 35, 36, 37, 39):
        start(rec(39)[:n], 2, True)
        start(rec(39)[:n], 2, False)
    for bs in (0x7FFFFF00, 0xFFFFFFFF, 0xFFFFFFFC, 36 + 60):  # block_size far beyond, wrapping, and a little beyond the bytes
        bogus = bytearray(rec(40))
        bogus[0:4] = struct.pack("<I", bs)
        start(bytes(bogus) + tail, 2, False)
        start(tail + bytes(bogus), 2, True)
        start(tail + bytes(bogus), 2, False)
    big, _ = in_quals(b"".join(rec(40, "p", k, tid=2) for k in range(8)), 600)
    start(big[10:] + tail, 2, True)
    start(big[10:] + tail, 3, True)
    # a name length and a CIGAR count that point beyond a short block_size, at the very end of the block
    for lq, ncg in ((255, 0), (1, 0xFFFF), (3, 1)):
        r = bytearray(rec(39))
        r[12], r[16:18] = lq, struct.pack("<H", ncg)
        start(tail + bytes(r), 2, True)
    rng = np.random.default_rng(99)
    for it in range(30):
        s = bytearray(mixed(int(rng.integers(1, 10)), int(rng.integers(1 << 30)), hi=160))
        s = s[int(rng.integers(0, 100)):]
        for _ in range(int(rng.integers(0, 3))):
            if len(s):
                s[int(rng.integers(0, len(s)))] = int(rng.integers(0, 256))
        s = bytes(s[:int(rng.integers(0, len(s) + 1))]) if rng.random() < 0.4 else bytes(s)
        start(s, 2, bool(it & 1), 64, it + 1, it + 1)
    good = b"".join(rec(70 + k, "pu"[k % 2], k) for k in range(5))
    gs = rec_starts(good)
    huge = bytearray(rec(90))
    huge[0:4] = struct.pack("<I", 0xFFFFFFFF)
    for tail_, final in ((bytes(huge), True), (bytes(huge), False), (rec(91)[:90], True), (rec(64)[:3], False), (_bad("bs0"), True), (b"", True)):
        for own in (0, gs[2] + 1, len(good), NO_END):
            cut(good + tail_, 128, 100, final, own)
        cut(good + tail_, 128, 2, final, gs[2], 1, 150)
    rc, err, got = epl.run_asan(cases, str(tmp_path))
    assert rc == 0, err
    assert len(got) == len(want) > 120
    for c, g, w in zip(cases, got, want):
        if c[0] == "start":
            assert g == w, c
        else:
            assert g.key() == w.key(), c


# ---- CPU: the reader's logic, zlib and the emulator standing in for the device -----------------------------------------------------------------------

class StandIn:
    """devreader.DeviceMemory without a device: host buffers, zlib for k_bgzf_inflate behind the real header walk, the emulator for the cut
    and the part start"""

    def __init__(self, seg=1024):
        import torch

        self.torch, self.dev, self.eng, self.seg, self.keep = torch, torch.device("cpu"), self, seg, None
        self.n_part_end = 0

    def on_stream(self):
        return contextlib.nullcontext()

    def pinned(self, n):
        return self.torch.empty(n, dtype=self.torch.uint8)

    empty = pinned

    def view(self, ptr, n, tdtype):
        nbytes = n * (8 if tdtype == self.torch.int64 else 1)
        raw = np.frombuffer(C.string_at(C.cast(ptr, C.c_void_p).value, nbytes), dtype=np.uint8).copy() if nbytes else np.zeros(0, np.uint8)
        return self.torch.from_numpy(raw.view(np.int64) if tdtype == self.torch.int64 else raw)

    def synchronize(self):
        pass

    def close(self):
        pass

    def bgzf_inflate_part_dev(self, bgzf, n, dst, cap, file_off, range_end):
        buf = C.string_at(bgzf, n)
        rc, used, nbytes, own, nblk = epl.bgzf_walk_part(buf, cap, file_off, range_end)
        if rc:
            raise api.PortelloError(IO, "not a BGZF block")
        for off, coff, clen, uoff, ulen, crc in ecl.bgzf_walk(buf, cap)[3]:
            d = zlib.decompress(buf[coff:coff + clen], -15) if ulen else b""
            assert len(d) == ulen and zlib.crc32(d) & 0xFFFFFFFF == crc and uoff + ulen <= cap
            C.memmove(dst + uoff, d, ulen)
        return abi.PloBgzfInflatePartOut(nblk, used, nbytes, 0.0, own)

    def window_cut_part_dev(self, stream, n, max_records, final, own, max_unmapped=0, max_bytes=0):
        c = epl.window_cut_part(C.string_at(stream, n), self.seg, max_records, final, own, max_unmapped, max_bytes, order_seed=5)
        if c.status != OK:
            raise api.PortelloError(c.status, "refused")
        self.n_part_end += c.ended_by == abi.CUT_PART_END
        off, unm = np.array(c.read_rec_off + [0], dtype=np.uint64), np.frombuffer(c.unmapped + b"\0", dtype=np.uint8).copy()
        self.keep = (off, unm)
        return abi.PloWindowCutOut(c.n_reads, off.ctypes.data_as(abi._u64p), c.n_unmapped, None, unm.ctypes.data_as(abi._u8p), len(c.unmapped), c.window_bytes,
                                   c.ended_by, abi.CUT_NO_ERR, 0.0, 0)

    def part_start_dev(self, stream, n, n_ref, final):
        kind, off = epl.part_start(C.string_at(stream, n), n_ref, final, 256, 3, 0)
        return abi.PloPartStartOut(kind, abi.CUT_NO_ERR if off is None else off, 0.0)


def reader_part(path, part, n_parts, max_records, mem=None, index=None, **kw):
    """the windows of devreader.DeviceBamReader(part, n_parts) as host_part gives the host's"""
    rd = devreader.DeviceBamReader(path, index, part=part, n_parts=n_parts, memory=mem, **kw)
    out = []
    while True:
        w = rd.read_window(max_records)
        if w is None:
            break
        ub, nu = w.unmapped_bytes()
        out.append((Cut(OK, w.n_reads, [int(x) for x in w.read_rec_off.cpu().numpy()], nu, ub, None, w.records_bytes, abi.CUT_EOF if w.eof else -1),
                    w.records[:w.records_bytes].cpu().numpy().tobytes()))
        eof = w.eof
        w.close()
        if eof:
            break
    assert rd.read_window(max_records) is None
    stats = (rd.n_refills, rd.n_recuts, rd.n_start_calls, rd.part_start_ms, rd.ref_names, rd.ref_lens)
    rd.close()
    return out, stats


def taken(wins):
    """the primary and the unmapped records of the windows, in order"""
    out = []
    for c, raw in wins:
        out += [raw[o:o + 4 + struct.unpack_from("<I", raw, o)[0]] for o in c.read_rec_off]
        at = 0
        while at < len(c.unmapped):
            out.append(c.unmapped[at:at + 4 + struct.unpack_from("<I", c.unmapped, at)[0]])
            at += len(out[-1])
    return out


def taken_of(stream):
    w = host_loop(stream, 1 << 30, True)
    return taken([(Cut(OK, w.n_reads, w.read_rec_off, w.n_unmapped, w.unmapped, None, w.window_bytes, w.ended_by), stream)])


def windows_equal(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for (g, graw), (w, wraw) in zip(got, want):
        assert (g.n_reads, g.read_rec_off, g.n_unmapped, g.unmapped, g.window_bytes, g.ended_by) == \
            (w.n_reads, w.read_rec_off, w.n_unmapped, w.unmapped, w.window_bytes, w.ended_by), what
        assert graw == wraw, what


def test_parts_are_disjoint_and_complete(files):
    """for n_parts in 1, 2, 3, 7 and 4 x #blocks every part's windows are the host part's, and their union is the whole file with no record
    twice"""
    n_found = 0
    for tb in files:
        for n_parts in part_counts(tb):
            union = []
            for part in range(n_parts):
                mem = StandIn()
                got, stats = reader_part(tb.path, part, n_parts, 9, mem)
                windows_equal(got, host_part(tb.path, part, n_parts, 9), (tb.path, n_parts, part))
                ref_ = tb.part_ref(part, n_parts)
                assert mem.n_part_end <= 1 and (mem.n_part_end == 1 or ref_ is None or ref_[1] == len(tb.stream)) and (part + 1 < n_parts or not mem.n_part_end)
                union += taken(got)
                n_found += stats[2] > 0
            assert sorted(union) == sorted(taken_of(tb.stream)) and len(set(union)) == len(union), (tb.path, n_parts)
    assert n_found > 30
    # the whole file without a part: the reader as it was
    tb = files[0]
    got, _ = reader_part(tb.path, None, 1, 9, StandIn())
    rd = bam.BamReader(tb.path, 2)
    assert (rd.ref_names, rd.ref_lens) == (NAMES, [500000, 500000])
    rd.close()
    windows_equal(got, host_part(tb.path, 0, 1, 9), "whole")


def test_reader_refills(tmp_path):
    """a file of several chunks: the file offset of every refill and the own_bytes position move with the stream"""
    tb = TinyBam(str(tmp_path / "big.bam"), mixed(3200, 77, hi=200), 78, p_empty=0.05, lo=20, hi=120)
    assert len(tb.data) > 4 * (1 << 16)
    union = []
    for part in range(2):
        mem = StandIn(seg=8192)
        got, stats = reader_part(tb.path, part, 2, 400, mem, start_bytes=40, chunk_bytes=1 << 16, stream_bytes=1 << 17)
        windows_equal(got, host_part(tb.path, part, 2, 400), part)
        assert stats[0] >= 3 and stats[2] == part and (mem.n_part_end > 0) == (part < 1)
        union += taken(got)
    assert sorted(union) == sorted(taken_of(tb.stream)) and len(set(union)) == len(union)


def test_device_input_takes_parts():
    from portello_amd import pipeline

    with pytest.raises(ValueError, match="one reader"):
        pipeline.run_bam_to_bam("in.bam", "out.bam", None, None, [], [], [], device_input=True, device_records=True, device_batch=True, n_readers=2, part=0, n_parts=2)
    # part / n_parts are no longer refused: the call gets as far as opening the input
    with pytest.raises(Exception) as e:
        pipeline.run_bam_to_bam("/nonexistent/in.bam", "out.bam", None, api.Index.__new__(api.Index), [], [], [], device_input=True, device_records=True,
                                device_batch=True, part=0, n_parts=2)
    assert not isinstance(e.value, ValueError) or "part" not in str(e.value)
    assert pipeline.PipelineStats().part_start_device_ms == 0.0


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------------

def reblock(src, dst, rng, lo=3000, hi=30000):
    """the BAM file `src` again with BGZF payloads of lo .. hi bytes and a few ISIZE-0 blocks in the middle -> (data, blocks)"""
    data = open(src, "rb").read()
    rc, used, nb, blks = ecl.bgzf_walk(data, 1 << 40)
    assert rc == 0 and used == len(data)
    plain = b"".join(zlib.decompress(data[c:c + l], -15) for _, c, l, _, u, _ in blks if u)
    out, blocks, at = b"", [], 0
    while at < len(plain):
        if rng.random() < 0.05:
            blocks.append((len(out), 28, at, 0))
            out += bgzf_block(b"")
        n = min(int(rng.integers(lo, hi)), len(plain) - at)
        b = bgzf_block(plain[at:at + n])
        blocks.append((len(out), len(b), at, n))
        out += b
        at += n
    blocks.append((len(out), 28, at, 0))
    out += bgzf_block(b"")
    with open(dst, "wb") as fh:
        fh.write(out)
    return out, blocks, plain


@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    """300 reads with supplementary records and an unmapped tail of 80, in BGZF blocks of 3-30 KB: every one of eight parts has records"""
    d = tmp_path_factory.mktemp("partgpu")
    w = synth.generate(synth.config("tiny", n_reads=300, seed=78, split_read_frac=0.3, sorted_reads=True))
    src, path = str(d / "src.bam"), str(d / "reads.bam")
    meta = bamsynth.write_read_bam(w, src, level=6, n_unmapped=80)
    data, blocks, plain = reblock(src, path, np.random.default_rng(4))
    return w, path, meta, data, blocks, plain


def host_first_and_own(path, plain, part, n_parts):
    """(offset in the inflated file of the host part's first record, of the end of its records), None for an empty part"""
    wins = host_part(path, part, n_parts, 1 << 20, keep_empty=True)
    if not wins:
        return None
    raw = b"".join(r for _, r in wins)
    a = plain.find(raw)
    assert a > 0 and plain.find(raw, a + 1) < 0
    return a, a + len(raw)


@pytest.mark.gpu
@pytest.mark.parametrize("n_parts", [2, 3, 8])
def test_part_start_and_own_bytes_through_the_abi(sample, n_parts):
    import torch

    w, path, meta, data, blocks, plain = sample
    index = api.Index(w.index_data(), 0)
    eng = api.Engine(index)
    dev = torch.device("cuda", 0)
    n_ref = len(devreader.parse_header(plain)[1])
    size, n_nonempty, hdr_bytes = len(data), 0, devreader.parse_header(plain)[3]
    starts = [hdr_bytes + x for x in rec_starts(plain[hdr_bytes:])]
    for part in range(n_parts):
        lo, hi = size * part // n_parts, size * (part + 1) // n_parts
        want = host_first_and_own(path, plain, part, n_parts)
        k = next(j for j, b in enumerate(blocks) if b[0] >= lo)
        assert want is not None and blocks[k][0] < hi
        n_nonempty += 1
        host = np.frombuffer(data[blocks[k][0]:], dtype=np.uint8).copy()
        cap = len(plain) - blocks[k][2]
        dst = torch.full((cap + 64,), 0xEE, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        range_end = NO_END if part + 1 == n_parts else hi
        io = eng.bgzf_inflate_part_dev(host.ctypes.data, len(host), dst.data_ptr(), cap, blocks[k][0], range_end)
        assert (int(io.bgzf_consumed), int(io.n_bytes)) == (len(host), cap) and io.inflate_ms > 0
        got = dst.cpu().numpy()
        assert got[:cap].tobytes() == plain[blocks[k][2]:] and (got[cap:] == 0xEE).all()
        # own_bytes: the host part's records end at the first record that starts at or behind it
        own = blocks[k][2] + int(io.own_bytes)
        assert own == next((b[2] for b in blocks if b[0] >= range_end), len(plain))
        assert want[1] == next((x for x in starts if x >= own), len(plain)) and (part + 1 < n_parts or own == len(plain))
        if part == 0:
            continue
        for nbytes, final in ((cap, True), (min(cap, 1 << 20), cap <= (1 << 20))):
            so = eng.part_start_dev(dst.data_ptr(), nbytes, n_ref, final)
            assert so.start_ms > 0 and (int(so.kind), blocks[k][2] + int(so.first_off)) == (FOUND, want[0]), (part, nbytes)
        # too few bytes for the chain: need more, or (nothing in them that could start a record) none -- as the host loop says
        short = min(cap, 5000)
        so = eng.part_start_dev(dst.data_ptr(), short, n_ref, False)
        ref_kind, ref_off = part_start_ref(plain[blocks[k][2]:blocks[k][2] + short], n_ref, False)
        assert (int(so.kind), int(so.first_off) if int(so.kind) == FOUND else None) == (ref_kind, ref_off)
    assert n_nonempty == n_parts
    assert int(eng.part_start_dev(0, 0, n_ref, True).kind) == NONE
    eng.close()
    index.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_parts", [1, 3, 8])
def test_device_reader_parts_equal_the_host_readers(sample, n_parts):
    """window for window: read_rec_off, the record bytes, the unmapped records and eof; a small chunk and a small stream buffer so that parts
    span several windows and refills"""
    w, path, meta, data, blocks, plain = sample
    index = api.Index(w.index_data(), 0)
    union, n_refills, start_ms = [], 0, 0.0
    for part in range(n_parts):
        got, stats = reader_part(path, part, n_parts, 17, index=index, chunk_bytes=1 << 16, stream_bytes=1 << 17, start_bytes=1 << 15)
        want = host_part(path, part, n_parts, 17)
        windows_equal(got, want, (n_parts, part))
        assert len(got) >= 2 and got[-1][0].ended_by == abi.CUT_EOF
        union += taken(got)
        n_refills += stats[0]
        start_ms += stats[3]
        assert (stats[2] > 0) == (part > 0)
    hdr = devreader.parse_header(plain)
    assert union == taken_of(plain[hdr[3]:]) and n_refills > 2 * n_parts and (start_ms > 0) == (n_parts > 1)
    index.close()


@pytest.mark.gpu
def test_bam_to_bam_with_device_input_in_parts(tmp_path):
    """run_bam_to_bam(device_input=True, part=i, n_parts=3), the parts in turn: the union of the outputs checked as
    test_bam_to_bam_with_device_input checks one file -- every read, every record, the unmapped pass-through exactly once"""
    from oracle import expect
    from portello_amd import pipeline

    w = synth.generate(synth.config("chr20", n_reads=3_000), device="cuda")
    src, inp, unp = str(tmp_path / "src.bam"), str(tmp_path / "reads.bam"), str(tmp_path / "unassembled.bam")
    meta = bamsynth.write_read_bam(w, src, level=1, n_threads=8, n_unmapped=50)
    reblock(src, inp, np.random.default_rng(6), 20000, 65000)
    ixd = w.index_data()
    index = api.Index(w.index_data_device())
    cn, rn = meta["contig_names"], bamsynth.ref_names(w)
    kw = dict(window_reads=700, n_workers=2, io_threads=8, device_records=True, device_batch=True)
    outs, uns, stats = [], [], []
    for part in range(3):
        outp, un = str(tmp_path / f"lifted{part}.bam"), str(tmp_path / f"un{part}.bam")
        st = pipeline.run_bam_to_bam(inp, outp, index, ixd, cn, rn, [int(s.numel()) for s in w.chrom_seq], unassembled_path=un, device_input=True,
                                     part=part, n_parts=3, **kw)
        assert not st.errors and st.reads > 0 and st.inflate_device_ms > 0 and st.cut_device_ms > 0 and (st.part_start_device_ms > 0) == (part > 0)
        outs += st.out_paths
        uns.append(un)
        stats.append(st)
    assert sum(s.reads for s in stats) == w.n_reads and sum(s.unmapped_passed_through for s in stats) == 50
    # the unassembled files of the parts side by side: one BAM for the check
    rd = bam.BamReader(uns[0], 2)
    wr = bam.BamWriter(unp, rd.header_text, rd.ref_names, rd.ref_lens, level=1)
    rd.close()
    for un in uns:
        for _, raw in host_part(un, 0, 1, 1 << 20):
            wr.write(raw)
    wr.close()
    v = expect.verify_lifted_bam(inp, outs, ixd, cn, rn, window=1000, every=1, threads=8, unassembled_bam=unp)
    assert v["ok"] and v["reads_verified"] == w.n_reads and v["records_verified"] == sum(s.records_out for s in stats) == v["records_in_output"], v
    assert v["unassembled_ok"]
    index.close()
