"""plo_bgzf_inflate_dev / plo_window_cut_dev (API 10): the inflated BAM stream kept on the device and cut there into the windows
plo_bam_read_window cuts.  CPU: window_core.hpp under the wave emulator (tests/emu/emu_cut.cpp) with shuffled lane order and segments of
128-512 bytes, against plo_bam_read_window on a BAM written from the same records and -- where the limits are small -- against host_loop
below, a restatement of the host loop that is itself checked against plo_bam_read_window at the host's own limits.  GPU: the two calls,
the cut feeding plo_batch_build_dev, and run_bam_to_bam(device_input=True) against the host pipeline."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

import emu_cut_lib as ecl
from emu_cut_lib import Cut
from portello_amd import abi, api, bam, bamsynth, synth

NAMES = ["ctgA", "ctgB"]
OK, IO, DATA = abi.PLO_OK, abi.PLO_ERR_IO, abi.PLO_ERR_DATA
SEGS = (128, 256, 512)


# ---- records and streams --------------------------------------------------------------------------------------------------------------------

def rec(total, cls="p", k=0, qual=None, l_seq=None):
    """a record of exactly `total` bytes (block_size word included, total >= 39): cls p(rimary) / u(nmapped) / s(upplementary)"""
    name = b"r%d" % (k % 10) + b"\0"
    body = total - 4 - 32 - len(name)
    if l_seq is None:
        l_seq = (2 * body) // 3  # bases + qualities fill the record, the rest is an aux field's worth of padding
        while (l_seq + 1) // 2 + l_seq > body:
            l_seq -= 1
    pad = body - (l_seq + 1) // 2 - l_seq
    assert pad >= 0
    flag, tid = {"p": (0, 0), "u": (4, -1), "s": (0x800, 1)}[cls]
    q = bytes([k % 40] * l_seq) if qual is None else qual
    b = struct.pack("<iiBBHHHIiii", tid, 100 + k, len(name), 30, 4680, 0, flag, l_seq, -1, -1, 0) + name + bytes([0x12] * ((l_seq + 1) // 2)) + q + b"\x00" * pad
    assert len(b) == total - 4
    return struct.pack("<I", len(b)) + b


def host_loop(stream, max_records, final, max_unmapped=0, max_bytes=0):
    """plo_bam_read_window's loop (bam_host.cpp:257-297) over bytes in memory"""
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
        bs = struct.unpack_from("<I", stream, at)[0] if n - at >= 4 else None
        if bs is not None and bs < 32:
            return Cut(IO, err_off=at)
        if bs is None or n - at < 4 + bs:
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


def host_windows(tmp_path, stream, max_records, name="w.bam"):
    """the windows of bam.BamReader over a BAM written from `stream`: Cut per window (ended_by: EOF or not)"""
    path = str(tmp_path / name)
    wr = bam.BamWriter(path, "@HD\tVN:1.6\n", NAMES, [500000] * len(NAMES), level=1)
    wr.write(stream)
    wr.close()
    rd = bam.BamReader(path, 2)
    out = []
    while True:
        h = C.c_void_p()
        st = bam.lib().plo_bam_read_window(rd.handle, max_records, C.byref(h))
        if st != OK:
            out.append(Cut(st))
            break
        w = bam.Window(h)
        raw = w.raw()
        ub, nu = w.unmapped_bytes()
        nr = int(raw.n_reads)
        out.append(Cut(OK, nr, [int(raw.read_rec_off[i]) for i in range(nr)], nu, ub, None, int(raw.raw_bytes), abi.CUT_EOF if w.eof else -1))
        eof = w.eof
        w.close()
        if eof:
            break
    rd.close()
    return out


def cut_all(stream, seg, max_records, cutter, **kw):
    """the whole stream window after window: every next window starts at the last one's window_bytes"""
    at, out = 0, []
    while True:
        c = cutter(stream[at:], seg, max_records, True, **kw)
        out.append((at, c))
        if c.status != OK or c.ended_by == abi.CUT_EOF:
            return out
        assert c.window_bytes > 0 or c.ended_by != abi.CUT_EOF
        if c.window_bytes == 0 and not (c.n_reads or c.n_unmapped):
            assert c.ended_by in (abi.CUT_MAX_UNMAPPED,), c  # (a window that takes nothing would loop)
            return out
        at += c.window_bytes


def emu(stream, seg, max_records, final, **kw):
    return ecl.window_cut(stream, seg, max_records, final, order_seed=kw.pop("order_seed", 7), **kw)


def ref(stream, seg, max_records, final, **kw):
    kw.pop("order_seed", None)
    return host_loop(stream, max_records, final, **kw)


def same(got: Cut, want: Cut, what=""):
    assert got.key() == want.key(), (what, got, want)
    if got.status == OK:
        assert got.unmapped_off[-1] == len(got.unmapped) and len(got.unmapped_off) == got.n_unmapped + 1
        for i in range(got.n_unmapped):
            assert struct.unpack_from("<I", got.unmapped, got.unmapped_off[i])[0] + 4 == got.unmapped_off[i + 1] - got.unmapped_off[i]


def mixed(n, seed, lo=39, hi=300, classes="pppppus"):
    rng = np.random.default_rng(seed)
    return b"".join(rec(int(rng.integers(lo, hi)), classes[int(rng.integers(0, len(classes)))], k) for k in range(n))


# ---- CPU: the emulator against the host reader and the host loop -----------------------------------------------------------------------------

def test_host_loop_restates_the_host_reader(tmp_path):
    """the restatement the small-limit tests lean on, against plo_bam_read_window at the host's own limits"""
    stream = mixed(120, 1)
    for mr in (7, 50, 1000):
        hw = host_windows(tmp_path, stream, mr)
        at = 0
        for k, w in enumerate(hw):
            last = k + 1 == len(hw)
            want = host_loop(stream[at:], mr, True)
            assert (w.n_reads, w.read_rec_off, w.n_unmapped, w.unmapped, w.window_bytes) == (want.n_reads, want.read_rec_off, want.n_unmapped, want.unmapped, want.window_bytes)
            assert (want.ended_by == abi.CUT_EOF) == (w.ended_by == abi.CUT_EOF) == last
            at += w.window_bytes
        assert at == len(stream)


@pytest.mark.parametrize("seg", SEGS)
def test_windows_equal_the_host_readers(tmp_path, seg):
    """supplementary records skipped, unmapped records between primaries packed in order, window after window"""
    stream = mixed(90, 2)
    hw = host_windows(tmp_path, stream, 11)
    got = cut_all(stream, seg, 11, emu)
    assert len(got) == len(hw)
    for (at, g), w in zip(got, hw):
        assert (g.status, g.n_reads, g.read_rec_off, g.n_unmapped, g.unmapped, g.window_bytes) == (OK, w.n_reads, w.read_rec_off, w.n_unmapped, w.unmapped, w.window_bytes)
        same(g, host_loop(stream[at:], 11, True))
    assert got[-1][1].ended_by == abi.CUT_EOF and sum(g.n_unmapped for _, g in got) > 3


def test_segment_geometry():
    seg = 128
    cases = {
        "a record starts at a segment's first byte": rec(128) + rec(60, "u", 1) + rec(90, k=2),
        "a block_size word straddles a boundary": rec(126) + rec(70, k=1) + rec(60, "u", 2) + rec(254 - 130 + 2, k=3) + rec(50, k=4),
        "a record spans three segments": rec(50) + rec(400, k=1) + rec(45, "u", 2) + rec(300, "s", 3) + rec(39, k=4),
        "shorter than a segment": rec(40) + rec(41, "u", 1),
        "one record": rec(77),
        "empty": b"",
    }
    for what, s in cases.items():
        for final in (True, False):
            for sg in (seg, 256):
                same(emu(s, sg, 100, final), host_loop(s, 100, final), what)
                same(emu(s, sg, 100, final, no_guess=True), host_loop(s, 100, final), what + " (no guesses)")
    e = emu(b"", 128, 5, True)
    assert (e.status, e.n_reads, e.n_unmapped, e.window_bytes, e.ended_by) == (OK, 0, 0, 0, abi.CUT_EOF)
    assert emu(b"", 128, 5, False).ended_by == abi.CUT_END_OF_BYTES
    for at in (126, 127):  # every place of the word across the boundary
        s = rec(at) + rec(64, k=1)
        same(emu(s, 128, 9, True), host_loop(s, 9, True))


def with_decoys(recs, seg):
    """lays eight well-formed fake records into the quality bytes of every record at every segment boundary that lies inside them with room
    -> (stream, boundaries with a decoy)"""
    fake = b"".join(rec(40, "p", k) for k in range(8))
    stream, laid = bytearray(b"".join(recs)), []
    at = 0
    for r in recs:
        bs, = struct.unpack_from("<I", r, 0)
        lq, lseq = r[12], struct.unpack_from("<I", r, 20)[0]
        q0 = at + 36 + lq + (lseq + 1) // 2
        b = -(-q0 // seg) * seg
        while b + len(fake) <= q0 + lseq:
            stream[b:b + len(fake)] = fake
            laid.append(b)
            b += -(-len(fake) // seg) * seg
        at += 4 + bs
    return bytes(stream), laid


def live_decoys(stream, laid, seg):
    starts = set()
    at = 0
    while at < len(stream):
        starts.add(at)
        at += 4 + struct.unpack_from("<I", stream, at)[0]
    live = {s // seg for s in starts}
    return [b for b in laid if b // seg in live and b not in starts]


def test_decoy_in_the_quality_bytes_is_repaired():
    """a guess that is wrong: the chain rule passes at the segment's first byte, inside a record (eight fake records are 312 bytes at
    least, so only a segment of 512 bytes can hold them AND the start of the next real record, i.e. be live).  The resolve pass walks the
    segment again (the harness counts it), and the result is the serial walk's"""
    seg = 512
    recs = [rec(60), rec(2 * seg + 400 - 60, k=1), rec(90, "u", 2), rec(70, k=3)]  # the long record ends 400 bytes into segment 2
    stream, laid = with_decoys(recs, seg)
    assert laid == [2 * seg]
    want = host_loop(stream, 100, True)
    assert want.n_reads == 3 and want.n_unmapped == 1
    base = emu(b"".join(recs), seg, 100, True)
    got = emu(stream, seg, 100, True)
    same(got, want)
    assert live_decoys(stream, laid, seg) == laid and got.n_rewalks == base.n_rewalks + 1
    # every live segment behind the first starts with a decoy: records of two segments' length, each ending 400 bytes into a segment
    recs = [rec(400)] + [rec(2 * seg, "pu"[k % 5 == 4], k) for k in range(1, 13)] + [rec(50, k=3)]
    stream, laid = with_decoys(recs, seg)
    hit = live_decoys(stream, laid, seg)
    assert len(laid) == 12 and hit == laid
    got = emu(stream, seg, 5, True)
    same(got, host_loop(stream, 5, True))
    assert got.n_rewalks >= len(hit)
    for (at, g) in cut_all(stream, seg, 5, emu):
        same(g, host_loop(stream[at:], 5, True))


def test_stop_rules():
    seg = 128
    s = b"".join(rec(60 + k, "pppu"[k % 4], k) for k in range(24))  # p p p u ...
    # max_records inside a segment / at the last record of the stretch / each with the next window's first record
    for mr in (1, 4, 18):
        wins = cut_all(s, seg, mr, emu)
        want = cut_all(s, seg, mr, ref)
        assert [a for a, _ in wins] == [a for a, _ in want] and len(wins) > 1
        for (_, g), (_, w) in zip(wins, want):
            same(g, w)
        assert wins[0][1].ended_by == abi.CUT_MAX_RECORDS
    only_p = b"".join(rec(50 + k, "p", k) for k in range(6))
    e = emu(only_p, seg, 6, True)
    same(e, host_loop(only_p, 6, True))
    assert e.ended_by == abi.CUT_MAX_RECORDS and e.window_bytes == len(only_p)  # (not EOF: the count test comes first)
    nxt = emu(only_p[e.window_bytes:], seg, 6, True)
    assert (nxt.n_reads, nxt.ended_by) == (0, abi.CUT_EOF)
    # max_unmapped
    for mu in (1, 2, 5):
        wins, want = cut_all(s, seg, 100, emu, max_unmapped=mu), cut_all(s, seg, 100, ref, max_unmapped=mu)
        assert [a for a, _ in wins] == [a for a, _ in want] and len(wins) > 1
        for (_, g), (_, w) in zip(wins, want):
            same(g, w)
        assert wins[0][1].ended_by == abi.CUT_MAX_UNMAPPED and wins[0][1].n_unmapped == mu
    # max_bytes: a first record is taken whatever its size ("at least one record"), supplementary records do not count as taken
    for mb in (1, 61, 200, 500):
        wins, want = cut_all(s, seg, 100, emu, max_bytes=mb), cut_all(s, seg, 100, ref, max_bytes=mb)
        assert [a for a, _ in wins] == [a for a, _ in want]
        for (_, g), (_, w) in zip(wins, want):
            same(g, w)
        assert wins[0][1].ended_by == abi.CUT_MAX_BYTES and wins[0][1].n_reads >= 1
    assert cut_all(s, seg, 100, emu, max_bytes=1)[0][1].n_reads == 1
    sup = rec(70, "s") + rec(80, "s", 1) + rec(60, "p", 2) + rec(60, "p", 3)
    e = emu(sup, seg, 100, True, max_bytes=10)
    same(e, host_loop(sup, 100, True, max_bytes=10))
    assert e.n_reads == 1 and e.window_bytes == 210


def _bad(kind):
    r = bytearray(rec(100, "p", 5))
    if kind == "bs0":
        r[0:4] = struct.pack("<I", 0)
    elif kind == "bs31":
        r[0:4] = struct.pack("<I", 31)
    elif kind == "layout":
        r[20:24] = struct.pack("<I", 90)  # l_seq: bases + qualities beyond block_size
    elif kind == "unm_tid":
        r[18:20] = struct.pack("<H", 4)   # flag 0x4, tid stays 0
    return bytes(r)


@pytest.mark.parametrize("kind,status", [("bs0", IO), ("bs31", IO), ("layout", IO), ("unm_tid", DATA), ("trunc", IO)])
def test_refusals(kind, status):
    seg = 128
    good = [rec(60 + 3 * k, "ppu"[k % 3], k) for k in range(9)]
    for where in (0, 4, 9):  # first, in the middle (another segment), last
        bad = rec(100, "p", 5)[:57] if kind == "trunc" else _bad(kind)
        tail = [] if kind == "trunc" else good[where:]
        s = b"".join(good[:where]) + bad + b"".join(tail)
        off = sum(len(g) for g in good[:where])
        got = emu(s, seg, 100, True)
        assert (got.status, got.err_off) == (status, off), (kind, where, got)
        same(got, host_loop(s, 100, True))
        same(emu(s, seg, 100, True, no_guess=True), host_loop(s, 100, True))
        if kind == "trunc":  # the same bytes when more may follow: the window ends in front of the record
            nf = emu(s, seg, 100, False)
            same(nf, host_loop(s, 100, False))
            assert (nf.status, nf.ended_by, nf.window_bytes) == (OK, abi.CUT_END_OF_BYTES, off)
            for cutoff in (1, 2, 3, 4, 5, 35):  # fewer than 4 bytes, and fewer than 4 + block_size
                s2 = b"".join(good[:where]) + rec(100)[:cutoff]
                assert emu(s2, seg, 100, True).key() == (IO, off)
                assert emu(s2, seg, 100, False).key() == host_loop(s2, 100, False).key()
        # behind the window's end the record fails nothing; it fails the window it belongs to
        if where:
            n_p = sum(1 for g in good[:where] if not g[18] & 4)
            w0 = emu(s, seg, n_p, True)
            same(w0, host_loop(s, n_p, True))
            assert w0.status == OK and w0.n_reads == n_p and w0.window_bytes <= off
            wins = cut_all(s, seg, n_p, emu)
            assert wins[-1][1].status == status and wins[-1][0] + wins[-1][1].err_off == off
    # the first of two offending records is the one reported
    s = good[0] + _bad("unm_tid") + good[1] + _bad("bs0")
    assert emu(s, seg, 100, True).key() == (DATA, len(good[0]))


def test_nothing_outside_the_stretch_is_read(tmp_path):
    """block_size 0xffffffff and one that ends a byte past the stretch, in a heap block of the exact size under ASan + UBSan"""
    good = b"".join(rec(70 + k, "pu"[k % 2], k) for k in range(3))
    huge = bytearray(rec(90))
    huge[0:4] = struct.pack("<I", 0xFFFFFFFF)
    past = rec(91)[:90]
    for tail, final in ((bytes(huge), True), (bytes(huge), False), (past, True), (past, False), (rec(64)[:3], False), (b"", True)):
        s = good + tail
        rc, err, got = ecl.run_asan(s, 128, 100, final, str(tmp_path))
        assert rc == 0, err
        same(got, host_loop(s, 100, final))
    stream, _ = with_decoys([rec(60), rec(2 * 512 + 340, k=1), rec(90, "u", 2)], 512)
    rc, err, got = ecl.run_asan(stream, 512, 100, True, str(tmp_path))
    assert rc == 0, err
    same(got, host_loop(stream, 100, True))


def test_fuzz_against_the_host_loop():
    rng = np.random.default_rng(20261017)
    n_err = n_multi = 0
    for it in range(240):
        seg = int(rng.choice([128, 192, 256, 512]))
        n = int(rng.integers(1, 14))
        s = bytearray(mixed(n, int(rng.integers(1 << 30)), hi=int(rng.choice([80, 300, 700]))))
        roll = rng.random()
        if roll < 0.15:  # damage: a byte of some record's fixed fields
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
        got, want = emu(s, seg, mr, final, order_seed=it + 1, **kw), host_loop(s, mr, final, **kw)
        same(got, want, (it, seg, mr, final, kw))
        n_err += want.status != OK
        n_multi += len(s) > 2 * seg
    assert n_err > 10 and n_multi > 60


def test_device_input_needs_device_batch():
    from portello_amd import pipeline

    with pytest.raises(ValueError, match="device_batch"):
        pipeline.run_bam_to_bam("in.bam", "out.bam", None, None, [], [], [], device_input=True)
    with pytest.raises(ValueError, match="device_batch"):
        pipeline.run_bam_to_bam("in.bam", "out.bam", None, None, [], [], [], device_input=True, device_records=True)
    with pytest.raises(ValueError, match="one reader"):
        pipeline.run_bam_to_bam("in.bam", "out.bam", None, None, [], [], [], device_input=True, device_records=True, device_batch=True, n_readers=2)
    assert pipeline.PipelineStats().inflate_device_ms == 0.0 == pipeline.PipelineStats().cut_device_ms


# ---- CPU: the header walk of plo_bgzf_inflate_dev (host code; zlib stands in for the inflate kernel) -----------------------------------------

def bgzf_block(payload: bytes) -> bytes:
    co = zlib.compressobj(6, zlib.DEFLATED, -15)
    d = co.compress(payload) + co.flush()
    return (b"\x1f\x8b\x08\x04" + bytes(6) + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, len(d) + 25) + d +
            struct.pack("<II", zlib.crc32(payload) & 0xFFFFFFFF, len(payload)))


EOF_BLOCK = bgzf_block(b"")


def inflate_walked(buf, blks):
    out = b""
    for off, coff, clen, uoff, ulen, crc in blks:
        d = zlib.decompress(buf[coff:coff + clen], -15) if ulen or clen else b""
        assert uoff == len(out) and len(d) == ulen and (zlib.crc32(d) & 0xFFFFFFFF) == crc
        out += d
    return out


def test_bgzf_header_walk():
    rng = np.random.default_rng(3)
    pay = [bytes(rng.integers(0, 20, int(n), dtype=np.uint8)) for n in (1000, 65280, 1, 300)]
    blocks = [bgzf_block(p) for p in pay]
    assert len(EOF_BLOCK) == 28
    buf = blocks[0] + blocks[1] + EOF_BLOCK + blocks[2] + blocks[3] + EOF_BLOCK  # an EOF block in the middle is consumed and adds nothing
    rc, used, nb, blks = ecl.bgzf_walk(buf, 1 << 30)
    assert (rc, used, nb, len(blks)) == (0, len(buf), sum(map(len, pay)), 6)
    assert inflate_walked(buf, blks) == b"".join(pay)
    assert [b[0] for b in blks][:3] == [0, len(blocks[0]), len(blocks[0]) + len(blocks[1])]
    # a partial trailing block is not consumed: cut anywhere inside the last data block
    whole = len(blocks[0]) + len(blocks[1]) + 28 + len(blocks[2])
    for cut in (1, 3, 4, 11, 17, 27, 28, len(blocks[3]) - 1):
        rc, used, nb, blks = ecl.bgzf_walk(buf[:whole + cut], 1 << 30)
        assert (rc, used, len(blks)) == (0, whole, 4), cut
    # blocks that no longer fit stop the walk at a block boundary
    rc, used, nb, blks = ecl.bgzf_walk(buf, 1000 + 65279)
    assert (rc, used, nb, len(blks)) == (0, len(blocks[0]), 1000, 1)
    rc, used, nb, blks = ecl.bgzf_walk(buf, 1000 + 65280)
    assert (rc, used, nb, len(blks)) == (0, len(blocks[0]) + len(blocks[1]) + 28, 66280, 3)  # (the EOF block behind them still fits)
    assert ecl.bgzf_walk(buf, 0)[1:3] == (0, 0) and ecl.bgzf_walk(b"", 100)[:3] == (0, 0, 0)
    # a damaged magic at a block boundary is refused, with the block's offset; so is what is left of one in a cut block
    for k, v in ((0, 0x1e), (1, 0x8c), (2, 7), (3, 0)):
        bad = bytearray(buf)
        bad[len(blocks[0]) + k] = v
        rc, used, _, _ = ecl.bgzf_walk(bytes(bad), 1 << 30)
        assert (rc, used) == (1, len(blocks[0])), k
    assert ecl.bgzf_walk(blocks[0] + b"\x1f\x8c", 1 << 30)[:2] == (1, len(blocks[0]))
    nobc = bytearray(blocks[0])
    nobc[12:14] = b"XY"
    assert ecl.bgzf_walk(bytes(nobc) + blocks[1], 1 << 30)[:2] == (2, 0)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def sample(tmp_path_factory):
    """1500 reads (46 MB of records) with supplementary records and an unmapped tail of 400"""
    d = tmp_path_factory.mktemp("cutdev")
    w = synth.generate(synth.config("tiny", n_reads=1500, seed=77, split_read_frac=0.3, sorted_reads=True))
    path = str(d / "reads.bam")
    meta = bamsynth.write_read_bam(w, path, level=6, n_unmapped=400)
    data = open(path, "rb").read()
    rc, used, nb, blks = ecl.bgzf_walk(data, 1 << 40)
    assert rc == 0 and used == len(data)
    return w, path, meta, data, inflate_walked(data, blks)


class Dev:
    def __init__(self, w):
        import torch

        self.torch = torch
        self.dev = torch.device("cuda", 0)
        self.index = api.Index(w.index_data(), 0)
        self.eng = api.Engine(self.index)

    def inflate(self, data: bytes, cap: int):
        host = np.frombuffer(data, dtype=np.uint8).copy()
        dst = self.torch.full((max(16, cap) + 64,), 0xEE, dtype=self.torch.uint8, device=self.dev)
        self.torch.cuda.synchronize()
        io = self.eng.bgzf_inflate_dev(host.ctypes.data, len(data), dst.data_ptr(), cap)
        return io, dst

    def cut(self, t, at, n, max_records, final, **kw) -> Cut:
        co = self.eng.window_cut_dev(t.data_ptr() + at, n, max_records, final, **kw)
        nr, nu, ub = int(co.n_reads), int(co.n_unmapped), int(co.unmapped_bytes)
        assert co.cut_ms > 0
        return Cut(OK, nr, [int(x) for x in self.eng.download(co.read_rec_off, np.uint64, nr)], nu, self.eng.download(co.unmapped, np.uint8, ub).tobytes(),
                   [int(x) for x in self.eng.download(co.unmapped_off, np.uint64, nu + 1)], int(co.window_bytes), int(co.ended_by), int(co.err_off), int(co.n_rewalks))

    def close(self):
        self.eng.close()
        self.index.close()


@pytest.mark.gpu
def test_inflate_dev(sample):
    w, path, meta, data, plain = sample
    d = Dev(w)
    io, dst = d.inflate(data, len(plain))
    assert (int(io.bgzf_consumed), int(io.n_bytes)) == (len(data), len(plain)) and io.inflate_ms > 0 and int(io.n_blocks) >= 2
    got = dst.cpu().numpy()
    assert got[:len(plain)].tobytes() == plain and (got[len(plain):] == 0xEE).all()
    # a small dst_cap stops at a block boundary; a partial trailing block is not consumed
    _, _, _, blks = ecl.bgzf_walk(data, 1 << 40)
    cap = blks[1][3] + blks[1][4] + 5 if len(blks) > 2 else blks[0][4]
    rc, used, nb, _ = ecl.bgzf_walk(data, cap)
    io, dst = d.inflate(data, cap)
    assert (int(io.bgzf_consumed), int(io.n_bytes)) == (used, nb) and 0 < nb <= cap
    got = dst.cpu().numpy()
    assert got[:nb].tobytes() == plain[:nb] and (got[nb:] == 0xEE).all()
    io, _ = d.inflate(data[:len(data) - 40], len(plain))
    assert int(io.bgzf_consumed) == ecl.bgzf_walk(data[:len(data) - 40], 1 << 40)[1] < len(data) - 40
    assert int(d.inflate(b"", 100)[0].n_blocks) == 0
    # a damaged CRC and a damaged magic are PLO_ERR_IO; the text names the block's offset (a deflate stream that does not decode:
    # test_inflate_crafted.py::test_dev_refused_stream, one per status of inflate.hpp)
    bad = bytearray(data)
    bad[blks[1][0] + (blks[1][1] - blks[1][0]) + blks[1][2]] ^= 0x55  # first CRC byte of block 1
    with pytest.raises(api.PortelloError) as e:
        d.inflate(bytes(bad), len(plain))
    assert e.value.status == IO and f"offset {blks[1][0]}" in str(e.value) and "CRC" in str(e.value)
    bad = bytearray(data)
    bad[blks[1][0]] = 0
    with pytest.raises(api.PortelloError) as e:
        d.inflate(bytes(bad), len(plain))
    assert e.value.status == IO and f"offset {blks[1][0]}" in str(e.value)
    d.close()


@pytest.mark.gpu
def test_cut_dev_equals_the_host_reader(sample):
    """at the ABI's own segment size with the host's limits, then with small limits and a stream that arrives in pieces (re-cut after a
    refill); also with small segments, where the sample has thousands of them"""
    w, path, meta, data, plain = sample
    d = Dev(w)
    from portello_amd import devreader
    hdr = devreader.parse_header(plain)
    rd = bam.BamReader(path, 2)
    assert (hdr[1], hdr[2]) == (rd.ref_names, rd.ref_lens)
    rd.close()
    rec_bytes = plain[hdr[3]:]
    t = d.torch.from_numpy(np.frombuffer(rec_bytes, dtype=np.uint8).copy()).to(d.dev)
    d.torch.cuda.synchronize()
    for mr, kw in ((100_000, {}), (700, {}), (500, {"max_unmapped": 60}), (100_000, {"max_bytes": 12_000_000}), (700, {"seg_bytes": 256})):
        at = n_win = 0
        while True:
            got = d.cut(t, at, len(rec_bytes) - at, mr, True, **kw)
            hk = {k: v for k, v in kw.items() if k != "seg_bytes"}
            same(got, host_loop(rec_bytes[at:], mr, True, **hk), (mr, kw, at))
            at += got.window_bytes
            n_win += 1
            if got.ended_by == abi.CUT_EOF:
                break
        assert at == len(rec_bytes) and (n_win > 1 or mr == 100_000 and not kw)
    # the host reader itself, window by window
    rd = bam.BamReader(path, 2)
    at = 0
    while True:
        win = rd.read_window(700)
        if win is None:
            break
        raw = win.raw()
        got = d.cut(t, at, len(rec_bytes) - at, 700, True)
        assert got.read_rec_off == [int(raw.read_rec_off[i]) for i in range(int(raw.n_reads))] and got.window_bytes == int(raw.raw_bytes)
        assert (got.unmapped, got.n_unmapped) == win.unmapped_bytes() and (got.ended_by == abi.CUT_EOF) == win.eof
        at += got.window_bytes
        win.close()
    rd.close()
    assert at == len(rec_bytes)
    # a stretch that ends inside a record: END_OF_BYTES in front of it, and the same start cut again with more bytes gives the full window
    part = len(rec_bytes) // 3
    g1 = d.cut(t, 0, part, 100_000, False)
    same(g1, host_loop(rec_bytes[:part], 100_000, False))
    assert g1.ended_by == abi.CUT_END_OF_BYTES and g1.window_bytes <= part
    same(d.cut(t, 0, len(rec_bytes), 100_000, True), host_loop(rec_bytes, 100_000, True))
    # one refused record through the ABI
    bad = bytearray(rec_bytes)
    off = host_loop(rec_bytes, 900, True).read_rec_off[-1]
    bad[off + 18] |= 4  # flag 0x4 on a record that has a tid
    tb = d.torch.from_numpy(np.frombuffer(bytes(bad), dtype=np.uint8).copy()).to(d.dev)
    d.torch.cuda.synchronize()
    with pytest.raises(api.PortelloError) as e:
        d.eng.window_cut_dev(tb.data_ptr(), len(bad), 100_000, True)
    assert (e.value.status, e.value.err_off) == (DATA, off) and str(off) in str(e.value)
    same(d.cut(tb, 0, len(bad), 899, True), host_loop(bytes(bad), 899, True))  # behind the window's end it fails nothing
    d.close()


@pytest.mark.gpu
def test_cut_feeds_batch_build_lift_and_records(sample):
    """read_rec_off of the cut straight into plo_batch_build_dev, lift and plo_records_build_dev: the records of the host route"""
    import torch

    from portello_amd import devbatch, devreader
    w, path, meta, data, plain = sample
    cn, rn = meta["contig_names"], bamsynth.ref_names(w)
    index = api.Index(w.index_data(), 0)
    dev = torch.device("cuda", 0)

    def records(eng, ur):
        labels = devbatch.contig_labels(cn, dev)
        sa_in, _keep = devbatch.sa_inputs(rn, dev)
        up = devbatch.DeviceBuiltWindow(ur, eng.batch_build_dev(ur.build_in(labels)))
        out = eng.liftover_batch_dev(up.desc())
        eng.compact_output_dev(out)
        eng.finish_batch_dev(up.desc(), up.finish_in())
        eng.sa_segments_dev(sa_in)
        ro = eng.records_build_dev(up.desc(), up.records_in(labels, False))
        return devbatch.DeviceRecords(ro, dev=dev).data()

    rdr = devreader.DeviceBamReader(path, index, chunk_bytes=1 << 20, stream_bytes=1 << 22)
    hrd = bam.BamReader(path, 2)
    eng = api.Engine(index)
    n = 0
    while True:
        dw, hw = rdr.read_window(600), hrd.read_window(600)
        assert (dw is None) == (hw is None)
        if dw is None:
            break
        assert dw.n_records == hw.n_records and dw.unmapped_bytes() == hw.unmapped_bytes() and dw.eof == hw.eof
        if dw.n_records:
            got = records(eng, devbatch.UploadedRecords(dw.records, dw.records_bytes, dw.read_rec_off, dw.n_reads))
            ur = devbatch.upload_records(hw.raw(), dev)
            torch.cuda.synchronize()
            assert got == records(eng, ur) and len(got) > 1000
        n += 1
        hw.close()
        dw.close()
    assert n >= 3 and rdr.n_refills > 3 and rdr.n_recuts >= 1 and rdr.inflate_ms > 0 and rdr.cut_ms > 0
    assert (rdr.ref_names, rdr.ref_lens) == (hrd.ref_names, hrd.ref_lens)
    for h in (rdr, hrd, eng, index):
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("device_bgzf", [False, True])
def test_bam_to_bam_with_device_input(tmp_path, device_bgzf):
    """run_bam_to_bam(device_input=True) as test_bam_to_bam_with_device_batch is set up: every read, every record, the unmapped pass-through"""
    from oracle import expect
    from portello_amd import pipeline

    w = synth.generate(synth.config("chr20", n_reads=6_000), device="cuda")
    inp, outp, unp = str(tmp_path / "reads.bam"), str(tmp_path / "lifted.bam"), str(tmp_path / "unassembled.bam")
    meta = bamsynth.write_read_bam(w, inp, level=1, n_threads=8, n_unmapped=50)
    ixd = w.index_data()
    index = api.Index(w.index_data_device())
    cn, rn = meta["contig_names"], bamsynth.ref_names(w)
    args = (inp, outp, index, ixd, cn, rn, [int(s.numel()) for s in w.chrom_seq])
    with pytest.raises(ValueError, match="device_batch"):
        pipeline.run_bam_to_bam(*args, device_input=True, device_records=True)
    kw = dict(window_reads=1500, n_workers=2, io_threads=8, device_records=True, device_batch=True, device_bgzf=device_bgzf, out_shards=2)
    st = pipeline.run_bam_to_bam(*args, unassembled_path=unp, device_input=True, **kw)
    assert st.reads == w.n_reads and len(st.out_paths) == 2 and all(os.path.exists(p_) and os.path.getsize(p_) > 1000 for p_ in st.out_paths)
    v = expect.verify_lifted_bam(inp, st.out_paths, ixd, cn, rn, window=1000, every=1, threads=8, unassembled_bam=unp)
    assert v["ok"] and v["reads_verified"] == w.n_reads and v["records_verified"] == st.records_out == v["records_in_output"], v
    assert v["unassembled_ok"] and st.unmapped_passed_through == 50
    assert st.inflate_device_ms > 0 and st.cut_device_ms > 0 and st.batch_device_ms > 0
    # the host pipeline's counts on the same input
    hp = str(tmp_path / "host.bam")
    hs = pipeline.run_bam_to_bam(inp, hp, *args[2:], unassembled_path=str(tmp_path / "host_un.bam"), **kw)
    assert (hs.reads, hs.records_out, hs.lifted, hs.unmapped_copies, hs.unmapped_passed_through, hs.bytes_out) == \
        (st.reads, st.records_out, st.lifted, st.unmapped_copies, st.unmapped_passed_through, st.bytes_out)
    assert hs.inflate_device_ms == 0 and hs.cut_device_ms == 0
    index.close()
