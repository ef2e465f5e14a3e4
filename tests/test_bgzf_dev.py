"""Output BGZF blocks compressed on the device (plo_bgzf_compress_dev, portello_amd/csrc/deflate.hpp; plo_bam_write_blocks).

The yardsticks are zlib (every block must inflate to its payload, as raw deflate data and as a gzip member; sizes are held against
zlib level 1), the format (RFC 1951 / 1952, the BGZF header) and the host writer (level 0 byte for byte).  The CPU tests run
deflate.hpp under the wave emulator (tests/emu/emu_deflate.cpp); the GPU tests run the C ABI on the device and the pipeline mode."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest

import emu_deflate_lib as edl
import emu_lib
from portello_amd import abi, api, bam

BLOCK = 0xff00
EOF_BLOCK = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0])
HDR = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0])


# ---- payloads ------------------------------------------------------------------------------------------------------------------------
def _payloads():  # the shapes of tests/test_inflate.py's _payloads()
    rng = np.random.default_rng(3)
    yield b""
    yield b"a"
    yield b"ACGT" * 5000
    yield rng.integers(0, 256, 40000, dtype=np.uint8).tobytes()  # incompressible
    yield bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), 65280))
    yield (b"the quick brown fox " * 700)[:13001]
    q = rng.integers(0, 94, 30000, dtype=np.uint8).tobytes()
    yield (q + q[::-1] + b"\0" * 3000 + q[:999])[:BLOCK]


def _big_payloads():  # ... and of its _big_payloads(): far and near repeats, stored stretches, two bits of entropy per byte
    rng = np.random.default_rng(17)
    text = (b"@read/%d/ccs\tACGTTGCA\tRG:Z:x\tnp:i:12\n" * 40)
    rnd = rng.integers(0, 256, 21000, dtype=np.uint8).tobytes()
    qual = bytes(rng.choice(np.arange(33, 74, dtype=np.uint8), 15000))
    a = text + qual + rnd[:9000] + text + b"A" * 700 + qual[:4000] + rnd[:3000] + qual[5000:9000] + text
    yield a[:65280]
    yield (rnd + rnd[100:8000] + b"xyz" * 50 + rnd[20000:] + rnd[:500])[:BLOCK]
    yield (bytes(rng.integers(0, 4, 65280, dtype=np.uint8) + 65))
    yield rng.integers(0, 256, 65280, dtype=np.uint8).tobytes()


def make_record(i, l_seq, qual, rng, ref_id=0, pos=None, flag=0):
    """one BAM record (block_size word first) with random bases, a PacBio-like name and the tags a HiFi read carries"""
    name = b"m84011_220902_175841_s1/%d/ccs\0" % (1000 + 37 * i)
    cig = struct.pack("<I", (l_seq << 4) | 7) if l_seq else b""
    codes = np.array([1, 2, 4, 8], np.uint8)[rng.integers(0, 4, l_seq + (l_seq & 1))]
    seq = ((codes[0::2] << 4) | codes[1::2]).astype(np.uint8)
    if l_seq & 1 and len(seq):
        seq[-1] &= 0xF0
    aux = b"RGZdefault\0" + b"npi" + struct.pack("<i", int(rng.integers(3, 40))) + b"rqf" + struct.pack("<f", 0.999) + b"ecf" + struct.pack("<f", float(rng.random() * 30))
    p = int(rng.integers(0, 1 << 20)) if pos is None else pos
    body = struct.pack("<iiBBHHHIiii", ref_id, p, len(name), 60, 4681, 1 if l_seq else 0, flag, l_seq, -1, -1, 0) + name + cig + seq.tobytes() + bytes(qual) + aux
    return struct.pack("<I", len(body)) + body


def bam_like_stream(n_bytes, seed=11):
    """records like bamsynth's: random bases, qualities uniform in 0 .. 93"""
    rng = np.random.default_rng(seed)
    out, size, i = [], 0, 0
    while size < n_bytes:
        l_seq = int(rng.integers(9000, 16000))
        out.append(make_record(i, l_seq, rng.integers(0, 94, l_seq, dtype=np.uint8), rng))
        size += len(out[-1])
        i += 1
    return out


def hifi_like_stream(n_bytes, seed=12):
    """records whose qualities are mostly one value (93) with short dips, as HiFi consensus qualities are"""
    rng = np.random.default_rng(seed)
    out, size, i = [], 0, 0
    while size < n_bytes:
        l_seq = int(rng.integers(9000, 16000))
        q = np.full(l_seq, 93, np.uint8)
        for at in rng.integers(0, l_seq, l_seq // 150):
            w = int(rng.integers(1, 12))
            q[at:at + w] = rng.integers(5, 60, len(q[at:at + w]), dtype=np.uint8)
        out.append(make_record(i, l_seq, q, rng))
        size += len(out[-1])
        i += 1
    return out


def zlib1(p):
    c = zlib.compressobj(1, zlib.DEFLATED, -15)
    return c.compress(p) + c.flush()


def _project_inflate(data, n, wave):
    L = emu_lib.lib()
    L.emu_inflate.restype = C.c_int
    L.emu_inflate.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_uint8), C.c_uint32, C.POINTER(C.c_uint32)]
    L.emu_inflate_wave.restype = C.c_int
    L.emu_inflate_wave.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_uint8), C.c_uint32, C.POINTER(C.c_uint32), C.c_uint]
    out = (C.c_uint8 * (n + 16))()
    w = C.c_uint32(0)
    rc = L.emu_inflate_wave(data, len(data), out, n, C.byref(w), 4711) if wave else L.emu_inflate(data, len(data), out, n, C.byref(w))
    return rc, bytes(out[:w.value])


def check_block(blk, payload, project=True):
    """the four conditions of a block: raw deflate data, gzip member, BSIZE / CRC-32 / ISIZE, the project's own decoder"""
    assert blk[:16] == HDR and len(blk) <= 18 + 5 + len(payload) + 8
    assert struct.unpack_from("<H", blk, 16)[0] + 1 == len(blk)
    data = blk[18:-8]
    assert zlib.decompress(data, -15) == payload
    assert zlib.decompress(blk, 31) == payload
    assert struct.unpack_from("<II", blk, len(blk) - 8) == (zlib.crc32(payload) & 0xffffffff, len(payload))
    assert data[0] & 1, "the deflate block is not final"
    if project:
        for wave in (False, True):
            rc, out = _project_inflate(data, len(payload), wave)
            assert rc == 0 and out == payload, (rc, wave, len(payload))


def emu_block(payload, level, seed=0):
    rc, blk = edl.deflate_block(payload, level, seed)  # (checks the guard bytes behind the slot and behind the block)
    assert rc == 0, rc
    return blk


# ---- CPU: deflate.hpp under the wave emulator -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", [0, 1])
def test_round_trip_of_the_inflate_tests_payloads(level):
    for p in list(_payloads()) + list(_big_payloads()):
        check_block(emu_block(p, level), p)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 257, 258, 259, 65279, 65280])
def test_round_trip_of_the_edge_lengths(n):
    rng = np.random.default_rng(n)
    text = bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), n))
    for p in (text, b"\x21" * n, (b"GATTACA" * 9400)[:n]):
        for level in (0, 1):
            check_block(emu_block(p, level), p)


@pytest.mark.parametrize("maker", [bam_like_stream, hifi_like_stream])
def test_round_trip_of_record_streams(maker):
    data = b"".join(maker(3 * BLOCK + 1234))
    blocks = edl.compress(data, 1)
    assert len(blocks) == (len(data) + BLOCK - 1) // BLOCK
    for k, blk in enumerate(blocks):
        check_block(blk, data[k * BLOCK:(k + 1) * BLOCK])
    assert sum(len(b) for b in blocks) < len(data)


def test_lane_order_does_not_change_a_byte():
    cases = [b"".join(bam_like_stream(BLOCK))[:BLOCK], b"".join(hifi_like_stream(BLOCK))[:BLOCK], next(_big_payloads()), b"\0" * 5000 + b"ab" * 3000, b"ACGT" * 16320]
    for p in cases:
        ref = emu_block(p, 1, 0)
        for seed in (1, 7, 4711, 99991):
            assert emu_block(p, 1, seed) == ref, (len(p), seed)
        assert emu_block(p, 0, 7) == emu_block(p, 0, 0)


def test_a_slot_that_is_too_small_or_a_long_payload_is_refused_without_a_write():
    p = b"ACGT" * 1000  # (compresses to a few dozen bytes: the bound is the stored form all the same, known before the encoder starts)
    for level in (0, 1):
        rc, blk = edl.deflate_block(p, level, cap=18 + 5 + len(p) + 8 - 1)  # (deflate_block asserts that nothing was written)
        assert rc == -1 and blk == b""
        assert edl.deflate_block(p, level, cap=18 + 5 + len(p) + 8)[0] == 0
        rc, blk = edl.deflate_block(b"x" * (BLOCK + 1), level, cap=BLOCK + 100)
        assert rc == -2 and blk == b""


def test_sanitizer_build(tmp_path):
    """the harness as a program with AddressSanitizer and UBSan: payloads, slots and token buffer in heap blocks of their exact size"""
    data = b"".join(hifi_like_stream(BLOCK + 3000)) + bytes(np.random.default_rng(1).integers(0, 256, 3000, dtype=np.uint8)) + b"\x07" * 9000
    for level in (0, 1):
        rc, err, out = edl.run_asan(data, level, str(tmp_path))
        assert rc == 0, (rc, err[-2000:])
        assert out == b"".join(edl.compress(data, level))
        got = b"".join(zlib.decompress(b, 31) for b in _split_blocks(out))
        assert got == data


def _split_blocks(run):
    at, out = 0, []
    while at < len(run):
        n = struct.unpack_from("<H", run, at + 16)[0] + 1
        out.append(run[at:at + n])
        at += n
    assert at == len(run)
    return out


# ---- conditions that follow from the format ---------------------------------------------------------------------------------------------
def test_random_bytes_take_exactly_the_stored_form():
    for n in (1, 300, 40000, 65280):
        p = np.random.default_rng(n).integers(0, 256, n, dtype=np.uint8).tobytes()
        for level in (0, 1):
            blk = emu_block(p, level)
            assert len(blk) == 18 + 5 + n + 8 and blk[18] == 1 and blk[23:23 + n] == p


def test_matches_are_used():
    """a Huffman-only coder cannot go below one bit per byte: less than len / 8 bytes means LZ77 matches (distance 4; distance 1)"""
    for p in (b"ACGT" * 16320, b"\x2a" * 65280):
        z = len(zlib1(p))
        assert z < len(p) // 8 // 4, z  # zlib level 1 stays far inside the bound
        data = emu_block(p, 1)[18:-8]
        print(f"len {len(p)}: device {len(data)} bytes, zlib level 1 {z} bytes, bound {len(p) // 8}")
        assert len(data) < len(p) // 8


def test_level_0_equals_the_host_writer(tmp_path):
    """BamWriter(level=0) + one write of the payload == header blocks + the device's blocks through write_blocks (+ the EOF block)"""
    data = b"".join(bam_like_stream(2 * BLOCK + 777))
    a, b = str(tmp_path / "host.bam"), str(tmp_path / "dev.bam")
    for seekable_copy in ("", "1"):  # the gather-write path of a regular file, and the path that builds the blocks in a buffer
        os.environ["PLO_BGZF_COPY_BLOCKS"] = seekable_copy
        if not seekable_copy:
            del os.environ["PLO_BGZF_COPY_BLOCKS"]
        try:
            w = bam.BamWriter(a, "@HD\tVN:1.6\n", ["c1"], [1 << 24], level=0, n_threads=3)
            w.write(data)
            w.close()
        finally:
            os.environ.pop("PLO_BGZF_COPY_BLOCKS", None)
        w = bam.BamWriter(b, "@HD\tVN:1.6\n", ["c1"], [1 << 24], level=0, n_threads=3)
        hdr_bytes = w.file_bytes()
        blocks = b"".join(edl.compress(data, 0))
        w.write_blocks(blocks)
        assert w.file_bytes() == hdr_bytes + len(blocks)
        w.close()
        fa, fb = open(a, "rb").read(), open(b, "rb").read()
        assert fa == fb and fb[hdr_bytes:] == blocks + EOF_BLOCK


# ---- size against zlib level 1 ---------------------------------------------------------------------------------------------------------
# Measured with this test (device bytes / zlib level 1 bytes, deflate data only, summed over six 65 280-byte payloads of each stream):
#   BAM-like  312 581 / 312 876 = 0.9991 (0.798 of the payload either way: random bases and uniform qualities leave only their Huffman codes)
#   HiFi-like  96 486 / 101 094 = 0.9544 (distance-1 matches of up to 258 bytes over the runs of one quality value)
# m = the measured excess plus two percentage points; neither stream shows an excess, so m = 0 + 0.02 for both.
RATIO_MARGIN = {"bam_like": 0.02, "hifi_like": 0.02}


@pytest.mark.parametrize("name,maker", [("bam_like", bam_like_stream), ("hifi_like", hifi_like_stream)])
def test_size_against_zlib_level_1(name, maker):
    data = b"".join(maker(6 * BLOCK))
    dev = zl = 0
    for k in range(6):
        p = data[k * BLOCK:(k + 1) * BLOCK]
        assert len(p) == BLOCK
        dev += len(emu_block(p, 1)) - 26
        zl += len(zlib1(p))
    print(f"{name}: device {dev} bytes, zlib level 1 {zl} bytes, ratio {dev / zl:.4f}, of the payload {dev / (6 * BLOCK):.4f} / {zl / (6 * BLOCK):.4f}")
    assert dev <= zl * (1 + RATIO_MARGIN[name]), (dev, zl, dev / zl)


# ---- plo_bam_write_blocks ---------------------------------------------------------------------------------------------------------------
def _read_all(path, device_inflate=False):
    rd = bam.BamReader(path, 2, device_inflate=device_inflate)
    recs = []
    while True:
        win = rd.read_window(1000)
        if win is None:
            break
        recs += [win.record_bytes(i) for i in range(win.n_records)]
        win.close()
    rd.close()
    return recs


def test_write_blocks_interleaved_with_write(tmp_path):
    """records through plo_bam_write, then device blocks, then records again: the pending tail goes out as a short block of its own, the
    order of the records is kept, and the file reads back record for record"""
    recs = hifi_like_stream(5 * BLOCK, seed=5)
    k1, k2 = len(recs) // 3, 2 * len(recs) // 3
    a, b, c = b"".join(recs[:k1]), b"".join(recs[k1:k2]), b"".join(recs[k2:])
    assert len(a) % BLOCK and len(c) % BLOCK
    path = str(tmp_path / "mixed.bam")
    w = bam.BamWriter(path, "@HD\tVN:1.6\n", ["c1"], [1 << 24], level=1, n_threads=3)
    w.write(a)
    before = w.file_bytes()
    blocks = b"".join(edl.compress(b, 1))
    w.write_blocks(blocks)
    grown = w.file_bytes() - before - len(blocks)
    assert grown > 0, "the pending tail of the first write was not flushed in front of the blocks"
    w.write(c)
    w.write_blocks(b"")  # nothing: no flush either
    w.close()
    got = _read_all(path)
    assert len(got) == len(recs)
    for i, (g, e) in enumerate(zip(got, recs)):
        assert g == e, i
    # the tail went out as ONE block of its own, directly in front of the device's
    raw = open(path, "rb").read()
    at = raw.index(blocks)
    assert at == before + grown
    tail = _split_blocks(raw[before:at])
    assert len(tail) == 1 and zlib.decompress(tail[0], 31) == a[len(a) // BLOCK * BLOCK:]


@pytest.mark.parametrize("damage", ["truncated", "magic", "trailing", "subfield"])
def test_write_blocks_refuses_a_malformed_run(tmp_path, damage):
    recs = bam_like_stream(2 * BLOCK, seed=9)
    good = b"".join(edl.compress(b"".join(recs), 1))
    bad = {"truncated": good[:-5], "magic": good[:len(good) // 2].replace(b"\x1f\x8b", b"\x1f\x8c", 1) + good[len(good) // 2:],
           "trailing": good + b"\0" * 7, "subfield": good[:12] + b"XC" + good[14:]}[damage]
    assert bad != good
    path = str(tmp_path / "refused.bam")
    w = bam.BamWriter(path, "@HD\tVN:1.6\n", ["c1"], [1 << 24], level=1, n_threads=2)
    w.write(recs[0][:1000])  # an open partial block: must stay open
    size0, content0 = w.file_bytes(), open(path, "rb").read()
    with pytest.raises(api.PortelloError) as e:
        w.write_blocks(bad)
    assert e.value.status == abi.PLO_ERR_INVALID_ARG
    assert w.file_bytes() == size0 and open(path, "rb").read()[:len(content0)] == content0 and os.path.getsize(path) <= max(len(content0), size0)
    w.close()
    # the header, the 1000 pending bytes as one block, the EOF block: nothing of the refused run
    blocks = _split_blocks(open(path, "rb").read())
    assert blocks[-1] == EOF_BLOCK and zlib.decompress(blocks[-2], 31) == recs[0][:1000] and len(blocks) == 3


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def device_run(tmp_path_factory):
    """a records buffer of a few thousand reads on the device: the lift, finish, SA and records calls of tests/test_records_dev.py"""
    from portello_amd import bamsynth, synth
    import test_records_dev as trd

    d = tmp_path_factory.mktemp("bgzfdev")
    w = synth.generate(synth.config("tiny", n_reads=3000, seed=77, split_read_frac=0.3, sorted_reads=True))
    path = str(d / "reads.bam")
    meta = bamsynth.write_read_bam(w, path, level=1, n_unmapped=3)
    index = api.Index(w.index_data(), 0)
    rd, win = trd.open_window(path)
    run = trd.DeviceRun(win, index, meta["contig_names"], bamsynth.ref_names(w), False)
    run.finish()
    run.sa()
    yield run
    run.eng.close()
    win.close()
    rd.close()
    index.close()


@pytest.mark.gpu
@pytest.mark.parametrize("level", [0, 1])
def test_c_abi_blocks_inflate_to_the_records_and_equal_the_emulator(device_run, level):
    run = device_run
    ro = run.eng.records_build_dev(run.ddesc, run.up.records_in(run.labels, False))
    n = int(ro.n_bytes)
    assert n > 3 * BLOCK
    before = run.eng.download(ro.bytes, np.uint8, n).tobytes()
    bo = run.eng.bgzf_compress_dev(ro.bytes, n, level)
    assert int(bo.n_in) == n and int(bo.n_blocks) == (n + BLOCK - 1) // BLOCK and bo.bgzf_ms > 0
    off = run.eng.download(bo.block_off, np.uint64, int(bo.n_blocks) + 1)
    assert off[0] == 0 and int(off[-1]) == int(bo.n_bytes) and np.all(np.diff(off.astype(np.int64)) > 0)
    blocks = run.eng.download(bo.blocks, np.uint8, int(bo.n_bytes)).tobytes()
    # the records are where they were, unchanged: the compress call has buffers of its own
    assert run.eng.download(ro.bytes, np.uint8, n).tobytes() == before
    parts = _split_blocks(blocks)
    assert [len(p) for p in parts] == list(np.diff(off.astype(np.int64)))
    for k, blk in enumerate(parts):  # (the project's decoder takes these bytes in the CPU tests: they are the emulator's, see below)
        check_block(blk, before[k * BLOCK:(k + 1) * BLOCK], project=False)
    assert b"".join(zlib.decompress(b, 31) for b in parts) == before
    if level == 1:
        assert len(blocks) < n
    # byte for byte what the emulator writes for the same payloads.  Level 0: every block.  Level 1 (the emulator takes about half a
    # second per block): every block of a second call over 12 whole payloads and a short one from the middle of the buffer, and of the
    # whole buffer a spread of blocks with the short last one.
    if level == 0:
        pick = range(len(parts))
    else:
        mid = len(parts) // 2
        n_sub = min(12 * BLOCK + 4321, n - mid * BLOCK)
        bs = run.eng.bgzf_compress_dev(C.cast(ro.bytes, C.c_void_p).value + mid * BLOCK, n_sub, level)  # (ends the first call's outputs: `blocks` is a copy)
        sub = _split_blocks(run.eng.download(bs.blocks, np.uint8, int(bs.n_bytes)).tobytes())
        assert len(sub) == (n_sub + BLOCK - 1) // BLOCK and sub[:n_sub // BLOCK] == parts[mid:mid + n_sub // BLOCK]
        for k, blk in enumerate(sub):
            at = (mid + k) * BLOCK
            assert blk == emu_block(before[at:at + min(BLOCK, n_sub - k * BLOCK)], level, 3 * k + 1), k
        pick = sorted(set(list(range(0, len(parts), max(1, len(parts) // 6))) + [len(parts) - 1]))
    for k in pick:
        assert parts[k] == emu_block(before[k * BLOCK:(k + 1) * BLOCK], level, 7 * k), k
    # a second call gives the same bytes
    bo2 = run.eng.bgzf_compress_dev(ro.bytes, n, level)
    assert run.eng.download(bo2.blocks, np.uint8, int(bo2.n_bytes)).tobytes() == blocks


@pytest.mark.gpu
def test_c_abi_refusals_and_nothing(device_run):
    run = device_run
    ro = run.eng.records_build_dev(run.ddesc, run.up.records_in(run.labels, False))
    for level in (-1, 2, 9):
        with pytest.raises(api.PortelloError, match="level") as e:
            run.eng.bgzf_compress_dev(ro.bytes, int(ro.n_bytes), level)
        assert e.value.status == abi.PLO_ERR_INVALID_ARG
    with pytest.raises(api.PortelloError) as e:
        run.eng.bgzf_compress_dev(None, 100, 1)
    assert e.value.status == abi.PLO_ERR_INVALID_ARG
    for ptr in (ro.bytes, None):
        bo = run.eng.bgzf_compress_dev(ptr, 0, 1)
        assert int(bo.n_blocks) == 0 and int(bo.n_bytes) == 0 and int(bo.n_in) == 0
        assert int(run.eng.download(bo.block_off, np.uint64, 1)[0]) == 0
    # a payload that is not a whole number of blocks, from the middle of the buffer (odd address), still works
    bo = run.eng.bgzf_compress_dev(C.cast(ro.bytes, C.c_void_p).value + 3, BLOCK + 5, 1)
    got = run.eng.download(bo.blocks, np.uint8, int(bo.n_bytes)).tobytes()
    want = run.eng.download(ro.bytes, np.uint8, BLOCK + 8).tobytes()[3:]
    assert b"".join(zlib.decompress(b, 31) for b in _split_blocks(got)) == want and int(bo.n_blocks) == 2


def _pipeline_inputs(tmp_path):
    from portello_amd import bamsynth, synth

    w = synth.generate(synth.config("chr20", n_reads=20_000), device="cuda")
    inp = str(tmp_path / "reads.bam")
    meta = bamsynth.write_read_bam(w, inp, level=1, n_threads=8)
    ixd = w.index_data()
    index = api.Index(w.index_data_device())
    return w, inp, meta, ixd, index, meta["contig_names"], bamsynth.ref_names(w), [int(s.numel()) for s in w.chrom_seq]


@pytest.mark.gpu
def test_bam_to_bam_with_device_bgzf(tmp_path):
    """run_bam_to_bam(device_records=True, device_bgzf=True) at level 0 and level 1 into two shards: every record of every shard against
    the oracle; level 1 read back with host inflate and with device inflate; level 0 byte-identical with the host-framed file"""
    from oracle import expect
    from portello_amd import pipeline

    w, inp, meta, ixd, index, cn, rn, rl = _pipeline_inputs(tmp_path)
    with pytest.raises(ValueError):
        pipeline.run_bam_to_bam(inp, str(tmp_path / "x.bam"), index, ixd, cn, rn, rl, device_bgzf=True)
    sizes = {}
    for level in (0, 1):
        outp, unp = str(tmp_path / f"lifted{level}.bam"), str(tmp_path / f"unassembled{level}.bam")
        st = pipeline.run_bam_to_bam(inp, outp, index, ixd, cn, rn, rl, window_reads=1500, n_workers=2, io_threads=8, level=level, unassembled_path=unp,
                                     device_records=True, device_bgzf=True, out_shards=2)
        assert st.reads == w.n_reads and len(st.out_paths) == 2 and all(os.path.getsize(p_) > 1000 for p_ in st.out_paths)
        assert st.bgzf_device_ms > 0 and st.out_file_bytes == sum(os.path.getsize(p_) for p_ in st.out_paths)
        v = expect.verify_lifted_bam(inp, st.out_paths, ixd, cn, rn, window=1000, every=1, threads=8, unassembled_bam=unp)
        assert v["ok"] and v["reads_verified"] == w.n_reads and v["records_verified"] == st.records_out == v["records_in_output"], v
        assert v["unassembled_ok"]
        sizes[level] = (st.out_file_bytes, st.bytes_out)
        if level == 1:
            for p_ in st.out_paths:
                host, dev = _read_all(p_, False), _read_all(p_, 0)
                assert len(host) > 0 and host == dev
    print(f"output files: level 0 {sizes[0][0]} bytes, level 1 {sizes[1][0]} bytes, records {sizes[0][1]} bytes")
    assert sizes[0][1] == sizes[1][1] and sizes[1][0] < sizes[0][1] < sizes[0][0]
    # Level 0, byte for byte: the host writer carries a window's tail into the next window's first block and the device ends a block with
    # every window, so the files are identical where the block boundaries are -- a shard that received one window.  One window, one worker:
    # the window goes to whichever of the two writers is free, the other shard holds the header only.
    files = {}
    for mode in (False, True):
        outp = str(tmp_path / f"one_window_{int(mode)}.bam")
        st = pipeline.run_bam_to_bam(inp, outp, index, ixd, cn, rn, rl, window_reads=w.n_reads + 100, n_workers=1, io_threads=8, level=0, ramp=False,
                                     device_records=True, device_bgzf=mode, out_shards=2)
        assert st.windows == 1
        files[mode] = sorted((open(p_, "rb").read() for p_ in st.out_paths), key=len)
    assert len(files[True][1]) > 100 * BLOCK and files[True] == files[False]
    index.close()
