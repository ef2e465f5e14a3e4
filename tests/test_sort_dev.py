"""Coordinate-sorted output: plo_records_sort_dev (portello_amd/csrc/sort_core.hpp), plo_bam_merge_runs, plo_bam_output_header_so and
run_bam_to_bam(sorted_runs=True).

The yardstick is tests/sort_expect.py: the key read from the record's bytes, sorted(range(n), key=(key, index)), the concatenated bytes and
offsets -- plain Python from the definition, not derived from the code under test.  All comparisons are of integers and bytes.  The test
records are hand-made byte strings (fixed fields, a name, a little payload): the call looks at the fixed fields only.  The CPU tests run
sort_core.hpp under the wave emulator (tests/emu/emu_sort.cpp) with shuffled lane, wave, tile and chunk orders -- the output between canary
bytes, every byte of it watched to be stored exactly once -- and once more in a program built with AddressSanitizer + UBSan where every
array sits in a heap block of its exact size; the merge needs no GPU either.  The GPU tests run the C ABI on the device and the pipeline
mode."""
import os
import random
import struct

import numpy as np
import pytest

import bamcheck
import emu_sort_lib as esl
import sort_expect as sx
import test_records_dev as trd
from portello_amd import abi, api, bam, bamsynth

T = 1024  # SORT_TILE (test_sizes asserts it)
SIZES = [0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 4 * T + 3]
N_REFS = [1, 25, 3000, 65537]


def random_records(n, n_ref, seed, pos_span=40):
    """n short records: few distinct keys (so that ties are many), lengths over all residues mod 16"""
    rng = random.Random(seed)
    recs = []
    for i in range(n):
        ref = rng.choice([-1, 0, n_ref - 1, rng.randrange(n_ref)])
        recs.append(sx.make_record(ref, rng.randrange(-1, pos_span), rng.choice([0, 16, 4, 1 | 16]), b"q%d" % i, bytes(rng.randrange(256) for _ in range(rng.randrange(24)))))
    return recs


def big_record(ref, pos, size=200_003, seed=9):
    return sx.make_record(ref, pos, 0, b"big", np.random.default_rng(seed).integers(0, 256, size - 36 - 3, dtype=np.uint8).tobytes())


def key_shapes(n_ref=25):
    """name -> records"""
    rec = sx.make_record
    s = {}
    s["all keys equal"] = [rec(3 % n_ref, 77, 0, b"e%d" % i, bytes(i % 19)) for i in range(200)]
    s["already sorted"] = [rec(i // 40 % n_ref, i % 40 * 3, 0, b"s%d" % i) for i in range(200)]
    s["reverse sorted"] = list(reversed(s["already sorted"]))
    s["all unmapped"] = [rec(-1, -1, 4, b"u%d" % i, bytes(i % 7)) for i in range(130)]
    s["one unmapped record first"] = [rec(-1, -1, 4, b"u")] + [rec(0, 50 - i, 0, b"m%d" % i) for i in range(40)]
    s["reverse flag alone"] = [rec(1 % n_ref, 500, 16, b"rev"), rec(1 % n_ref, 500, 0, b"fwd"), rec(1 % n_ref, 499, 16, b"before")]
    s["pos -1 on a reference"] = [rec(0, 0, 0, b"zero"), rec(0, -1, 0, b"minus"), rec(-1, -1, 4, b"u"), rec(0, -1, 16, b"minus reverse")]
    s["the largest pos"] = [rec(0, sx.POS_MAX, 16, b"top reverse"), rec(-1, 5, 4, b"u"), rec(0, sx.POS_MAX, 0, b"top"), rec(0, sx.POS_MAX - 1, 16, b"below")]
    s["minimum length"] = [rec(i % 3 - 1, 9 - i % 10, 0) for i in range(70)]
    assert all(len(r) == 36 for r in s["minimum length"])
    # lengths 36 .. 36 + 47: every residue mod 16 for the source offsets, and -- the sorted order being another -- for the destination's
    s["every alignment residue"] = [rec(0, (i * 7) % 48, 0, b"", bytes([i]) * i) for i in range(48)] + [rec(0, (i * 5) % 48, 16, b"", bytes([i]) * (47 - i)) for i in range(48)]
    s["a 200 kB record between short ones"] = [rec(0, 10 + i, 0, b"a%d" % i, bytes(i)) for i in range(20)] + [big_record(0, 15)] + [rec(0, i, 16, b"b%d" % i, bytes(5)) for i in range(30)]
    return s


def check_result(res, e, what=""):
    assert np.array_equal(res["perm"], e["perm"]), what
    assert np.array_equal(res["key"], e["key"]), what
    assert np.array_equal(res["record_off"], e["record_off"]), what
    assert res["bytes"] == e["bytes"], what
    assert res["n_mapped"] == e["n_mapped"], what


def emu_check(recs, n_ref, seed, what=""):
    data, off = sx.concat(recs)
    assert sx.first_offender(data, off, n_ref) is None
    e = sx.expect(data, off, n_ref)
    st, res, er, ek = esl.sort(data, off, n_ref, e["bytes"], order_seed=seed)
    assert st == abi.PLO_OK, (what, seed, st)  # -2: a store outside the output, -3: a byte not stored exactly once
    assert er == 0xFFFFFFFF
    check_result(res, e, (what, seed))
    return e


# ---- CPU: sort_core.hpp under the wave emulator ---------------------------------------------------------------------------------------------

def test_expectation_by_hand():
    """the yardstick itself on an example small enough to sort by eye"""
    rec = sx.make_record
    recs = [rec(-1, -1, 4, b"u"), rec(1, 5, 0, b"b"), rec(0, 9, 16, b"c"), rec(1, 5, 0, b"d"), rec(0, 9, 0, b"e"), rec(0, -1, 0, b"f")]
    data, off = sx.concat(recs)
    e = sx.expect(data, off, 2)
    assert list(e["perm"]) == [5, 4, 2, 1, 3, 0] and e["n_mapped"] == 5
    assert list(e["key"]) == [0, 20, 21, (1 << 32) | 12, (1 << 32) | 12, 2 << 32]
    assert e["bytes"] == b"".join(recs[i] for i in (5, 4, 2, 1, 3, 0)) and int(e["record_off"][-1]) == len(data)


@pytest.mark.parametrize("n", SIZES)
def test_sizes(n):
    """1. every size around the wave and the tile, three lane / tile / chunk orders"""
    assert esl.tile() == T
    for seed in (0, 1, 2):
        emu_check(random_records(n, 25, 100 + n + seed), 25, seed, n)


@pytest.mark.parametrize("name", sorted(key_shapes()))
def test_key_shapes(name):
    """2. the key shapes and the lengths, alone and spread over more than two tiles"""
    recs = key_shapes()[name]
    for seed in (0, 1, 2):
        e = emu_check(recs, 25, seed, name)
    if name == "all keys equal":
        assert list(e["perm"]) == list(range(len(recs)))
    if name == "all unmapped":
        assert e["n_mapped"] == 0
    filler = random_records(2 * T + 1 - len(recs) // 2, 25, 5)
    k = len(filler) // 2
    emu_check(filler[:k] + recs + filler[k:], 25, 3, name + " in three tiles")


@pytest.mark.parametrize("n_ref", N_REFS)
def test_reference_counts(n_ref):
    """3. the width of the key's upper half; the highest reference and the unmapped tail next to each other"""
    recs = random_records(T + 65, n_ref, 7 + n_ref) + [sx.make_record(n_ref - 1, sx.POS_MAX, 16, b"last"), sx.make_record(-1, 0, 4, b"tail")]
    for seed in (0, 1):
        emu_check(recs, n_ref, seed, n_ref)


def refusals(n_ref=25):
    """name -> (data, off, n_ref): one offender each, inside a buffer of otherwise good records, in the second tile"""
    good = random_records(T + 40, n_ref, 77)
    at = T + 7

    def with_record(r):
        recs = list(good)
        recs[at] = r
        return sx.concat(recs)

    out = {}
    data, off = sx.concat(good)
    o = off.copy()
    o[at + 1] = o[at] - 1
    out["record_off decreases"] = (data, o, at, sx.ERR_OFFSET)
    o = off.copy()
    o[-1] -= 1
    out["record_off[n] != n_bytes"] = (data, o, len(good) - 1, sx.ERR_OFFSET)
    o = off.copy()
    o[0] = 1
    out["record_off[0] != 0"] = (data, o, 0, sx.ERR_OFFSET)
    d2, o2 = with_record(sx.make_record(0, 1)[:35])
    out["shorter than 36 bytes"] = (d2, o2, at, sx.ERR_SHORT)
    d2, o2 = with_record(sx.make_record(0, 1, 0, b"name", block_size=37))
    out["block_size disagrees"] = (d2, o2, at, sx.ERR_BLOCK)
    d2, o2 = with_record(sx.make_record(n_ref, 1))
    out["refID == n_ref"] = (d2, o2, at, sx.ERR_REFID)
    d2, o2 = with_record(sx.make_record(-2, 1))
    out["refID == -2"] = (d2, o2, at, sx.ERR_REFID)
    d2, o2 = with_record(sx.make_record(0, -2))
    out["pos == -2"] = (d2, o2, at, sx.ERR_POS)
    recs = list(good)
    recs[at], recs[90] = sx.make_record(0, -2), sx.make_record(-3, 0)
    d2, o2 = sx.concat(recs)
    out["two offenders"] = (d2, o2, 90, sx.ERR_REFID)
    return out


@pytest.mark.parametrize("name", sorted(refusals()))
def test_refusal(name):
    """4. every check refuses, names the LOWEST offending record, and nothing is copied"""
    data, off, rec, kind = refusals()[name]
    assert sx.first_offender(data, off, 25) == (rec, kind)
    for seed in (0, 1):
        st, res, er, ek = esl.sort(data, off, 25, b"", order_seed=seed)
        assert (st, res, er, ek) == (abi.PLO_ERR_INVALID_ARG, None, rec, kind), name


def test_asan_program(tmp_path):
    """5. the same harness as a stand-alone program with ASan + UBSan, every array in a heap block of its exact size: sizes, shapes,
    refusals"""
    cases, wants = [], []
    for n in SIZES:
        recs = random_records(n, 25, 300 + n)
        data, off = sx.concat(recs)
        e = sx.expect(data, off, 25)
        cases.append((data, off, 25, e["bytes"], n % 3))
        wants.append(e)
    for name, recs in sorted(key_shapes().items()):
        data, off = sx.concat(recs)
        e = sx.expect(data, off, 25)
        cases.append((data, off, 25, e["bytes"], 1))
        wants.append(e)
    for name, (data, off, rec, kind) in sorted(refusals().items()):
        cases.append((data, off, 25, None, 0))
        wants.append((rec, kind))
    rc, err, res = esl.run_asan(cases, str(tmp_path))
    assert rc == 0, err[-3000:]
    assert "ERROR" not in err and "runtime error" not in err, err[-3000:]
    for (st, r, er, ek), want, case in zip(res, wants, cases):
        if isinstance(want, tuple):
            assert (st, er, ek) == (abi.PLO_ERR_INVALID_ARG,) + want
        else:
            assert st == abi.PLO_OK
            if len(case[1]) > 1:
                check_result(r, want)


# ---- CPU: the host side ---------------------------------------------------------------------------------------------------------------------

REFS, LENS = ["chr1", "chr2", "chrM"], [5000, 4000, 160]


def write_run(path, recs, header=None, refs=REFS, lens=LENS):
    wr = bam.BamWriter(path, header if header is not None else bam.output_header(refs, lens, sort_order="coordinate"), refs, lens, level=0)
    if recs:
        wr.write(b"".join(recs))
    wr.close()
    return path


def sorted_run(n, seed):
    recs = random_records(n, len(REFS), seed)
    return [recs[i] for i in sorted(range(n), key=lambda i: (sx.key_of(recs[i], len(REFS)), i))]


def test_output_header_sort_order():
    a, b = bam.output_header(REFS, LENS, cmdline="x y"), bam.output_header(REFS, LENS, cmdline="x y", sort_order="coordinate")
    assert a.startswith("@HD\tVN:1.6\tSO:unsorted\n") and b == a.replace("SO:unsorted", "SO:coordinate", 1) and a.count("SO:") == 1
    assert bam.output_header(REFS, LENS, cmdline="x y", sort_order="unsorted") == a


def test_merge_runs(tmp_path):
    """three runs with equal keys across them and an unmapped tail each -> sorted(all, key=(key, run, index)); also deflated"""
    runs = [sorted_run(300, 1), sorted_run(5, 2), sorted_run(170, 3)]
    assert all(any(r[4:8] == b"\xff\xff\xff\xff" for r in run) for run in runs)
    keys = [set(sx.key_of(r, 3) for r in run) for run in runs]
    assert keys[0] & keys[1] and keys[0] & keys[2]
    paths = [write_run(str(tmp_path / f"run{k}.bam"), run) for k, run in enumerate(runs)]
    want = sx.merged(runs, 3)
    for level in (0, 1):
        out = str(tmp_path / f"merged{level}.bam")
        bam.merge_runs(paths, out, level=level)
        text, refs, recs = bamcheck.read_bam(out)
        assert text == bam.output_header(REFS, LENS, sort_order="coordinate") and refs == list(zip(REFS, LENS))
        assert recs == want
    # another order of the paths is another tie order
    out = str(tmp_path / "merged_other.bam")
    bam.merge_runs(paths[::-1], out)
    assert bamcheck.read_bam(out)[2] == sx.merged(runs[::-1], 3) != want


def test_merge_refuses_an_unsorted_run(tmp_path):
    run = sorted_run(50, 4)
    k = next(i for i in range(49) if sx.key_of(run[i], 3) != sx.key_of(run[i + 1], 3))
    run[k], run[k + 1] = run[k + 1], run[k]
    good, bad = write_run(str(tmp_path / "good.bam"), sorted_run(20, 5)), write_run(str(tmp_path / "swapped.bam"), run)
    out = str(tmp_path / "out.bam")
    with pytest.raises(api.PortelloError, match=r"swapped\.bam: record %d " % (k + 1)) as e:
        bam.merge_runs([good, bad], out)
    assert e.value.status == bam.ERR_DATA and not os.path.exists(out)  # a failed merge leaves no file that reads as a complete BAM


def test_merge_refuses_differing_headers(tmp_path):
    a = write_run(str(tmp_path / "a.bam"), sorted_run(10, 6))
    b = write_run(str(tmp_path / "b.bam"), sorted_run(10, 7), header=bam.output_header(REFS, LENS, cmdline="another", sort_order="coordinate"))
    c = write_run(str(tmp_path / "c.bam"), [], refs=REFS[:2], lens=LENS[:2], header=bam.output_header(REFS, LENS, sort_order="coordinate"))
    for other in (b, c):
        with pytest.raises(api.PortelloError, match="header differs") as e:
            bam.merge_runs([a, other], str(tmp_path / "out.bam"))
        assert e.value.status == abi.PLO_ERR_INVALID_ARG
    with pytest.raises(api.PortelloError) as e:
        bam.merge_runs([], str(tmp_path / "out.bam"))
    assert e.value.status == abi.PLO_ERR_INVALID_ARG


@pytest.mark.parametrize("cut", [40, 28, 5000])
def test_merge_refuses_a_truncated_run(tmp_path, cut):
    """cut inside the last data block, exactly in front of the EOF block, and in the middle of the file"""
    a = write_run(str(tmp_path / "a.bam"), sorted_run(400, 8))
    blob = open(a, "rb").read()
    assert len(blob) > 2 * cut
    short = str(tmp_path / "short.bam")
    open(short, "wb").write(blob[:-cut])
    with pytest.raises(api.PortelloError, match=r"short\.bam") as e:
        bam.merge_runs([a, short], str(tmp_path / "out.bam"))
    assert e.value.status == bam.ERR_IO


def test_merge_refuses_a_corrupt_block_behind_the_first_refill(tmp_path):
    """a run of 6 MB whose last data block has a flipped byte: the header and the first 4 MB refill are sound, so the failure comes from a
    later refill of the record walk -- PLO_ERR_IO, the message names the run, no output file stays"""
    big = [big_record(0, 100 + i, seed=i) for i in range(30)]
    a, b = write_run(str(tmp_path / "a.bam"), sorted_run(20, 9)), write_run(str(tmp_path / "big.bam"), big)
    out = str(tmp_path / "out.bam")
    bam.merge_runs([a, b], out)
    assert bamcheck.read_bam(out)[2] == sx.merged([sorted_run(20, 9), big], 3)
    blob = bytearray(open(b, "rb").read())
    assert len(blob) > 6_000_000
    blob[-28 - 8 - 1000] ^= 0x40  # a stored byte of the last data block: its CRC no longer holds
    bad = str(tmp_path / "corrupt.bam")
    open(bad, "wb").write(bytes(blob))
    os.remove(out)
    with pytest.raises(api.PortelloError, match=r"corrupt\.bam") as e:
        bam.merge_runs([a, bad], out)
    assert e.value.status == bam.ERR_IO and not os.path.exists(out)


def test_merge_of_a_header_only_run(tmp_path):
    a = write_run(str(tmp_path / "empty.bam"), [])
    out = str(tmp_path / "out.bam")
    bam.merge_runs([a], out)
    text, refs, recs = bamcheck.read_bam(out)
    assert text == bam.output_header(REFS, LENS, sort_order="coordinate") and refs == list(zip(REFS, LENS)) and recs == []
    assert open(out, "rb").read() == open(a, "rb").read()


def test_sorted_runs_needs_device_records_and_one_shard(tmp_path):
    from portello_amd import pipeline

    with pytest.raises(ValueError, match="device_records"):
        pipeline.run_bam_to_bam("in.bam", str(tmp_path / "x.bam"), None, None, [], [], [], sorted_runs=True)
    with pytest.raises(ValueError, match="out_shards"):
        pipeline.run_bam_to_bam("in.bam", str(tmp_path / "x.bam"), None, None, [], [], [], device_records=True, sorted_runs=True, out_shards=2)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------

class DevSorter:
    """hand-made records through Engine.records_sort_dev"""

    def __init__(self):
        import torch

        self.torch = torch
        self.dev = torch.device("cuda", 0)
        self.index = api.Index(trd.hand_index(), 0)
        self.eng = api.Engine(self.index)

    def upload(self, data, off):
        t = self.torch
        raw = t.from_numpy(np.frombuffer(data, np.uint8).copy()).to(self.dev) if len(data) else t.zeros(16, dtype=t.uint8, device=self.dev)
        offs = t.from_numpy(np.ascontiguousarray(off, np.uint64).view(np.int64)).to(self.dev)
        t.cuda.synchronize()
        return raw, offs

    def sort(self, raw, offs, n_bytes, n_ref):
        return self.eng.records_sort_dev(raw.data_ptr(), n_bytes, offs.numel() - 1, offs.data_ptr(), n_ref)

    def result(self, so):
        n, nb = int(so.n_records), int(so.n_bytes)
        dl = self.eng.download
        return {"perm": dl(so.perm, np.uint32, n), "key": dl(so.key, np.uint64, n), "record_off": dl(so.record_off, np.uint64, n + 1),
                "bytes": dl(so.bytes, np.uint8, nb).tobytes(), "n_mapped": int(so.n_mapped)}

    def check(self, recs, n_ref, what="", bgzf=False):
        data, off = sx.concat(recs)
        e = sx.expect(data, off, n_ref)
        raw, offs = self.upload(data, off)
        so = self.sort(raw, offs, len(data), n_ref)
        assert int(so.n_records) == len(recs) and int(so.n_bytes) == len(data) and int(so.err_record) == 0xFFFFFFFF, what
        check_result(self.result(so), e, what)
        self.torch.cuda.synchronize()
        assert raw[:len(data)].cpu().numpy().tobytes() == data and np.array_equal(offs.cpu().numpy().view(np.uint64), off), what  # the input is unchanged
        if bgzf and recs:  # the sorted buffer composes with plo_bgzf_compress_dev as plo_records_out::bytes does
            import gzip
            bo = self.eng.bgzf_compress_dev(so.bytes, int(so.n_bytes), 0)
            assert gzip.decompress(self.eng.download(bo.blocks, np.uint8, int(bo.n_bytes)).tobytes()) == e["bytes"], what
        return so

    def close(self):
        self.eng.close()
        self.index.close()


@pytest.mark.gpu
def test_device_sizes_and_key_shapes():
    """6. the sizes and key shapes of the CPU tests through the C ABI, one context for all: buffers grow and are reused"""
    ds = DevSorter()
    for n in SIZES:
        so = ds.check(random_records(n, 25, 100 + n), 25, n, bgzf=n in (65, 4 * T + 3))
        assert n == 0 or so.sort_ms > 0
    for name, recs in sorted(key_shapes().items()):
        ds.check(recs, 25, name, bgzf="200 kB" in name)
        filler = random_records(2 * T + 1 - len(recs) // 2, 25, 5)
        k = len(filler) // 2
        ds.check(filler[:k] + recs + filler[k:], 25, name + " in three tiles")
    for n_ref in N_REFS:
        ds.check(random_records(T + 65, n_ref, 7 + n_ref) + [sx.make_record(n_ref - 1, sx.POS_MAX, 16, b"last"), sx.make_record(-1, 0, 4, b"tail")], n_ref, n_ref)
    ds.close()


@pytest.mark.gpu
def test_device_refusals():
    """7. every refusal returns its status and err_record, names the record and the field, and the context sorts the next call"""
    ds = DevSorter()
    field = {sx.ERR_OFFSET: "record_off", sx.ERR_SHORT: "36 bytes", sx.ERR_BLOCK: "block_size", sx.ERR_REFID: "refID", sx.ERR_POS: "pos"}
    good = random_records(T + 40, 25, 77)
    for name, (data, off, rec, kind) in sorted(refusals().items()):
        raw, offs = ds.upload(data, off)
        with pytest.raises(api.PortelloError, match=r"record %d .*%s" % (rec, field[kind])) as e:
            ds.sort(raw, offs, len(data), 25)
        assert e.value.status == abi.PLO_ERR_INVALID_ARG and e.value.err_record == rec, name
        ds.check(good, 25, "after " + name)
    raw, offs = ds.upload(*sx.concat(good))
    with pytest.raises(api.PortelloError) as e:
        ds.eng.records_sort_dev(0, 100, 3, offs.data_ptr(), 25)
    assert e.value.status == abi.PLO_ERR_INVALID_ARG
    ds.close()


@pytest.fixture(scope="module")
def small_bam(tmp_path_factory):
    from portello_amd import synth

    d = tmp_path_factory.mktemp("sortdev")
    w = synth.generate(synth.config("tiny", n_reads=300, seed=411, split_read_frac=0.3, sorted_reads=True))
    path = str(d / "reads.bam")
    meta = bamsynth.write_read_bam(w, path, level=6, n_unmapped=4)
    return w, path, meta


@pytest.mark.gpu
def test_device_sort_of_the_small_bam(small_bam):
    """8. lift -> finish -> records -> sort: a permutation, by perm, of plo_records_build_dev's records, in key order"""
    w, path, meta = small_bam
    index = api.Index(w.index_data(), 0)
    cn, rn = meta["contig_names"], bamsynth.ref_names(w)
    rd, win = trd.open_window(path)
    run = trd.DeviceRun(win, index, cn, rn, False)
    run.finish()
    run.sa()
    ro = run.eng.records_build_dev(run.ddesc, run.up.records_in(run.labels, False))
    n, nb = int(ro.n_records), int(ro.n_bytes)
    data, off = run.eng.download(ro.bytes, np.uint8, nb).tobytes(), run.eng.download(ro.record_off, np.uint64, n + 1)
    so = run.eng.records_sort_dev(ro.bytes, nb, n, ro.record_off, len(rn))
    dl = run.eng.download
    perm, key, soff, sdata = dl(so.perm, np.uint32, n), dl(so.key, np.uint64, n), dl(so.record_off, np.uint64, n + 1), dl(so.bytes, np.uint8, nb).tobytes()
    recs, srecs = trd._split(data, off), trd._split(sdata, soff)
    assert n > 300 and sorted(perm.tolist()) == list(range(n)) and srecs == [recs[i] for i in perm]
    assert [sx.key_of(r, len(rn)) for r in srecs] == key.tolist() and all(a <= b for a, b in zip(key[:-1].tolist(), key[1:].tolist()))
    assert 0 < int(so.n_mapped) < n and all((sx.key_of(r, len(rn)) >> 32 < len(rn)) == (j < int(so.n_mapped)) for j, r in enumerate(srecs))
    check_result({"perm": perm, "key": key, "record_off": soff, "bytes": sdata, "n_mapped": int(so.n_mapped)}, sx.expect(data, off, len(rn)))
    assert dl(ro.bytes, np.uint8, nb).tobytes() == data  # plo_records_build_dev's output stays
    run.eng.close()
    win.close()
    rd.close()
    index.close()


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [dict(), dict(device_bgzf=True, level=1), dict(emit_nm=True, emit_md=True)], ids=["plain", "device_bgzf", "nm_md"])
def test_bam_to_bam_sorted_runs(small_bam, tmp_path, extra):
    """9. run_bam_to_bam(device_records=True, sorted_runs=True): every run a complete SO:coordinate BAM in key order, named after its window;
    the runs' records are those of the same call with sorted_runs off; merge_runs of them is the Python sort by (key, run, index)"""
    from portello_amd import pipeline

    w, path, meta = small_bam
    ixd = w.index_data()
    index = api.Index(ixd, 0)
    cn, rn = meta["contig_names"], bamsynth.ref_names(w)
    lens = [len(s) for s in ixd.chrom_seq]
    kw = dict(window_reads=90, ramp=False, n_workers=2, io_threads=4, device_records=True, device_batch=True, **extra)
    off_path, runs_path = str(tmp_path / "unsorted.bam"), str(tmp_path / "lifted.bam")
    st0 = pipeline.run_bam_to_bam(path, off_path, index, ixd, cn, rn, lens, **kw)
    st = pipeline.run_bam_to_bam(path, runs_path, index, ixd, cn, rn, lens, sorted_runs=True, **kw)
    assert st0.out_paths == [off_path] and st0.sort_device_ms == 0 and "sort" not in st0.lift_detail_s
    assert "SO:unsorted" in bamcheck.read_bam(off_path)[0]
    assert st.reads == st0.reads == w.n_reads and st.records_out == st0.records_out and st.sort_device_ms > 0 and st.lift_detail_s.get("sort", 0) > 0
    assert len(st.out_paths) >= 3 and st.out_paths == sorted(st.out_paths) and not os.path.exists(runs_path)
    assert [os.path.basename(p) for p in st.out_paths] == ["lifted.r00w%06d.bam" % k for k in range(len(st.out_paths))]
    hdr = bam.output_header(rn, lens, sort_order="coordinate")
    runs = []
    for p in st.out_paths:
        text, refs, recs = bamcheck.read_bam(p)
        assert text == hdr and refs == list(zip(rn, lens)) and recs
        keys = [sx.key_of(r, len(rn)) for r in recs]
        assert keys == sorted(keys)
        assert open(p, "rb").read()[-28:] == open(off_path, "rb").read()[-28:]  # the EOF block
        runs.append(recs)
    assert sorted(r for run in runs for r in run) == sorted(bamcheck.read_bam(off_path)[2]) and sum(map(len, runs)) == st.records_out
    merged = str(tmp_path / "merged.bam")
    bam.merge_runs(st.out_paths, merged)
    text, refs, recs = bamcheck.read_bam(merged)
    assert text == hdr and recs == sx.merged(runs, len(rn))
    index.close()
