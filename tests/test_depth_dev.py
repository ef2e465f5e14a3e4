"""Depth of the records on the device: plo_depth_* (portello_amd/csrc/depth_core.hpp), portello_amd.depth and run_bam_to_bam(depth_out=...).

The yardstick is tests/depth_expect.py -- the rule of include/portello_liftover.h restated in plain Python, the depths counted base by base --
and, for the yardstick itself, the hand-worked vectors of tests/golden/depth_vectors.json.  All comparisons are of integers and text.  The CPU
tests run depth_core.hpp under the wave emulator (tests/emu/emu_depth.cpp) with PLO_DEPTH_TILE = 12, shuffled lane orders and several wave
counts, and once more in a program built with AddressSanitizer + UBSan where every array sits in a heap block of its exact size.  The GPU
tests run the C ABI on the device and the pipeline mode.

Mutations this file is meant to catch (each was tried on depth_core.hpp):
  * dropping the carry across the 64-op seam (`open` reset to false at every trip of depth_add_record) fails
    test_op_counts[65], test_op_counts[129] and test_fuzz[1]: the stretch that crosses the seam is opened a second time;
  * dropping the slot's extra entry (depth_slot_entries without the + 1) fails test_chromosome_lengths and the hand vector "a chromosome of
    length 0 has no run": the slots are not the stated ones, and a record that ends at the end of a chromosome of 63 bases would put its
    -1 into the next chromosome's first base."""
import json
import os
import random
import struct
import threading

import numpy as np
import pytest

import depth_expect as dx
import emu_depth_lib as edl
import index_expect as ix
from portello_amd import abi, api, depth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "depth_vectors.json")))
T = edl.TILE
NO_RECORD = 0xFFFFFFFF
OP_COUNTS = [0, 1, 63, 64, 65, 129]
CHROM_LENS = [0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, T * T + 1]
CODES = "MIDNSHP=X"


def cigar(text):
    out, n = [], ""
    for ch in text:
        if ch.isdigit():
            n += ch
        else:
            out.append(ix.op(int(n), CODES.index(ch)))
            n = ""
    return out


def rec(ref, pos, flag=0, ops=(), name=b"r", l_seq=0, aux=b"", n_cigar=None, block_size=None, l_seq_says=None):
    """a record with l_seq bases and qualities (zeros) in front of its aux fields; ops: words or CIGAR text; n_cigar / block_size /
    l_seq_says: the fields, when they shall lie"""
    ops = cigar(ops) if isinstance(ops, str) else list(ops)
    body = struct.pack("<iiBBHHHIiii", ref, pos, len(name), 0, 0, len(ops) if n_cigar is None else n_cigar, flag, l_seq if l_seq_says is None else l_seq_says, -1, -1, 0) + name
    body += struct.pack("<%dI" % len(ops), *ops) + bytes((l_seq + 1) // 2 + l_seq) + aux
    return struct.pack("<I", len(body) if block_size is None else block_size) + body


def cg_field(ops, count=None):
    return b"CGBI" + struct.pack("<I", len(ops) if count is None else count) + struct.pack("<%dI" % len(ops), *ops)


def placeholder(ref, pos, real, flag=0, l_seq=7, front=b"XAZabc\0NMi\x05\0\0\0", cg=True, count=None):
    """the real ops behind the placeholder <l_seq>S<ref_len>N, as BAM stores more than 65 535 ops (the rule asks for the form, not the count)"""
    ref_len = sum(o >> 4 for o in real if (o & 15) in dx.REF)
    return rec(ref, pos, flag, [ix.op(l_seq, 4), ix.op(ref_len, 3)], b"long", l_seq, front + (cg_field(real, count) if cg else b""))


def golden_records(v):
    return [rec(r, p, f, c, b"g%d" % k) for k, (r, p, f, c) in enumerate(v["records"])]


def rand_ops(rng, n, max_len=6, codes=(0, 0, 1, 2, 3, 4, 5, 6, 7, 7, 8, 8, 11)):
    return [ix.op(rng.choice([0, 1, 1, rng.randrange(1, max_len)]), rng.choice(codes)) for _ in range(n)]


def fit(rng, ops, ref_len):
    """a position at which the ops end inside ref_len, or None"""
    span = dx.covered(ops, 0)[1]
    return rng.randrange(ref_len - span + 1) if span <= ref_len else None


def random_records(rng, ref_len, n, max_ops=12):
    out = []
    while len(out) < n:
        r = rng.randrange(len(ref_len))
        ops = rand_ops(rng, rng.randrange(max_ops))
        pos = fit(rng, ops, ref_len[r])
        if pos is None:
            continue
        flag = rng.choice([0, 0, 0, 16, 0x800, 0x100, 0x400, 4, 1 | 16])
        form = rng.randrange(8)
        if form == 0:
            out.append(placeholder(r, pos, ops, flag))
        elif form == 1:
            out.append(rec(rng.choice([-1, r]), rng.choice([-1, pos]), flag | 4, ops, b"u%d" % len(out)))
        else:
            out.append(rec(r, pos, flag, ops, b"q%d" % len(out), rng.randrange(5), bytes(rng.randrange(256) for _ in range(rng.randrange(9)))))
    return out


class Emu:
    def __init__(self, ref_len, **kw):
        self.o = edl.EmuDepth(ref_len, **kw)

    def __enter__(self):
        return self.o

    def __exit__(self, *a):
        self.o.close()


def check_results(what, ref_len, dep, arr, first_sums, runs, w):
    assert np.array_equal(arr, dx.array(dep, ref_len)), what
    wf, ws = dx.windows(dep, w)
    assert np.array_equal(first_sums[0], wf) and np.array_equal(first_sums[1], ws), (what, w)
    assert np.array_equal(runs, dx.runs(dep)), what


def emu_check(recs, ref_len, deletions=False, exclude=dx.EXCLUDE_DEFAULT, ws=(1, 5), what="", geometries=((0, 1), (1, 3), (2, 8))):
    data, off = ix.concat(recs)
    assert dx.first_offender(data, off, ref_len, exclude) is None, what
    dep, n_counted = dx.depths(recs, ref_len, exclude, deletions)
    for seed, n_waves in geometries:
        with Emu(ref_len, exclude=exclude, deletions=deletions) as o:
            assert np.array_equal(o.slots(), dx.slot_off(ref_len)), what
            assert o.add(data, off, seed, n_waves) == (abi.PLO_OK, n_counted, NO_RECORD, 0), (what, seed)  # -4: the wave and the one-thread rule disagree
            assert np.array_equal(o.array(), dx.differences(dep, ref_len)), (what, seed)
            assert o.finish(seed) == abi.PLO_OK
            st_r, runs = o.runs(seed)
            assert st_r == abi.PLO_OK
            for w in ws:
                st_w, first, sums = o.windows(w, seed, n_waves)
                assert st_w == abi.PLO_OK
                check_results((what, seed), ref_len, dep, o.array(), (first, sums), runs, w)
    return dep


# ---- CPU: the yardstick -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("v", GOLDEN["vectors"], ids=lambda v: v["name"])
def test_expectation_by_hand(v):
    """the restatement gives the hand-worked runs"""
    recs = golden_records(v)
    assert dx.first_offender(*ix.concat(recs), v["ref_len"]) is None
    dep, n = dx.depths(recs, v["ref_len"], deletions=v["deletions"])
    assert n == v["n_counted"] and dx.runs(dep).tolist() == [tuple(r) for r in v["runs"]]


@pytest.mark.parametrize("v", GOLDEN["refused"], ids=lambda v: v["name"])
def test_expectation_of_refusals_by_hand(v):
    assert dx.first_offender(*ix.concat(golden_records(v)), v["ref_len"]) == (v["err_record"], v["err_kind"])


def test_mean_text():
    """two decimals from the integer sum, round-half-even"""
    for total, n, want in ((0, 5, "0.00"), (1, 8, "0.12"), (3, 8, "0.38"), (5, 8, "0.62"), (1, 3, "0.33"), (2, 3, "0.67"), (1, 200, "0.00"), (3, 200, "0.02"), (1005, 1000, "1.00"),
                           (1015, 1000, "1.02"), (10 ** 15 + 1, 2, "500000000000000.50"), (7, 1, "7.00")):
        assert dx.mean_text(total, n) == want == depth.format_mean(total, n), (total, n)


# ---- CPU: depth_core.hpp under the wave emulator ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("v", GOLDEN["vectors"], ids=lambda v: v["name"])
def test_hand_vectors(v):
    """1. the hand vectors: the runs are the hand-worked ones, array and windows the restatement's"""
    recs = golden_records(v)
    emu_check(recs, v["ref_len"], deletions=v["deletions"], ws=(1, 3, 50), what=v["name"])
    with Emu(v["ref_len"], deletions=v["deletions"]) as o:
        assert o.add(*ix.concat(recs))[:2] == (abi.PLO_OK, v["n_counted"]) and o.finish() == abi.PLO_OK
        assert o.runs()[1].tolist() == [tuple(r) for r in v["runs"]]


@pytest.mark.parametrize("v", GOLDEN["refused"], ids=lambda v: v["name"])
def test_hand_refusals(v):
    with Emu(v["ref_len"]) as o:
        assert o.add(*ix.concat(golden_records(v)))[0::2] == (abi.PLO_ERR_INVALID_ARG, v["err_record"]) and not o.array().any()


def seam_record(n_ops, kind):
    """n_ops ops around the 64-op seam.  kind 0: every op covers -- one stretch across every seam; kind 1: a D sits on op 64 (and on 63 for the
    counts below), covers on both sides; kind 2: insertions and clips around the seam, which do not break the stretch"""
    ops = [ix.op(1 + k % 3, (7, 8, 0)[k % 3]) for k in range(n_ops)]
    if kind == 1 and n_ops:
        ops[min(64, n_ops - 1)] = ix.op(2, 2)
    if kind == 2:
        for k in (62, 63, 64, 65):
            if k < n_ops:
                ops[k] = ix.op(3, (1, 4, 6, 1)[k - 62])
    return ops


@pytest.mark.parametrize("n_ops", OP_COUNTS)
def test_op_counts(n_ops):
    """2. op counts around the wave's width: a stretch crossing the 64-op seam costs one +1 and one -1, a D sitting on the seam splits it
    (or, with count_deletions, does not)"""
    ref_len = [400]
    recs = [rec(0, 3 + k, 0, seam_record(n_ops, k), b"s%d" % k) for k in range(3)]
    for deletions in (False, True):
        dep = emu_check(recs, ref_len, deletions=deletions, what=(n_ops, deletions), geometries=((0, 1), (1, 2)))
        if n_ops >= 65:
            span = dx.covered(seam_record(n_ops, 0), 3)[1]
            assert dep[0][3] == 1 and dep[0][span - 1] >= 1 and dep[0].max() == 3
    if n_ops >= 65:  # the number of atomics shows in the differences: the all-covering record alone leaves exactly one +1 and one -1
        with Emu(ref_len) as o:
            assert o.add(*ix.concat(recs[:1]))[0] == abi.PLO_OK
            a = o.array()
            assert sorted(a[a != 0].tolist()) == [-1, 1]


def test_long_cigar_through_cg():
    """3. a 65 536-op record through the placeholder and CG:B,I; a placeholder without CG is taken as it stands (its N covers nothing)"""
    rng = random.Random(5)
    real = [ix.op(1, rng.choice([7, 7, 8, 2, 1])) for _ in range(65536)]
    span = dx.covered(real, 0)[1]
    ref_len = [span + 150, 40]
    recs = [rec(0, 3, 0, "5M", b"short"), placeholder(0, 100, real), placeholder(0, 20, cigar("4=2D4="), cg=False), placeholder(1, 1, cigar("3=2N3X"), front=b""),
            rec(1, 0, 0, [ix.op(9, 4), ix.op(5, 3)], b"not the form", 7, cg_field(cigar("5M")))]  # 9S: l_seq is 7, so the in-record ops stand
    assert dx.real_cigar(recs[1]) == real and dx.real_cigar(recs[2]) == [ix.op(7, 4), ix.op(10, 3)] and dx.real_cigar(recs[4]) == [ix.op(9, 4), ix.op(5, 3)]
    for deletions in (False, True):
        dep = emu_check(recs, ref_len, deletions=deletions, ws=(500,), what="long", geometries=((1, 2),))
        assert dep[0][20:30].sum() == 0 and dep[0][100:100 + span].max() == 1 and dep[1].tolist()[:8] == [0, 1, 1, 1, 0, 0, 1, 1]


def test_chromosome_lengths():
    """4. chromosome lengths around the slot and the tile, T * T + 1 among them: every level of the scan has a seam.  Each chromosome's last
    base and the next one's first base are covered; runs and windows at those borders; w = 1, a w that divides a length, one that does not,
    one greater than every length"""
    ref_len = CHROM_LENS
    recs = []
    for r, n in enumerate(ref_len):
        if n:
            recs.append(rec(r, n - 1, 0, "1M", b"last%d" % r))
            recs.append(rec(r, 0, 16, "1=", b"first%d" % r))
            recs.append(rec(r, 0, 0, [ix.op(n, 0)], b"whole%d" % r))
            recs.append(rec(r, n // 2, 0, [ix.op(n - n // 2, 8)], b"half%d" % r))
    recs.append(rec(0, 0, 0, "3S", b"on the empty one"))
    dep = emu_check(recs, ref_len, ws=(1, T + 1, 7, 1000), what="lengths")
    assert dep[2][62] == 3 and dep[3][0] == 2  # the 63-base chromosome's last base, the next one's first
    assert T * T + 1 in ref_len and 65 % (T + 1) == 0 and 65 % 7 != 0
    runs = dx.runs(dep)
    assert not (runs["ref_id"] == 0).any() and all((runs["end"][runs["ref_id"] == r]).max() == n for r, n in enumerate(ref_len) if n)


def test_order_and_splits():
    """5. the same records shuffled, and split over several add calls with other wave counts, give an identical array"""
    rng = random.Random(17)
    ref_len = [700, 65, 300]
    recs = random_records(rng, ref_len, 150)
    dep, n_counted = dx.depths(recs, ref_len)
    want = dx.differences(dep, ref_len)
    arrays = []
    for k in range(3):
        order = list(recs)
        random.Random(k).shuffle(order)
        cuts = sorted(random.Random(40 + k).sample(range(len(order)), k * 2))
        pieces = [order[a:b] for a, b in zip([0] + cuts, cuts + [len(order)])]
        with Emu(ref_len) as o:
            total = 0
            for j, piece in enumerate(pieces):
                st, nc, er, ek = o.add(*ix.concat(piece), order_seed=j + k, n_waves=1 + (3 * j + k) % 5)
                assert (st, er, ek) == (abi.PLO_OK, NO_RECORD, 0)
                total += nc
            assert total == n_counted
            arrays.append(o.array())
    assert all(np.array_equal(a, want) for a in arrays)


def refusals(ref_len=(5000, 300, 64)):
    """name -> (data, off, lowest offender, kind): inside a buffer of otherwise good records, behind the first wave's worth of them, and in
    front of a SECOND offender of another kind"""
    rng = random.Random(77)
    good = random_records(rng, list(ref_len), 130)
    at, second = 70, 100

    def two(bad, later=None):
        recs = list(good)
        recs[at] = bad
        recs[second] = rec(0, 0, 0, "5M", b"cut", n_cigar=9) if later is None else later
        return ix.concat(recs)

    end_bad = rec(1, 298, 0, "3M", b"beyond")
    out = {}
    data, off = two(rec(0, 0, 0, "1M"), end_bad)
    o = off.copy()
    o[at + 1] = o[at] - 1
    out["record_off decreases"] = (data, o, at, dx.ERR_OFFSET)
    out["shorter than 36 bytes"] = two(rec(0, 5)[:35]) + (at, dx.ERR_SHORT)
    out["block_size disagrees"] = two(rec(0, 5, 0, "4M", block_size=41)) + (at, dx.ERR_BLOCK)
    out["refID == n_ref"] = two(rec(len(ref_len), 5)) + (at, dx.ERR_REFID)
    out["pos == -2"] = two(rec(0, -2)) + (at, dx.ERR_POS)
    out["the CIGAR one op past the record"] = two(rec(0, 5, 0, [ix.op(1, 0)] * 70, b"cut", n_cigar=71), end_bad) + (at, dx.ERR_CIGAR)
    out["an uncounted record is checked too"] = two(rec(-1, -1, 4, [ix.op(1, 0)] * 3, b"cut", n_cigar=4), end_bad) + (at, dx.ERR_CIGAR)
    out["a malformed field in front of CG"] = two(placeholder(0, 5, cigar("4M"), front=b"XAZno end", cg=False)) + (at, dx.ERR_AUX)
    out["an unknown type in front of CG"] = two(placeholder(0, 5, cigar("4M"), front=b"XAq\0")) + (at, dx.ERR_AUX)
    out["CG leaves the record"] = two(placeholder(0, 5, cigar("4M2I4M"), count=4)) + (at, dx.ERR_AUX)
    out["CG leaves the record, uncounted"] = two(placeholder(0, 5, cigar("4M"), flag=0x400, count=1 << 30)) + (at, dx.ERR_AUX)
    out["the aux fields begin behind the end"] = two(rec(0, 5, 0, [ix.op(900, 4), ix.op(5, 3)], b"l_seq lies", 0, l_seq_says=900)) + (at, dx.ERR_AUX)
    out["one base beyond ref_len"] = two(end_bad) + (at, dx.ERR_END)
    out["the real CIGAR in CG reaches beyond ref_len"] = two(placeholder(2, 60, cigar("2=1D2X"))) + (at, dx.ERR_END)
    return out, list(ref_len), good


def test_refusal_cases_cover_every_kind():
    cases, ref_len, _ = refusals()
    assert {k for _, _, _, k in cases.values()} == set(range(1, 9))
    for name, (data, off, r, kind) in cases.items():
        assert dx.first_offender(data, off, ref_len) == (r, kind), name


@pytest.mark.parametrize("name", sorted(refusals()[0]))
def test_refusal(name):
    """6. every kind as the lowest of two offenders; the array after a refused add equals the array before it"""
    cases, ref_len, good = refusals()
    data, off, r, kind = cases[name]
    for seed, n_waves in ((0, 1), (1, 4), (2, 7)):
        with Emu(ref_len) as o:
            assert o.add(*ix.concat(good), seed, n_waves)[0] == abi.PLO_OK
            before = o.array()
            assert before.any()
            assert o.add(data, off, seed, n_waves) == (abi.PLO_ERR_INVALID_ARG, 0, r, kind), name
            assert np.array_equal(o.array(), before), name


def test_states():
    """7. add after finish, windows and runs before finish, a second finish; reset zeroes the array and reopens the object"""
    ref_len = [100, 30]
    recs = [rec(0, 10, 0, "20M"), rec(1, 0, 0, "30M")]
    data, off = ix.concat(recs)
    with Emu(ref_len) as o:
        assert o.windows(10)[0] == abi.PLO_ERR_INVALID_ARG and o.runs()[0] == abi.PLO_ERR_INVALID_ARG
        assert o.add(data, off)[0] == abi.PLO_OK and o.finish() == abi.PLO_OK
        after = o.array()
        assert o.add(data, off)[0] == abi.PLO_ERR_INVALID_ARG and o.finish() == abi.PLO_ERR_INVALID_ARG and np.array_equal(o.array(), after)
        assert o.windows(0)[0] == abi.PLO_ERR_INVALID_ARG and o.windows(10)[0] == abi.PLO_OK
        assert o.reset() == abi.PLO_OK and not o.array().any() and o.runs()[0] == abi.PLO_ERR_INVALID_ARG
        assert o.add(data, off)[0] == abi.PLO_OK and o.add(data, off)[0] == abi.PLO_OK and o.finish() == abi.PLO_OK
        assert np.array_equal(o.array(), 2 * after)
    with Emu([]) as o:  # no chromosome at all
        assert o.add(*ix.concat([rec(-1, -1, 4)]))[:2] == (abi.PLO_OK, 0) and o.finish() == abi.PLO_OK and len(o.runs()[1]) == 0 and len(o.windows(5)[2]) == 0


@pytest.mark.parametrize("seed", range(4))
def test_fuzz(seed):
    """8. seeded: 3 chromosomes of up to 5 000 bases, 200 records, against the restatement"""
    rng = random.Random(1000 + seed)
    ref_len = [rng.randrange(1, 5001) for _ in range(3)]
    recs = random_records(rng, ref_len, 200, max_ops=rng.choice([6, 30, 140]))
    exclude = rng.choice([dx.EXCLUDE_DEFAULT, 0, 0x10])
    dep = emu_check(recs, ref_len, deletions=bool(seed & 1), exclude=exclude, ws=(rng.randrange(1, 64), rng.randrange(64, 900)), what=seed, geometries=((seed, 1 + seed),))
    assert sum(int(d.sum()) for d in dep) > 0


def test_asan_program(tmp_path):
    """9. the same harness as a stand-alone program with ASan + UBSan, every array in a heap block of its exact size: hand vectors, op counts,
    chromosome lengths, a CG record, a fuzz case, refusals"""
    cases, wants = [], []

    def case(recs, ref_len, deletions=False, w=5, pieces=1):
        step = (len(recs) + pieces - 1) // pieces or 1
        adds = [ix.concat(recs[a:a + step]) + (len(cases) % 3, 1 + len(cases) % 4) for a in range(0, max(1, len(recs)), step)]
        cases.append((ref_len, dx.EXCLUDE_DEFAULT, deletions, w, adds))
        wants.append((recs, ref_len, deletions, w))

    for v in GOLDEN["vectors"]:
        case(golden_records(v), v["ref_len"], v["deletions"], 3)
    for n_ops in OP_COUNTS:
        case([rec(0, 3 + k, 0, seam_record(n_ops, k)) for k in range(3)], [400], n_ops & 1, 64)
    case([rec(r, n - 1, 0, "1M") for r, n in enumerate(CHROM_LENS) if n] + [rec(r, 0, 0, [ix.op(n, 7)]) for r, n in enumerate(CHROM_LENS) if n], CHROM_LENS, False, T + 1, 2)
    case([placeholder(0, 9, rand_ops(random.Random(3), 300, codes=(7, 8, 2, 1))), placeholder(0, 2, cigar("3M"), cg=False)], [900], True, 100)
    rng = random.Random(99)
    case(random_records(rng, [900, 64, 1300], 120), [900, 64, 1300], False, 37, 3)
    ref_cases, ref_lens, good = refusals()
    for name, (data, off, r, kind) in sorted(ref_cases.items()):
        cases.append((ref_lens, dx.EXCLUDE_DEFAULT, False, 50, [ix.concat(good) + (0, 3), (data, off, 1, 3)]))
        wants.append((good, ref_lens, False, 50, (r, kind)))
    rc, err, res = edl.run_asan(cases, str(tmp_path))
    assert rc == 0, err[-3000:]
    assert "ERROR" not in err and "runtime error" not in err, err[-3000:]
    for got, want in zip(res, wants):
        recs, ref_len, deletions, w = want[:4]
        dep, n_counted = dx.depths(recs, ref_len, deletions=deletions)
        if len(want) == 5:
            assert got["adds"][0][0] == abi.PLO_OK and got["adds"][1][:3] == (abi.PLO_ERR_INVALID_ARG,) + want[4]
        else:
            assert all(a[0] == abi.PLO_OK for a in got["adds"]) and sum(a[3] for a in got["adds"]) == n_counted
        assert np.array_equal(got["diff"], dx.differences(dep, ref_len))
        check_results(want[1:], ref_len, dep, got["depth"], (got["win_first"], got["sums"]), got["runs"], w)


# ---- CPU: Python ------------------------------------------------------------------------------------------------------------------------------

def test_writers(tmp_path):
    """10. the text of the two files"""
    names, ref_len = ["chr1", "chrM", "empty"], [10, 3, 0]
    dep = [np.array([0, 0, 1, 1, 2, 2, 2, 1, 0, 0]), np.array([5, 5, 5]), np.zeros(0, np.int64)]
    runs = dx.runs(dep)
    p1, p2 = str(tmp_path / "x.per-base.bed"), str(tmp_path / "x.regions.bed")
    depth.write_per_base(p1, names, runs.astype(abi.DEPTH_RUN_DTYPE))
    assert open(p1).read() == "chr1\t0\t2\t0\nchr1\t2\t4\t1\nchr1\t4\t7\t2\nchr1\t7\t8\t1\nchr1\t8\t10\t0\nchrM\t0\t3\t5\n" == dx.per_base_text(names, runs)
    first, sums = dx.windows(dep, 4)
    depth.write_regions(p2, names, ref_len, 4, first, sums)
    assert open(p2).read() == "chr1\t0\t4\t0.50\nchr1\t4\t8\t1.75\nchr1\t8\t10\t0.00\nchrM\t0\t3\t5.00\n" == dx.regions_text(names, ref_len, 4, first, sums)
    first, sums = dx.windows(dep, 8)
    depth.write_regions(p2, names, ref_len, 8, first, sums)
    assert open(p2).read() == "chr1\t0\t8\t1.12\nchr1\t8\t10\t0.00\nchrM\t0\t3\t5.00\n"  # 9 / 8 = 1.125: half to even


def test_depth_out_needs_device_records(tmp_path):
    from portello_amd import pipeline

    with pytest.raises(ValueError, match="device_records"):
        pipeline.run_bam_to_bam("in.bam", str(tmp_path / "x.bam"), None, None, [], [], [], depth_out=str(tmp_path / "d"))
    with pytest.raises(ValueError, match="depth_window"):
        pipeline.run_bam_to_bam("in.bam", str(tmp_path / "x.bam"), None, None, [], [], [], device_records=True, depth_out=str(tmp_path / "d"), depth_window=0)


def test_abi_structs():
    import ctypes as C

    assert abi.PLO_API_VERSION >= 19 and abi.DEPTH_EXCLUDE_DEFAULT == 0x704 == dx.EXCLUDE_DEFAULT
    assert C.sizeof(abi.PloDepthRun) == 16 == abi.DEPTH_RUN_DTYPE.itemsize and abi.DEPTH_RUN_DTYPE == dx.RUN
    assert [(n, abi.DEPTH_RUN_DTYPE.fields[n][1]) for n in abi.DEPTH_RUN_DTYPE.names] == [(f[0], getattr(abi.PloDepthRun, f[0]).offset) for f in abi.PloDepthRun._fields_]
    assert C.sizeof(abi.PloDepthOpts) == 8 and C.sizeof(abi.PloDepthIn) == 32 and abi.PloDepthIn.record_off.offset == 24
    assert C.sizeof(abi.PloDepthAddOut) == 20 and abi.PloDepthAddOut.add_ms.offset == 16
    assert C.sizeof(abi.PloDepthInfo) == 48 and abi.PloDepthInfo.bytes_allocated.offset == 24 and abi.PloDepthInfo.finished.offset == 44
    assert C.sizeof(abi.PloDepthWindowsOut) == 32 and abi.PloDepthWindowsOut.windows_ms.offset == 24
    assert C.sizeof(abi.PloDepthRunsOut) == 24 and abi.PloDepthRunsOut.runs_ms.offset == 16
    text = open(os.path.join(HERE, "..", "include", "portello_liftover.h")).read()
    for name, cls in (("plo_depth_opts", abi.PloDepthOpts), ("plo_depth_info", abi.PloDepthInfo), ("plo_depth_in", abi.PloDepthIn), ("plo_depth_add_out", abi.PloDepthAddOut),
                      ("plo_depth_windows_out", abi.PloDepthWindowsOut), ("plo_depth_run", abi.PloDepthRun), ("plo_depth_runs_out", abi.PloDepthRunsOut)):
        body = text[text.index("typedef struct %s {" % name):]
        body = body[:body.index("} %s;" % name)]
        import re
        declared = [n for line in body.splitlines()[1:] for n in re.findall(r"(\w+)\s*(?:,|;)", line.split("/*")[0])]
        assert declared == [f[0] for f in cls._fields_], name


def test_context_and_object_free_what_they_hold():
    """the add's scratch on the context is released with it, its events are destroyed by the one loop (test_index_dev checks the loops)"""
    src = open(os.path.join(HERE, "..", "portello_amd", "csrc", "engine.hip")).read()
    body = src[src.index("void plo_ctx_destroy(plo_ctx *c) {"):]
    body = body[:body.index("\n}\n")]
    assert "&c->dp_plan" in body and "&c->dp_blk" in body and "&c->h_dp" in body and "c->dpev[i]" in body


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------

def shipped_tile():
    import re

    return int(re.search(r"#define PLO_DEPTH_TILE (\d+)", open(os.path.join(HERE, "..", "portello_amd", "csrc", "depth_core.hpp")).read()).group(1))


class Dev:
    """hand-made records through depth.DeviceDepth on one engine"""

    def __init__(self):
        import torch

        import test_records_dev as trd

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

    def add(self, obj, recs, eng=None):
        data, off = ix.concat(recs)
        raw, offs = self.upload(data, off)
        return obj.add(eng or self.eng, raw.data_ptr(), len(data), len(recs), offs.data_ptr())

    def check(self, recs, ref_len, deletions=False, exclude=dx.EXCLUDE_DEFAULT, ws=(1, 5), pieces=1, what=""):
        assert dx.first_offender(*ix.concat(recs), ref_len, exclude) is None, what
        dep, n_counted = dx.depths(recs, ref_len, exclude, deletions)
        obj = depth.DeviceDepth(self.eng, ref_len, exclude, deletions)
        info = obj.info()
        assert int(info.n_entries) == dx.slot_off(ref_len)[-1] and int(info.bytes_allocated) >= 4 * int(info.n_entries) and not info.finished, what
        assert np.ctypeslib.as_array(info.slot_off, (len(ref_len) + 1,)).tolist() == dx.slot_off(ref_len), what
        step = (len(recs) + pieces - 1) // pieces or 1
        total = 0
        for a in range(0, max(1, len(recs)), step):
            ao = self.add(obj, recs[a:a + step])
            assert (int(ao.err_record), int(ao.err_kind)) == (NO_RECORD, 0), what
            total += int(ao.n_counted)
        assert total == n_counted, what
        assert np.array_equal(obj.array(self.eng), dx.differences(dep, ref_len)), what
        obj.finish(self.eng)
        assert obj.info().finished
        runs = obj.runs(self.eng)
        for w in ws:
            first, sums, _ = obj.windows(self.eng, w)
            check_results(what, ref_len, dep, obj.array(self.eng), (first, sums), runs, w)
        obj.close()
        return runs

    def close(self):
        self.eng.close()
        self.index.close()


@pytest.mark.gpu
def test_device_vectors_and_shapes():
    """11. the hand vectors, op counts, chromosome lengths around the slot and the shipped tile, the CG record and a fuzz case through the C
    ABI, one context for all"""
    d = Dev()
    for v in GOLDEN["vectors"]:
        runs = d.check(golden_records(v), v["ref_len"], deletions=v["deletions"], ws=(1, 3, 50), what=v["name"])
        assert runs.tolist() == [tuple(r) for r in v["runs"]], v["name"]
    for n_ops in OP_COUNTS:
        for deletions in (False, True):
            d.check([rec(0, 3 + k, 0, seam_record(n_ops, k), b"s%d" % k) for k in range(3)], [400], deletions=deletions, ws=(64,), what=n_ops)
    tile = shipped_tile()
    lens = [0, 1, 63, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 1]
    recs = []
    for r, n in enumerate(lens):
        if n:
            recs += [rec(r, n - 1, 0, "1M"), rec(r, 0, 16, "1="), rec(r, 0, 0, [ix.op(n, 0)]), rec(r, n // 2, 0, [ix.op(n - n // 2, 8)])]
    d.check(recs, lens, ws=(1, 13, 7, 5000), pieces=2, what="lengths")
    rng = random.Random(5)
    real = [ix.op(1, rng.choice([7, 7, 8, 2, 1])) for _ in range(65536)]
    span = dx.covered(real, 0)[1]
    d.check([rec(0, 3, 0, "5M"), placeholder(0, 100, real), placeholder(0, 20, cigar("4=2D4="), cg=False)], [span + 150], deletions=True, ws=(500,), what="long")
    rng = random.Random(2024)
    ref_len = [4999, 64, 3100]
    d.check(random_records(rng, ref_len, 200, max_ops=140), ref_len, ws=(17, 500), pieces=3, what="fuzz")
    d.close()


@pytest.mark.gpu
def test_device_refusals_and_states():
    """12. every refusal returns its status, err_record and err_kind, names the record, and leaves the array as it was; the order of calls"""
    d = Dev()
    cases, ref_len, good = refusals()
    obj = depth.DeviceDepth(d.eng, ref_len)
    d.add(obj, good)
    before = obj.array(d.eng)
    assert before.any()
    for name, (data, off, r, kind) in sorted(cases.items()):
        raw, offs = d.upload(data, off)
        with pytest.raises(api.PortelloError, match=r"record %d " % r) as e:
            obj.add(d.eng, raw.data_ptr(), len(data), len(off) - 1, offs.data_ptr())
        assert (e.value.status, e.value.err_record, e.value.err_kind) == (abi.PLO_ERR_INVALID_ARG, r, kind), name
        assert np.array_equal(obj.array(d.eng), before), name
    for v in GOLDEN["refused"]:
        o2 = depth.DeviceDepth(d.eng, v["ref_len"])
        with pytest.raises(api.PortelloError) as e:
            d.add(o2, golden_records(v))
        assert (e.value.err_record, e.value.err_kind) == (v["err_record"], v["err_kind"]) and not o2.array(d.eng).any()
        o2.close()
    for call in (lambda: obj.windows(d.eng, 10), lambda: obj.runs(d.eng)):
        with pytest.raises(api.PortelloError, match="not finished") as e:
            call()
        assert e.value.status == abi.PLO_ERR_INVALID_ARG
    obj.finish(d.eng)
    dep, _ = dx.depths(good, ref_len)
    assert np.array_equal(obj.array(d.eng), dx.array(dep, ref_len))
    for call in (lambda: d.add(obj, good), lambda: obj.finish(d.eng)):
        with pytest.raises(api.PortelloError, match="is finished") as e:
            call()
        assert e.value.status == abi.PLO_ERR_INVALID_ARG
    with pytest.raises(api.PortelloError, match="1 or more"):
        obj.windows(d.eng, 0)
    assert np.array_equal(obj.array(d.eng), dx.array(dep, ref_len))
    obj.reset(d.eng)
    assert not obj.array(d.eng).any() and not obj.info().finished
    d.add(obj, good)
    d.add(obj, good)
    obj.finish(d.eng)
    assert np.array_equal(obj.array(d.eng), 2 * dx.array(dep, ref_len))
    obj.close()
    with pytest.raises(api.PortelloError) as e:
        depth.DeviceDepth(d.eng, [5, -1])
    assert e.value.status == abi.PLO_ERR_INVALID_ARG
    d.close()


def interval_records(rng, n, ref_len, max_span):
    out = []
    for k in range(n):
        span = rng.randrange(1, max_span)
        out.append(rec(0, rng.randrange(ref_len - span + 1), 0, [ix.op(span, 0)], b"i"))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("top_tiles", [2, 65], ids=["two top values", "two trips of the top wave"])
def test_device_scan_levels(top_tiles):
    """13. the scan at the smallest entry counts that give every level more than one tile at the shipped PLO_DEPTH_TILE: more than T * T
    entries (two sums of sums), and more than 64 T * T (the one wave at the top takes a second trip).  The expectation is numpy's: the
    differences by np.add.at, the depths by cumsum, the window sums by reduceat, the runs from the positions where the depth changes"""
    tile = shipped_tile()
    n = (top_tiles - 1) * tile * tile  # entries: n + 64
    assert (n + 64 + tile - 1) // tile > (top_tiles - 1) * tile
    d = Dev()
    rng = random.Random(top_tiles)
    recs = interval_records(rng, 3000, n, 40_000) + [rec(0, 0, 0, [ix.op(n, 7)], b"whole"), rec(0, n - 1, 0, "1X", b"last")]
    diff = np.zeros(n + 64, np.int64)
    for r in recs:
        pos, span = ix.fields(r)[1], dx.real_cigar(r)[0] >> 4
        diff[pos] += 1
        diff[pos + span] -= 1
    want = np.cumsum(diff)
    obj = depth.DeviceDepth(d.eng, [n])
    assert int(d.add(obj, recs).n_counted) == len(recs)
    assert np.array_equal(obj.array(d.eng), diff.astype(np.int32))
    obj.finish(d.eng)
    assert np.array_equal(obj.array(d.eng), want.astype(np.int32)) and want[n:].max() == 0 and want[:n].min() >= 1
    w = 4096 + 1
    first, sums, _ = obj.windows(d.eng, w)
    assert first.tolist() == [0, (n + w - 1) // w] and np.array_equal(sums, np.add.reduceat(want[:n], np.arange(0, n, w)).astype(np.uint64))
    runs = obj.runs(d.eng)
    beg = np.concatenate([[0], 1 + np.flatnonzero(want[1:n] != want[:n - 1])])
    assert np.array_equal(runs["beg"], beg) and np.array_equal(runs["end"], np.concatenate([beg[1:], [n]])) and np.array_equal(runs["depth"], want[beg]) and not runs["ref_id"].any()
    obj.close()
    d.close()


@pytest.mark.gpu
def test_two_engines_add_at_once():
    """14. two engines on two Python threads add disjoint halves of a record set into one object at the same time"""
    d = Dev()
    eng2 = api.Engine(d.index)
    rng = random.Random(8)
    ref_len = [30_000, 700, 64]
    recs = random_records(rng, ref_len, 4000, max_ops=40)
    dep, n_counted = dx.depths(recs, ref_len)
    obj = depth.DeviceDepth(d.eng, ref_len)
    halves = [recs[:2000], recs[2000:]]
    ups = [[d.upload(*ix.concat(h[a:a + 250])) + (len(ix.concat(h[a:a + 250])[0]),) for a in range(0, 2000, 250)] for h in halves]
    counted, errors = [0, 0], []
    gate = threading.Barrier(2)

    def work(k, eng):
        try:
            gate.wait()
            for raw, offs, nb in ups[k]:
                counted[k] += int(obj.add(eng, raw.data_ptr(), nb, offs.numel() - 1, offs.data_ptr()).n_counted)
        except BaseException as e:  # noqa: BLE001
            errors.append(repr(e))

    ts = [threading.Thread(target=work, args=(k, e)) for k, e in enumerate((d.eng, eng2))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors and sum(counted) == n_counted
    assert np.array_equal(obj.array(eng2), dx.differences(dep, ref_len))
    obj.finish(eng2)
    assert np.array_equal(obj.array(d.eng), dx.array(dep, ref_len))
    obj.close()
    eng2.close()
    d.close()


@pytest.fixture(scope="module")
def small_bam(tmp_path_factory):
    from portello_amd import bamsynth, synth

    d = tmp_path_factory.mktemp("depthdev")
    w = synth.generate(synth.config("tiny", n_reads=300, seed=411, split_read_frac=0.3, sorted_reads=True))
    path = str(d / "reads.bam")
    meta = bamsynth.write_read_bam(w, path, level=6, n_unmapped=4)
    return w, path, meta


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [dict(), dict(sorted_runs=True, emit_eqx=True)], ids=["plain", "sorted_runs+eqx"])
def test_bam_to_bam_depth_out(small_bam, tmp_path, extra):
    """15. run_bam_to_bam(depth_out=...): both files are the restatement's over the records read back from the written BAM, and the BAM is
    byte for byte the one of a run without depth_out"""
    import bamcheck
    from portello_amd import bamsynth, pipeline

    w, path, meta = small_bam
    ixd = w.index_data()
    index = api.Index(ixd, 0)
    cn, rn = meta["contig_names"], bamsynth.ref_names(w)
    lens = [len(s) for s in ixd.chrom_seq]
    # one file takes the windows in the order the workers finish them, so the plain mode has fixed bytes with one worker only; a sorted
    # window is a file of its own, whichever of the two workers lifted it, and both add to the one depth object
    kw = dict(window_reads=90, ramp=False, n_workers=2 if extra else 1, io_threads=4, device_records=True, device_batch=True, **extra)
    (tmp_path / "off").mkdir()
    (tmp_path / "on").mkdir()
    st0 = pipeline.run_bam_to_bam(path, str(tmp_path / "off" / "lifted.bam"), index, ixd, cn, rn, lens, **kw)
    st = pipeline.run_bam_to_bam(path, str(tmp_path / "on" / "lifted.bam"), index, ixd, cn, rn, lens, depth_out=str(tmp_path / "on" / "cov"), depth_window=500,
                                 depth_deletions=bool(extra), **kw)
    assert st0.depth_paths == [] and st0.depth_device_ms == 0 and sorted(os.listdir(str(tmp_path / "off"))) == sorted(map(os.path.basename, st0.out_paths))
    assert st.depth_paths == [str(tmp_path / "on" / "cov.per-base.bed"), str(tmp_path / "on" / "cov.regions.bed")] and st.depth_device_ms > 0 and st.lift_detail_s.get("depth", 0) > 0
    assert [os.path.basename(p) for p in st.out_paths] == [os.path.basename(p) for p in st0.out_paths] and st.records_out == st0.records_out
    recs = []
    for p0, p in zip(st0.out_paths, st.out_paths):
        assert open(p, "rb").read() == open(p0, "rb").read()
        recs += bamcheck.read_bam(p)[2]
    assert len(recs) == st.records_out > 300 and dx.first_offender(*ix.concat(recs), lens) is None
    dep, n_counted = dx.depths(recs, lens, deletions=bool(extra))
    assert n_counted > 250 and sum(int(x.sum()) for x in dep) > 0
    assert open(st.depth_paths[0]).read() == dx.per_base_text(rn, dx.runs(dep))
    first, sums = dx.windows(dep, 500)
    assert open(st.depth_paths[1]).read() == dx.regions_text(rn, lens, 500, first, sums)
    if extra:
        assert any((o & 15) in (7, 8) for r in recs[:50] for o in (dx.real_cigar(r) or []))  # the = / X CIGARs were what was added
    index.close()
