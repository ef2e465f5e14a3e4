"""The BAM index of sorted output: plo_records_index_dev (portello_amd/csrc/index_core.hpp), the writer's index (plo_bam_writer_index_enable /
_index_add), plo_bam_merge_runs_indexed and run_bam_to_bam(sorted_runs=True, index_runs=True).

The yardstick is tests/index_expect.py: the entry of a record, the lowest record the device refuses, the .bai bytes from entries and a
block table, and a region query through a parsed index -- plain Python from the definitions in the headers and SAMv1 5.2, not derived from
the code under test.  All comparisons are of integers and bytes.  The CPU tests run index_core.hpp under the wave emulator
(tests/emu/emu_index.cpp) with shuffled lane orders and several wave counts, and once more in a program built with AddressSanitizer + UBSan
where every array sits in a heap block of its exact size; the host side needs no GPU either.  The GPU tests run the C ABI on the device and
the pipeline mode."""
import os
import random
import struct

import numpy as np
import pytest

import bamcheck
import emu_index_lib as eil
import index_expect as ix
import test_records_dev as trd
from portello_amd import abi, api, bam, bamsynth

N_RECORDS = [0, 1, 63, 64, 65, 1025]
N_CIGAR = [0, 1, 63, 64, 65, 129, 4097]
NO_RECORD = 0xFFFFFFFF


def rand_cigar(rng, n_ops, max_len=40):
    return [ix.op(rng.randrange(1, max_len), rng.choice([0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 11])) for _ in range(n_ops)]


def sorted_records(n, n_ref, seed, span=150_000, max_ops=9, pad=24):
    """n records in (reference, pos) order with an unplaced tail, pos -1 and equal positions among them, the strand bit at random"""
    rng = random.Random(seed)
    keys = sorted((rng.choice([0, n_ref - 1, rng.randrange(n_ref), n_ref]), rng.choice([-1, rng.randrange(span), rng.randrange(span) // 5000 * 5000])) for _ in range(n))
    recs = []
    for i, (r, p) in enumerate(keys):
        flag = rng.choice([0, 16, 0, 4, 1 | 16]) if r < n_ref else 4
        recs.append(ix.make_record(-1 if r == n_ref else r, p, flag, b"q%d" % i, rand_cigar(rng, rng.randrange(max_ops)), bytes(rng.randrange(256) for _ in range(rng.randrange(pad)))))
    return recs


def long_cigar_record(ref, pos, n_real=65536, seed=3):
    """a record of n_real > 65 535 ops as BAM stores it: the CIGAR <l_seq>S<ref_len>N and the real ops in CG:B,I"""
    rng = random.Random(seed)
    real = [ix.op(rng.randrange(1, 4), rng.choice([0, 1, 2, 7, 8])) for _ in range(n_real)]
    l_seq = sum(o >> 4 for o in real if (o & 15) in (0, 1, 4, 7, 8))
    ref_len = sum(o >> 4 for o in real if (o & 15) in ix.REF_OPS)
    rec = ix.make_record(ref, pos, 0, b"long", [ix.op(l_seq, 4), ix.op(ref_len, 3)], b"CGBI" + struct.pack("<I", n_real) + struct.pack("<%dI" % n_real, *real))
    assert ix.interval(rec)[1:3] == (pos, pos + ref_len)
    return rec


def shapes():
    """name -> (records, n_ref)"""
    rec, op, rng = ix.make_record, ix.op, random.Random(11)
    s = {}
    s["cigar lengths"] = ([rec(0, 10 * k, 0, b"c%d" % k, rand_cigar(rng, nc)) for k, nc in enumerate(N_CIGAR)], 1)
    s["cigar lengths, odd name lengths"] = ([rec(0, 10 * k, 16, b"n" * (k + 1), rand_cigar(rng, nc), bytes(k)) for k, nc in enumerate(N_CIGAR)], 1)
    s["every op code"] = ([rec(0, 5, 0, b"ops", [op(3 + c, c) for c in range(9)] + [op(1000, 12), op(7, 15)])], 1)
    s["flag 4 with a cigar"] = ([rec(0, 100, 4, b"u", [op(50, 0)]), rec(0, 100, 0, b"m", [op(50, 0)])], 1)
    s["an unplaced tail"] = ([rec(0, 7, 0, b"a", [op(5, 0)]), rec(-1, -1, 4, b"t0"), rec(-1, -1, 4 | 1, b"t1", [op(9, 0)]), rec(-1, 5, 4, b"t2")], 1)
    s["pos -1 on a reference"] = ([rec(0, -1, 0, b"minus", [op(10, 0)]), rec(0, -1, 4, b"minus unmapped"), rec(0, 0, 0, b"zero", [op(10, 0)])], 1)
    s["three references"] = ([rec(0, 9, 0, b"a", [op(4, 0)]), rec(2, 3, 16, b"b", [op(4, 7), op(2, 1), op(4, 8)]), rec(-1, -1, 4, b"c")], 3)
    s["only soft clips"] = ([rec(0, 40, 0, b"s", [op(30, 4), op(5, 5)])], 1)
    s["window edges"] = ([rec(0, 16383, 0, b"in", [op(1, 0)]), rec(0, 16383, 0, b"over", [op(2, 0)]), rec(0, (1 << 26) - 5, 0, b"level 1 edge", [op(10, 0)])], 1)
    s["end exactly 2^29"] = ([rec(0, (1 << 29) - 10, 0, b"top", [op(10, 0)]), rec(0, (1 << 29) - 1, 16, b"last base", [op(1, 2)])], 1)
    s["equal pos, reverse in front of forward"] = ([rec(0, 50, 16, b"r", [op(5, 0)]), rec(0, 50, 0, b"f", [op(6, 0)])], 1)
    s["a 65 536-op record"] = ([rec(0, 3, 0, b"short", [op(5, 0)]), long_cigar_record(0, 100), rec(0, 200, 0, b"after", [op(5, 0)])], 1)
    assert [ix.entry_of(r, 0)[2:4] for r in s["window edges"][0]] == [(16383, 16384), (16383, 16385), ((1 << 26) - 5, (1 << 26) + 5)]
    assert [ix.entry_of(r, 0)[4] >> 16 for r in s["window edges"][0]] == [4681, 585, 0]
    assert ix.entry_of(s["end exactly 2^29"][0][0], 0)[3] == 1 << 29
    return s


def refusals(n_ref=3):
    """name -> (data, off, lowest offender, kind): inside a buffer of otherwise good records, behind the first wave's worth of them"""
    good = sorted_records(130, n_ref, 77)
    placed = [i for i, r in enumerate(good) if ix.fields(r)[0] >= 0]
    at = 70
    assert at + 5 < len(placed) and ix.fields(good[at])[0] == ix.fields(good[at + 1])[0]
    rec, op = ix.make_record, ix.op
    ref_at, pos_at = ix.fields(good[at])[:2]

    def with_record(r, where=at):
        recs = list(good)
        recs[where] = r
        return ix.concat(recs)

    out = {}
    data, off = ix.concat(good)
    o = off.copy()
    o[at + 1] = o[at] - 1
    out["record_off decreases"] = (data, o, at, ix.ERR_OFFSET)
    o = off.copy()
    o[-1] -= 1
    out["record_off[n] != n_bytes"] = (data, o, len(good) - 1, ix.ERR_OFFSET)
    o = off.copy()
    o[0] = 1
    out["record_off[0] != 0"] = (data, o, 0, ix.ERR_OFFSET)
    out["shorter than 36 bytes"] = with_record(rec(ref_at, pos_at)[:35]) + (at, ix.ERR_SHORT)
    out["block_size disagrees"] = with_record(rec(ref_at, pos_at, 0, b"name", block_size=37)) + (at, ix.ERR_BLOCK)
    out["refID == n_ref"] = with_record(rec(n_ref, pos_at)) + (at, ix.ERR_REFID)
    out["pos == -2"] = with_record(rec(ref_at, -2)) + (at, ix.ERR_POS)
    out["the CIGAR one op past the record"] = with_record(rec(ref_at, pos_at, 0, b"cut", [op(5, 0)] * 70, n_cigar=71)) + (at, ix.ERR_CIGAR)
    out["the CIGAR one op past the LAST record"] = with_record(rec(-1, -1, 4, b"cut", [op(5, 0)] * 3, n_cigar=4), len(good) - 1) + (len(good) - 1, ix.ERR_CIGAR)
    out["end == 2^29 + 1"] = with_record(rec(ref_at, (1 << 29) - 10, 0, b"far", [op(5, 0), op(6, 2)])) + (at, ix.ERR_END)
    k = next(i for i in range(64, len(placed) - 1) if ix.fields(good[i])[0] == ix.fields(good[i + 1])[0] and ix.fields(good[i])[1] < ix.fields(good[i + 1])[1])
    recs = list(good)
    recs[k], recs[k + 1] = recs[k + 1], recs[k]
    out["pos decreases"] = ix.concat(recs) + (k + 1, ix.ERR_ORDER)
    k = next(i for i in range(len(placed) - 1) if ix.fields(good[i])[0] < ix.fields(good[i + 1])[0])
    recs = list(good)
    recs[k], recs[k + 1] = recs[k + 1], recs[k]
    out["the reference decreases"] = ix.concat(recs) + (k + 1, ix.ERR_ORDER)
    assert len(placed) < len(good)
    recs = list(good)
    recs[len(placed) - 1], recs[len(placed)] = recs[len(placed)], recs[len(placed) - 1]
    out["a placed record behind an unplaced one"] = ix.concat(recs) + (len(placed), ix.ERR_ORDER)
    recs = list(good)
    recs[at], recs[20] = rec(ref_at, -2), rec(ix.fields(good[20])[0], ix.fields(good[20])[1], 0, b"x", [op(1, 0)], n_cigar=9)
    out["two offenders"] = ix.concat(recs) + (20, ix.ERR_CIGAR)
    return out


def emu_check(recs, n_ref, what=""):
    data, off = ix.concat(recs)
    assert ix.first_offender(data, off, n_ref) is None, what
    want = ix.entries(data, off)
    for seed, n_waves in ((0, 1), (1, 3), (2, 8)):
        st, ent, n_placed, er, ek = eil.index(data, off, n_ref, order_seed=seed, n_waves=n_waves)
        assert (st, er, ek) == (abi.PLO_OK, NO_RECORD, 0), (what, seed, st)  # -4: the wave and the one-thread rule disagree
        assert np.array_equal(ent, want), (what, seed)
        assert n_placed == int((want["ref_id"] >= 0).sum()), what
    return want


# ---- CPU: the yardstick, and index_core.hpp under the wave emulator -------------------------------------------------------------------------

def test_expectation_by_hand():
    """the yardstick itself on an example small enough to verify by eye: two references, four records of 50 bytes in two blocks of 100
    stream bytes at file offsets 1000 and 1070, the EOF block at 1200"""
    rec, op = ix.make_record, ix.op
    recs = [rec(0, 100, 0, b"a" * 10, [op(50, 0)]),          # [100, 150)      bin 4681, window 0
            rec(0, 16380, 0, b"b" * 10, [op(10, 0)]),        # [16380, 16390)  bin 585: it crosses 16384; windows 0 and 1
            rec(0, 50000, 4, b"c" * 10, [op(10, 0)]),        # FLAG 4: [50000, 50001)  bin 4684, window 3
            rec(-1, -1, 4, b"d" * 14)]                       # unplaced
    assert [len(r) for r in recs] == [50] * 4
    data, off = ix.concat(recs)
    ents = ix.entries(data, off)
    assert ents.tolist() == [(0, 0, 100, 150, 4681 << 16), (50, 0, 16380, 16390, 585 << 16), (100, 0, 50000, 50001, 1 | (4684 << 16)), (150, -1, -1, 0, 1 | (4680 << 16))]
    v = lambda fo, uo: (fo << 16) | uo
    got = ix.bai_bytes(ents, 200, [(0, 1000), (100, 1070)], 1200, 2)
    want = b"BAI\x01" + struct.pack("<I", 2)
    want += struct.pack("<I", 4)                                              # reference 0: three bins and the pseudo-bin
    want += struct.pack("<IIQQ", 585, 1, v(1000, 50), v(1070, 0))             # the record at stream 50 ends where the second block begins
    want += struct.pack("<IIQQ", 4681, 1, v(1000, 0), v(1000, 50))
    want += struct.pack("<IIQQ", 4684, 1, v(1070, 0), v(1070, 50))
    want += struct.pack("<IIQQQQ", 37450, 2, v(1000, 0), v(1070, 50), 2, 1)   # first record .. behind the last; 2 mapped, 1 with FLAG 4
    want += struct.pack("<I4Q", 4, v(1000, 0), v(1000, 50), v(1070, 0), v(1070, 0))  # window 2 is unset: it takes window 3's value
    want += struct.pack("<II", 0, 0)                                          # reference 1 has no record
    want += struct.pack("<Q", 1)
    assert got == want
    refs, n_no_coor = ix.parse_bai(got)
    assert n_no_coor == 1 and sorted(refs[0]["bins"]) == [585, 4681, 4684] and refs[0]["meta"][1] == (2, 1) and refs[1] == {"bins": {}, "meta": None, "linear": []}
    assert ix.reg2bin(0, 1 << 29) == 0 and ix.reg2bin((1 << 29) - 1, 1 << 29) == 4681 + 32767 and 585 in ix.reg2bins(16384, 16385) and len(ix.reg2bins(0, 1 << 29)) == 37449
    assert ix.first_offender(data, off, 2) is None and ix.first_offender(data, off, 1) is None
    assert ix.first_offender(*ix.concat(recs[::-1]), 2) == (1, ix.ERR_ORDER)


@pytest.mark.parametrize("n", N_RECORDS)
def test_sizes(n):
    """1. the record counts around the wave and past a thousand; three references"""
    emu_check(sorted_records(n, 3, 100 + n), 3, n)


@pytest.mark.parametrize("name", sorted(shapes()))
def test_shapes(name):
    """2. the CIGAR lengths around the wave's width and the record shapes"""
    recs, n_ref = shapes()[name]
    want = emu_check(recs, n_ref, name)
    if name == "flag 4 with a cigar":
        assert want["end"].tolist() == [101, 150] and want["flags"].tolist() == [1 | (4681 << 16), 4681 << 16]
    if name == "pos -1 on a reference":
        assert want["beg"].tolist() == [0, 0, 0] and want["end"].tolist() == [10, 1, 10]
    if name == "every op code":
        assert int(want["end"][0]) == 5 + (3 + 0) + (3 + 2) + (3 + 3) + (3 + 7) + (3 + 8)


@pytest.mark.parametrize("name", sorted(refusals()))
def test_refusal(name):
    """3. every check refuses and names the LOWEST offending record and what it broke; no entry is handed out"""
    data, off, rec, kind = refusals()[name]
    assert ix.first_offender(data, off, 3) == (rec, kind)
    for seed, n_waves in ((0, 1), (1, 4), (2, 7)):
        st, ent, n_placed, er, ek = eil.index(data, off, 3, order_seed=seed, n_waves=n_waves)
        assert (st, ent, er, ek) == (abi.PLO_ERR_INVALID_ARG, None, rec, kind), name


def test_asan_program(tmp_path):
    """4. the same harness as a stand-alone program with ASan + UBSan, every array in a heap block of its exact size: sizes, shapes,
    refusals"""
    cases, wants = [], []
    for n in N_RECORDS:
        data, off = ix.concat(sorted_records(n, 3, 300 + n))
        cases.append((data, off, 3, n % 3, 1 + n % 5))
        wants.append(ix.entries(data, off))
    for name, (recs, n_ref) in sorted(shapes().items()):
        data, off = ix.concat(recs)
        cases.append((data, off, n_ref, 1, 2))
        wants.append(ix.entries(data, off))
    for name, (data, off, rec, kind) in sorted(refusals().items()):
        cases.append((data, off, 3, 0, 3))
        wants.append((rec, kind))
    rc, err, res = eil.run_asan(cases, str(tmp_path))
    assert rc == 0, err[-3000:]
    assert "ERROR" not in err and "runtime error" not in err, err[-3000:]
    for (st, ent, n_placed, er, ek), want in zip(res, wants):
        if isinstance(want, tuple):
            assert (st, er, ek) == (abi.PLO_ERR_INVALID_ARG,) + want
        else:
            assert st == abi.PLO_OK and np.array_equal(ent, want) and n_placed == int((want["ref_id"] >= 0).sum())


# ---- CPU: the host side ---------------------------------------------------------------------------------------------------------------------

REFS, LENS = ["chr1", "chr2", "chrM"], [1 << 29, 200_000, 5000]
HDR = None


def header():
    return bam.output_header(REFS, LENS, sort_order="coordinate")


def run_records(n, seed, pad=400):
    """a sorted run of n records over some ten linear windows of three references, a few long spans among them"""
    recs = sorted_records(n, len(REFS), seed, pad=pad)
    rng = random.Random(seed)
    spans = [ix.make_record(0, p, 0, b"span%d" % k, [ix.op(rng.randrange(20_000, 140_000), 0)]) for k, p in enumerate(sorted(rng.randrange(100_000) for _ in range(4)))]
    recs = sorted(recs + spans, key=lambda r: (len(REFS) if ix.fields(r)[0] < 0 else ix.fields(r)[0], ix.fields(r)[1]))
    assert ix.first_offender(*ix.concat(recs), len(REFS)) is None
    return recs


def write_indexed(path, pieces, level):
    """the records of `pieces` (lists of records), an index_add and a write per piece"""
    wr = bam.BamWriter(path, header(), REFS, LENS, level=level, index_path=path + ".bai")
    for piece in pieces:
        data, off = ix.concat(piece)
        wr.index_add(ix.entries(data, off))
        wr.write(data)
    wr.close()
    return open(path, "rb").read(), open(path + ".bai", "rb").read()


def regions(rng, n):
    out = []
    for _ in range(n):
        ref = rng.randrange(len(REFS))
        top = min(LENS[ref], 170_000)
        a = rng.randrange(top)
        out.append((ref, a, min(LENS[ref], a + rng.choice([1, 2, 100, 16384, 40_000, top]))))
    out += [(r, 0, LENS[r]) for r in range(len(REFS))]                      # whole references
    out += [(0, 5, 5), (1, 100, 50), (0, 1 << 28, (1 << 28) + 10), (2, 4999, 5000)]  # empty regions, and one far from every record
    return out


def check_queries(blob, bai_blob, n=300, seed=5):
    recs = ix.bam_layout(blob)[0]
    bai = ix.parse_bai(bai_blob)
    hits = 0
    for ref, a, b in regions(random.Random(seed), n):
        got, want = ix.query(blob, bai, ref, a, b), ix.brute(recs, ref, a, b)
        assert got == want, (ref, a, b, len(got), len(want))
        hits += bool(want)
    assert hits > n // 3  # the regions are no empty test


@pytest.mark.parametrize("level", [0, 1])
def test_writer_index(tmp_path, level):
    """5. a run written in one piece: the .bai is the restatement's over the file's own bytes, and every region query through it returns the
    brute-force overlap set"""
    recs = run_records(700, 21)
    blob, bai_blob = write_indexed(str(tmp_path / "run.bam"), [recs], level)
    assert bamcheck.read_bam(str(tmp_path / "run.bam"))[2] == recs and len(ix.bam_layout(blob)[1]) >= 3
    assert bai_blob == ix.expected_bai(blob)
    check_queries(blob, bai_blob)
    # the BAM is the one the writer makes without an index
    wr = bam.BamWriter(str(tmp_path / "plain.bam"), header(), REFS, LENS, level=level)
    wr.write(b"".join(recs))
    wr.close()
    assert open(str(tmp_path / "plain.bam"), "rb").read() == blob


@pytest.mark.parametrize("level", [0, 1])
def test_writer_index_in_pieces(tmp_path, level):
    """6. several writes that end inside a block, and a record that starts exactly on a block boundary"""
    recs = run_records(700, 22)
    k = next(i for i in range(len(recs)) if sum(map(len, recs[:i + 1])) > 0xff00 - 36)  # stretch record k - 1 so that record k starts at 0xff00
    fill = 0xff00 - sum(map(len, recs[:k]))
    r = recs[k - 1]
    ref, pos, lrn, ncig, flag = ix.fields(r)
    recs[k - 1] = ix.make_record(ref, pos, flag, r[36:36 + lrn], struct.unpack_from("<%dI" % ncig, r, 36 + lrn), r[36 + lrn + 4 * ncig:] + bytes(fill))
    assert sum(map(len, recs[:k])) == 0xff00
    pieces = [recs[:100], recs[100:101], [], recs[101:450], recs[450:]]
    blob, bai_blob = write_indexed(str(tmp_path / "pieces.bam"), pieces, level)
    whole, whole_bai = write_indexed(str(tmp_path / "whole.bam"), [recs], level)
    assert blob == whole and bai_blob == whole_bai == ix.expected_bai(blob)
    table = ix.bam_layout(blob)[1]
    assert table[1][0] == 0xff00
    f = ix.BgzfFile(blob)
    assert f.records(table[1][1] << 16, (table[1][1] << 16) + 1)[0][1] == recs[k]  # the record at the boundary is found at the new block's start
    check_queries(blob, bai_blob, n=120, seed=6)


def test_writer_index_of_no_record(tmp_path):
    p = str(tmp_path / "empty.bam")
    blob, bai_blob = write_indexed(p, [], 0)
    assert bai_blob == ix.expected_bai(blob) == b"BAI\x01" + struct.pack("<I", 3) + struct.pack("<II", 0, 0) * 3 + struct.pack("<Q", 0)


def test_writer_refusals(tmp_path):
    """7. entries that do not tile the bytes: PLO_ERR_INVALID_ARG at the close, no .bai, the BAM complete; an @SQ over 2^29 refuses the index"""
    recs = run_records(60, 23)
    data, off = ix.concat(recs)
    ents = ix.entries(data, off)
    shifted = ents.copy()
    shifted["off"][30] = shifted["off"][29] + 35  # record 29 would be shorter than its fixed fields
    swapped = ents.copy()
    swapped[[10, 11]] = swapped[[11, 10]]
    late = ents.copy()
    late["off"][-1] = len(data) - 10
    for name, adds in (("the first entry is missing", [ents[1:]]), ("an entry inside its neighbour", [shifted]), ("entries out of order", [swapped]),
                       ("the last entry too close to the end", [late]), ("no entries at all", []), ("an empty add", [ents[:0]])):
        p = str(tmp_path / "bad.bam")
        wr = bam.BamWriter(p, header(), REFS, LENS, level=0, index_path=p + ".bai")
        for a in adds:
            wr.index_add(a)
        wr.write(data)
        with pytest.raises(api.PortelloError, match="no index is written") as e:
            wr.close()
        assert e.value.status == abi.PLO_ERR_INVALID_ARG and not os.path.exists(p + ".bai"), name
        assert bamcheck.read_bam(p)[2] == recs, name
    # bytes behind the entries' write, without entries of their own
    p = str(tmp_path / "tail.bam")
    wr = bam.BamWriter(p, header(), REFS, LENS, level=0, index_path=p + ".bai")
    wr.index_add(ents)
    wr.write(data)
    wr.index_add(ents[:0])
    wr.write(recs[-1])
    with pytest.raises(api.PortelloError, match="no index is written"):
        wr.close()
    assert not os.path.exists(p + ".bai")
    with pytest.raises(api.PortelloError, match="2\\^29") as e:
        bam.BamWriter(str(tmp_path / "long.bam"), bam.output_header(["big"], [(1 << 29) + 1]), ["big"], [(1 << 29) + 1], index_path=str(tmp_path / "long.bam.bai"))
    assert e.value.status == abi.PLO_ERR_INVALID_ARG and not os.path.exists(str(tmp_path / "long.bam.bai"))
    assert "@SQ 0" in str(e.value) and not os.path.exists(str(tmp_path / "long.bam"))  # the constructor raised: no header-only file stays
    # the index comes before the first record byte
    wr = bam.BamWriter(str(tmp_path / "late.bam"), header(), REFS, LENS)
    wr.write(recs[0])
    assert bam.lib().plo_bam_writer_index_enable(wr.handle, str(tmp_path / "late.bam.bai").encode()) == abi.PLO_ERR_INVALID_ARG
    wr.close()


def merge_run(n, seed):
    """run_records in the order plo_bam_merge_runs asks of a run: plo_records_sort_dev's key, forward in front of reverse at one position"""
    return sorted(run_records(n, seed), key=lambda r: (len(REFS) if ix.fields(r)[0] < 0 else ix.fields(r)[0], ix.fields(r)[1], (ix.fields(r)[4] >> 4) & 1))


def write_run(path, recs, level=0):
    wr = bam.BamWriter(path, header(), REFS, LENS, level=level)
    if recs:
        wr.write(b"".join(recs))
    wr.close()
    return path


@pytest.mark.parametrize("level", [0, 1])
def test_merge_runs_indexed(tmp_path, level):
    """8. three runs with ties across them: the merged file is byte for byte the one of index=False, its .bai the restatement's over it, and
    the queries hold"""
    runs = [merge_run(400, 31), merge_run(7, 32), merge_run(250, 33)]
    keys = [set(ix.fields(r)[:2] for r in run) for run in runs]
    assert keys[0] & keys[2] and keys[0] & keys[1]
    paths = [write_run(str(tmp_path / f"run{k}.bam"), run) for k, run in enumerate(runs)]
    plain, out = str(tmp_path / "plain.bam"), str(tmp_path / "merged.bam")
    bam.merge_runs(paths, plain, level=level)
    bam.merge_runs(paths, out, level=level, index=True)
    blob = open(out, "rb").read()
    assert blob == open(plain, "rb").read() and not os.path.exists(plain + ".bai")
    assert sorted(bamcheck.read_bam(out)[2]) == sorted(r for run in runs for r in run)
    bai_blob = open(out + ".bai", "rb").read()
    assert bai_blob == ix.expected_bai(blob)
    check_queries(blob, bai_blob, n=200, seed=7)


def test_merge_indexed_failures_leave_no_file(tmp_path):
    """9. a run out of order, and a record the index rule refuses (which the plain merge passes): neither the BAM nor the .bai stays"""
    good = write_run(str(tmp_path / "good.bam"), merge_run(30, 41))
    run = merge_run(50, 42)
    k = next(i for i in range(49) if ix.fields(run[i])[:2] < ix.fields(run[i + 1])[:2] and ix.fields(run[i + 1])[0] >= 0)
    run[k], run[k + 1] = run[k + 1], run[k]
    swapped = write_run(str(tmp_path / "swapped.bam"), run)
    cut = write_run(str(tmp_path / "cut.bam"), [ix.make_record(0, 5, 0, b"ok", [ix.op(5, 0)]), ix.make_record(0, 6, 0, b"cut", [ix.op(5, 0)] * 2, n_cigar=3)])
    far = write_run(str(tmp_path / "far.bam"), [ix.make_record(0, (1 << 29) - 3, 0, b"far", [ix.op(4, 0)])])
    out = str(tmp_path / "out.bam")
    for bad, what, status in ((swapped, r"swapped\.bam: record %d " % (k + 1), bam.ERR_DATA), (cut, r"cut\.bam: record 1 cannot be indexed", bam.ERR_DATA),
                              (far, r"far\.bam: record 0 cannot be indexed", bam.ERR_DATA)):
        with pytest.raises(api.PortelloError, match=what) as e:
            bam.merge_runs([good, bad], out, index=True)
        assert e.value.status == status and not os.path.exists(out) and not os.path.exists(out + ".bai"), bad
    bam.merge_runs([good, cut], out)  # without an index the merge does not look at a CIGAR
    assert os.path.exists(out) and not os.path.exists(out + ".bai")


def test_index_runs_needs_sorted_runs(tmp_path):
    from portello_amd import pipeline

    with pytest.raises(ValueError, match="sorted_runs"):
        pipeline.run_bam_to_bam("in.bam", str(tmp_path / "x.bam"), None, None, [], [], [], device_records=True, index_runs=True)


def test_abi_structs():
    import ctypes as C

    assert C.sizeof(abi.PloIndexEntry) == 24 == abi.INDEX_ENTRY_DTYPE.itemsize and abi.PLO_API_VERSION >= 15
    assert [(n, abi.INDEX_ENTRY_DTYPE.fields[n][1]) for n in abi.INDEX_ENTRY_DTYPE.names] == [(f[0], getattr(abi.PloIndexEntry, f[0]).offset) for f in abi.PloIndexEntry._fields_]
    assert abi.INDEX_ENTRY_DTYPE == ix.ENTRY


def test_context_destroys_every_event_once():
    """every array of HIP events on the context is destroyed by exactly one loop of plo_ctx_destroy, over its whole length: none leaks,
    none is handed to hipEventDestroy twice"""
    import re

    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "portello_amd", "csrc", "engine.hip")).read()
    at = src.index("void plo_ctx_destroy(plo_ctx *c) {")
    members = dict(re.findall(r"^\s*hipEvent_t (\w+)\[(\d+)\] = \{", src[src.index("struct plo_ctx {"):at], re.M))
    assert {"iev", "xev", "sev"} <= set(members)
    body = src[at:]
    body = body[:body.index("\n}\n")]
    loops = re.findall(r"for \(int i = 0; i < (\d+); \+\+i\)\s*if \(c->(\w+)\[i\]\) \(void\)hipEventDestroy\(c->(\w+)\[i\]\);", body)
    assert sorted((name, n) for n, name, _ in loops) == sorted(members.items())
    assert all(a == b for _, a, b in loops) and len(loops) == body.count("[i]);")


def test_entries_share_the_windows_block():
    """the entries of a window stand behind its bytes in the one page-locked block, 8-aligned; an index of another record count is refused"""
    from portello_amd import devbatch

    class Out:
        n_records = 5

    assert devbatch._entries_room(1001, None, 5) == (1001, 1001)
    assert devbatch._entries_room(1001, Out, 5) == (1008, 1008 + 5 * 24)
    with pytest.raises(ValueError, match="5 entries for a window of 6 records"):
        devbatch._entries_room(1001, Out, 6)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------

class DevIndexer:
    """hand-made records through Engine.records_index_dev"""

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

    def run(self, raw, offs, n_bytes, n_ref):
        return self.eng.records_index_dev(raw.data_ptr(), n_bytes, offs.numel() - 1, offs.data_ptr(), n_ref)

    def check(self, recs, n_ref, what=""):
        data, off = ix.concat(recs)
        want = ix.entries(data, off)
        raw, offs = self.upload(data, off)
        io = self.run(raw, offs, len(data), n_ref)
        assert (int(io.n_records), int(io.err_record), int(io.err_kind)) == (len(recs), NO_RECORD, 0), what
        got = self.eng.download(io.entry, np.uint8, 24 * len(recs)).view(ix.ENTRY)
        assert np.array_equal(got, want), what
        assert int(io.n_placed) == int((want["ref_id"] >= 0).sum()), what
        self.torch.cuda.synchronize()
        assert raw[:len(data)].cpu().numpy().tobytes() == data and np.array_equal(offs.cpu().numpy().view(np.uint64), off), what  # the input is unchanged
        return io

    def close(self):
        self.eng.close()
        self.index.close()


@pytest.mark.gpu
def test_device_sizes_and_shapes():
    """10. the sizes and shapes of the CPU tests through the C ABI, entry for entry, one context for all: the buffer grows and is reused"""
    di = DevIndexer()
    for n in N_RECORDS + [5000]:
        io = di.check(sorted_records(n, 3, 100 + n), 3, n)
        assert n == 0 or io.index_ms > 0
    for name, (recs, n_ref) in sorted(shapes().items()):
        di.check(recs, n_ref, name)
    di.close()


@pytest.mark.gpu
def test_device_refusals():
    """11. every refusal returns its status, err_record and err_kind, names the record, and the context indexes the next call"""
    di = DevIndexer()
    good = sorted_records(130, 3, 77)
    for name, (data, off, rec, kind) in sorted(refusals().items()):
        raw, offs = di.upload(data, off)
        with pytest.raises(api.PortelloError, match=r"record %d " % rec) as e:
            di.run(raw, offs, len(data), 3)
        assert (e.value.status, e.value.err_record, e.value.err_kind) == (abi.PLO_ERR_INVALID_ARG, rec, kind), name
        di.check(good, 3, "after " + name)
    raw, offs = di.upload(*ix.concat(good))
    with pytest.raises(api.PortelloError) as e:
        di.eng.records_index_dev(0, 100, 3, offs.data_ptr(), 3)
    assert e.value.status == abi.PLO_ERR_INVALID_ARG
    di.close()


@pytest.fixture(scope="module")
def small_bam(tmp_path_factory):
    from portello_amd import synth

    d = tmp_path_factory.mktemp("indexdev")
    w = synth.generate(synth.config("tiny", n_reads=300, seed=411, split_read_frac=0.3, sorted_reads=True))
    path = str(d / "reads.bam")
    meta = bamsynth.write_read_bam(w, path, level=6, n_unmapped=4)
    return w, path, meta


@pytest.mark.gpu
def test_device_index_of_the_small_bam(small_bam):
    """12. lift -> finish -> records -> sort -> index: the entries of the sorted buffer are the restatement's, and the sorted buffer stays"""
    w, path, meta = small_bam
    index = api.Index(w.index_data(), 0)
    cn, rn = meta["contig_names"], bamsynth.ref_names(w)
    rd, win = trd.open_window(path)
    run = trd.DeviceRun(win, index, cn, rn, False)
    run.finish()
    run.sa()
    ro = run.eng.records_build_dev(run.ddesc, run.up.records_in(run.labels, False))
    n, nb = int(ro.n_records), int(ro.n_bytes)
    so = run.eng.records_sort_dev(ro.bytes, nb, n, ro.record_off, len(rn))
    dl = run.eng.download
    sdata, soff = dl(so.bytes, np.uint8, nb).tobytes(), dl(so.record_off, np.uint64, n + 1)
    assert n > 300 and ix.first_offender(sdata, soff, len(rn)) is None
    io = run.eng.records_index_dev(so.bytes, nb, n, so.record_off, len(rn))
    want = ix.entries(sdata, soff)
    assert np.array_equal(dl(io.entry, np.uint8, 24 * n).view(ix.ENTRY), want)
    assert int(io.n_placed) == int(so.n_mapped) == int((want["ref_id"] >= 0).sum()) and int(io.n_records) == n
    assert (want["end"][want["ref_id"] >= 0] - want["beg"][want["ref_id"] >= 0]).max() > 1
    assert dl(so.bytes, np.uint8, nb).tobytes() == sdata and np.array_equal(dl(so.record_off, np.uint64, n + 1), soff)
    # the unsorted records are refused for their order
    with pytest.raises(api.PortelloError) as e:
        run.eng.records_index_dev(ro.bytes, nb, n, ro.record_off, len(rn))
    assert e.value.err_kind == ix.ERR_ORDER and (e.value.err_record, ix.ERR_ORDER) == ix.first_offender(dl(ro.bytes, np.uint8, nb).tobytes(), dl(ro.record_off, np.uint64, n + 1), len(rn))
    run.eng.close()
    win.close()
    rd.close()
    index.close()


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [dict(), dict(device_bgzf=True, level=1), dict(emit_nm=True, emit_md=True)], ids=["plain", "device_bgzf", "nm_md"])
def test_bam_to_bam_index_runs(small_bam, tmp_path, extra):
    """13. run_bam_to_bam(sorted_runs=True, index_runs=True): every run's .bai is the restatement's over that run's file, the queries hold
    on a run and on the indexed merge; with index_runs off the runs are the same files, byte for byte, and no .bai appears"""
    from portello_amd import pipeline

    w, path, meta = small_bam
    ixd = w.index_data()
    index = api.Index(ixd, 0)
    cn, rn = meta["contig_names"], bamsynth.ref_names(w)
    lens = [len(s) for s in ixd.chrom_seq]
    kw = dict(window_reads=90, ramp=False, n_workers=2, io_threads=4, device_records=True, device_batch=True, sorted_runs=True, **extra)
    (tmp_path / "off").mkdir()
    (tmp_path / "on").mkdir()
    st0 = pipeline.run_bam_to_bam(path, str(tmp_path / "off" / "lifted.bam"), index, ixd, cn, rn, lens, **kw)
    st = pipeline.run_bam_to_bam(path, str(tmp_path / "on" / "lifted.bam"), index, ixd, cn, rn, lens, index_runs=True, **kw)
    assert st0.index_paths == [] and st0.index_device_ms == 0 and "index" not in st0.lift_detail_s and sorted(os.listdir(str(tmp_path / "off"))) == sorted(map(os.path.basename, st0.out_paths))
    assert len(st.out_paths) >= 3 and [os.path.basename(p) for p in st.out_paths] == [os.path.basename(p) for p in st0.out_paths]
    assert st.index_paths == [p + ".bai" for p in st.out_paths] and st.index_device_ms > 0 and st.lift_detail_s.get("index", 0) > 0
    assert st.records_out == st0.records_out and st.out_file_bytes == st0.out_file_bytes
    largest = max(st.out_paths, key=os.path.getsize)
    for p0, p in zip(st0.out_paths, st.out_paths):
        blob = open(p, "rb").read()
        assert blob == open(p0, "rb").read()
        bai_blob = open(p + ".bai", "rb").read()
        assert bai_blob == ix.expected_bai(blob), p
        if p == largest:
            check_bam_queries(blob, bai_blob, lens)
    merged = str(tmp_path / "merged.bam")
    bam.merge_runs(st.out_paths, merged, index=True)
    blob, bai_blob = open(merged, "rb").read(), open(merged + ".bai", "rb").read()
    assert bai_blob == ix.expected_bai(blob) and len(ix.bam_layout(blob)[0]) == st.records_out
    check_bam_queries(blob, bai_blob, lens)
    index.close()


def check_bam_queries(blob, bai_blob, lens, n=60, seed=9):
    recs, bai, rng = ix.bam_layout(blob)[0], ix.parse_bai(bai_blob), random.Random(seed)
    regs = [(r, 0, lens[r]) for r in range(len(lens))] + [(0, 7, 7)]
    for _ in range(n):
        r = rng.randrange(len(lens))
        a = rng.randrange(lens[r])
        regs.append((r, a, min(lens[r], a + rng.choice([1, 50, 2000, 20_000]))))
    hits = 0
    for r, a, b in regs:
        got, want = ix.query(blob, bai, r, a, b), ix.brute(recs, r, a, b)
        assert got == want, (r, a, b, len(got), len(want))
        hits += bool(want)
    assert hits > 5
