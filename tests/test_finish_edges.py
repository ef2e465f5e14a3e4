"""Finishing and SA text on hand-built edge cases (finish_core.hpp): three voices on every case -- the plain reference tests/finish_expect.py
(written from the Rust text), the C oracle, and the device code: under the emulator (CPU), as a stand-alone AddressSanitizer + UBSan program
over heap blocks of exact size (CPU), and on the device (gpu).  The cases are tests/finish_cases.py's."""
import json
import os
import time

import numpy as np
import pytest

import emu_finish_lib as efl
import emu_lib
import finish_cases as fc
import finish_expect as fx
from portello_amd import abi, api
from portello_amd import cigar as cg

BAM4, ASCII = abi.SEQ_BAM4, abi.SEQ_ASCII
FMTS = [BAM4, ASCII]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "finish_vectors.json")


def check_case(case, oracle, threads=(7,), names=None, want=None):
    """reference vs oracle vs emulated device code, byte for byte -> the reference's result"""
    exp = fx.finish(*case.fin()) if want is None else want
    fx.compare(oracle.finish_batch(*case.fin()), exp, "oracle " + case.name)
    for t in threads:
        fx.compare(emu_lib.finish_batch(*case.fin(), nthreads=t), exp, "emulator %s, %d threads" % (case.name, t))
    if names is not None:
        want_sa = fx.sa_values(case.batch, case.lift, exp["item_flag"], names)
        assert oracle.sa_values(case.batch, case.lift, exp["item_flag"], names) == want_sa, case.name
        off, text, item_read = emu_lib.sa_segments(case.batch, case.lift, exp["item_flag"], exp["read_n_lifted"], names)
        assert api.assemble_sa_values(off, text, item_read) == want_sa, case.name
    return exp


# ---- 1. the reference itself -------------------------------------------------------------------------------------------------------------

def test_reference_reproduces_the_hand_worked_vectors():
    g = json.load(open(GOLDEN))
    for v in g["reg2bin"]:
        assert fx.reg2bin(v["beg"], v["end"]) == v["bin"], v
    for v in g["ref_end"]:
        assert fx.ref_end(v["pos"], cg.encode(v["cigar"]) if v["cigar"] else []) == v["end"], v
    for v in g["item_flag"]:
        assert fx.item_flag(v["read_flag"], v["flipped"], v["primary"]) == v["flag"], v
    for v in g["unmapped_flag"]:
        assert fx.unmapped_flag(v["read_flag"]) == (v["flag"], v["reversed"]), v
    for v in g["revcomp_bam4"]:
        assert fx.revcomp_bam4(np.array(v["packed"], np.uint8), v["len"]).tolist() == v["out"], v
    for v in g["revcomp_ascii"]:
        assert fx.revcomp_ascii(np.frombuffer(v["in"].encode(), np.uint8), len(v["in"])).tobytes() == v["out"].encode(), v
    lay = g["layout"]
    case = fc.build([(L, f, None, None) for L, f in zip(lay["read_len"], lay["read_flag"])],
                    [(r, fc.L_, flip, 30, 0, 10, [fc.M(lay["read_len"][r])]) for r, flip in lay["items"]], lay["seq_fmt"])
    res = fx.finish(*case.fin())
    fix = lambda xs: [abi.NO_FLIP if x < 0 else x for x in xs]
    for name in ("item_seq_off", "item_qual_off", "read_seq_off", "read_qual_off"):
        assert res[name].tolist() == fix(lay[name]), name
    assert (res["rev_seq_bytes"], res["rev_qual_bytes"]) == (lay["rev_seq_bytes"], lay["rev_qual_bytes"])
    sa = g["sa"]
    case = fc.build([(10, sa["read_flag"], None, None)],
                    [(0, fc.L_, it["flip"], it["mapq"], it["chrom"], it["pos"], cg.encode(it["cigar"]) if it["cigar"] else []) for it in sa["items"]])
    res = fx.finish(*case.fin())
    assert fx.sa_values(case.batch, case.lift, res["item_flag"], sa["chroms"]) == [v.encode() for v in sa["values"]]


def test_golden_vectors_on_oracle_and_emulator(oracle):
    """the same hand-worked values through the two other voices"""
    g = json.load(open(GOLDEN))
    span = lambda n: [fc.M(fc.BIG)] * (n // fc.BIG) + [fc.M(n % fc.BIG)]  # (an op holds 28 bits)
    items = [(0, fc.L_, 0, 30, 0, v["beg"], span(v["end"] - v["beg"])) for v in g["reg2bin"]]
    items += [(0, fc.L_, 0, 30, 0, v["pos"], cg.encode(v["cigar"]) if v["cigar"] else []) for v in g["ref_end"]]
    case = fc.build([(10, 0, None, None)], items)
    for res in (oracle.finish_batch(*case.fin()), emu_lib.finish_batch(*case.fin())):
        assert res["item_bin"][:len(g["reg2bin"])].tolist() == [v["bin"] for v in g["reg2bin"]]
        assert res["item_ref_end"].tolist() == [v["end"] for v in g["reg2bin"]] + [v["end"] for v in g["ref_end"]]
    for v in g["revcomp_bam4"]:
        codes = np.array([[b >> 4, b & 15] for b in v["packed"]], np.uint8).reshape(-1)[:v["len"]]
        case = fc.build([(v["len"], 0x10, codes, None)], [])
        for res in (oracle.finish_batch(*case.fin()), emu_lib.finish_batch(*case.fin())):
            got = res["rev_seq"][:len(v["out"])].copy()
            if v["len"] & 1:
                got[-1] &= 0xF0
            assert got.tolist() == v["out"], v
    for v in g["revcomp_ascii"]:
        case = fc.build([(len(v["in"]), 0x10, np.frombuffer(v["in"].encode(), np.uint8), None)], [], ASCII)
        for res in (oracle.finish_batch(*case.fin()), emu_lib.finish_batch(*case.fin())):
            assert res["rev_seq"][:len(v["in"])].tobytes() == v["out"].encode(), v


# ---- 2. placement -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seq_fmt", FMTS)
def test_placement_grid(oracle, seq_fmt):
    """single-read batches: every length x front pad x tail pad x address mod 4.  The four thread counts are dealt over the grid in
    turn (every length and every pad pair meets each of them: the innermost dimension has four values and the count moves on by one
    per case and by one more per row)"""
    t0, n = time.perf_counter(), 0
    for k, case in fc.grid_cases(seq_fmt):
        check_case(case, oracle, threads=(fc.THREADS[(k + k // 4) % 4],))
        n += 1
    assert n == len(fc.GRID_L) * len(fc.FRONTS) * len(fc.TAILS) * len(fc.SHIFTS)
    print("placement grid, format %d: %d batches in %.1f s" % (seq_fmt, n, time.perf_counter() - t0))


@pytest.mark.parametrize("seq_fmt", FMTS)
def test_placement_grid_long_read(oracle, seq_fmt):
    """L = 100 003: several trips of every thread count's loops, an odd tail"""
    n = 0
    for k, case in fc.grid_cases(seq_fmt, lengths=[fc.LONG_L]):
        check_case(case, oracle, threads=(fc.THREADS[(k + k // 4) % 4],))
        n += 1
    assert n == len(fc.FRONTS) * len(fc.TAILS) * len(fc.SHIFTS)


@pytest.mark.parametrize("seq_fmt", FMTS)
def test_gaps_between_reads(oracle, seq_fmt):
    for k, case in fc.gap_cases(seq_fmt):
        check_case(case, oracle, threads=(fc.THREADS[(k + k // 4) % 4],))


@pytest.mark.parametrize("one_buffer", [False, True])
@pytest.mark.parametrize("seq_fmt", FMTS)
def test_packed_batches(oracle, seq_fmt, one_buffer):
    """all lengths back to back, ascending and descending, at every thread count; also with bases and qualities interleaved in one buffer"""
    for shift in fc.SHIFTS:
        for ls in (fc.GRID_L, fc.GRID_L[::-1]):
            case = fc.packed(ls, seq_fmt, shift=shift, seed=40 + shift, one_buffer=one_buffer)
            if not one_buffer:  # the quality offsets take every residue mod 16, the base offsets both parities (and, over the shifts, every address mod 4)
                assert {int(o) % 16 for o in case.qoff} == set(range(16)) and {int(o) % 2 for o in case.batch.read_seq_off} == {0, 1}
            exp = check_case(case, oracle, threads=fc.THREADS)
            assert len(exp["entries"]) > 100


# ---- 3. base codes --------------------------------------------------------------------------------------------------------------------------------

def test_every_bam4_code_in_both_nibbles(oracle):
    """all 16 codes as first and as last base of odd and even reads (the last base of an odd read is a high nibble, of an even read a low
    one), and all 256 pairs inside a read"""
    reads = []
    for L in (1, 2, 3, 4, 31, 32, 33, 64, 65):
        for a in range(16):
            for b in range(16) if L <= 4 else (15 - a,):
                codes = np.full(L, 1, np.uint8)
                codes[0], codes[-1] = a, b if L > 1 else a
                reads.append((L, 0x10, codes, None))
    pairs = np.array([[a, b] for a in range(16) for b in range(16)], np.uint8).reshape(-1)
    reads.append((512, 0x10, pairs, None))
    reads.append((513, 0x10, np.concatenate([[7], pairs]).astype(np.uint8), None))  # the same pairs across the byte boundaries
    for shift in (0, 1):
        case = fc.build(reads, [], BAM4, shift=shift, seed=8, name="bam4 codes")
        exp = check_case(case, oracle, threads=(1, 64))
        assert len(exp["entries"]) == len(reads)


def test_every_ascii_byte(oracle):
    reads = [(256, 0x10, np.arange(256, dtype=np.uint8), None), (255, 0x10, np.arange(255, 0, -1, dtype=np.uint8), None), (1, 0x10, [0], None), (1, 0x10, [255], None)]
    for shift in (0, 3):
        case = fc.build(reads, [], ASCII, shift=shift, seed=9, name="ascii bytes")
        check_case(case, oracle, threads=(1, 7))


# ---- 4. the item and read rows -------------------------------------------------------------------------------------------------------------------

def test_ref_end_and_bin(oracle):
    case = fc.end_bin_case()
    exp = check_case(case, oracle)
    ends, bins = exp["item_ref_end"], exp["item_bin"]
    assert (ends == case.lift.item_ref_pos).sum() > 30 and int(ends.max()) == 1 << 29 and int(case.lift.item_cigar_len.max()) == 70_000
    assert {0, 1, 9, 73, 585, 4681} <= set(int(b) for b in bins)  # a bin of every level


@pytest.mark.parametrize("seq_fmt", FMTS)
def test_flag_patterns(oracle, seq_fmt):
    case = fc.flag_case(seq_fmt)
    exp = check_case(case, oracle, threads=(64,))
    # source 0x800 on primaries and on unmapped copies is cleared; everything else of the source flag survives
    prim = exp["item_is_primary"] == 1
    assert prim.sum() == 3 * 128 and not (exp["item_flag"][prim] & 0x800).any() and (exp["item_flag"][~prim] & 0x800).all()
    unm = exp["read_n_lifted"] == 0
    assert unm.sum() == 128 and not (exp["read_unmapped_flag"][unm] & 0x810).any() and (exp["read_unmapped_flag"][unm] & 0x4).all()
    assert ((case.flags[unm] & 0x800) != 0).sum() == 64


def test_primary_choice(oracle):
    case = fc.primary_case()
    exp = check_case(case, oracle)
    p = exp["read_primary_item"]
    first = {int(r): i for i, r in reversed(list(enumerate(exp["item_read"])))}  # a read's first item
    rel = [int(p[r]) - first[r] if p[r] != fx.NO_ITEM else None for r in range(case.batch.n_reads)]
    assert rel[:6] == [None, 0, 1, 0, 0, 1]                      # the MAPQ rows: first of a tie wins
    assert rel[6:18] == [3, 1, 0] * 4                            # the non-lifted item with MAPQ 200 never wins
    assert rel[18:23] == [None] * 5 and rel[-1] is None and rel[-2] == 0
    assert int(exp["read_n_lifted"][23]) == 56 and case.lift.item_mapq[p[23]] == max(case.lift.item_mapq[i] for i in range(case.lift.n_items) if exp["item_read"][i] == 23 and case.lift.item_status[i] == 0)


def test_fault_count(oracle):
    """emu_finish_batch returns what plo_finish_batch_dev refuses a batch for: LEN_MISMATCH, PANIC and NEED_BASES count, NO_LIFTOVER does not"""
    for statuses, want in (([fc.L_, fc.NOLIFT, fc.L_], 0), ([fc.MISMATCH], 1), ([fc.PANIC], 1), ([fc.NEED], 1), ([fc.NOLIFT], 0),
                           ([fc.MISMATCH, fc.L_, fc.PANIC, fc.NOLIFT, fc.NEED, fc.NEED, fc.L_], 4)):
        case = fc.fault_case(statuses)
        exp = fx.finish(*case.fin())
        assert exp["n_fault"] == want
        for t in (1, 64):
            got = emu_lib.finish_batch(*case.fin(), nthreads=t)
            assert got["n_fault"] == want, statuses
            fx.compare(got, exp, "fault")


def test_empty_batches(oracle):
    for case in fc.empty_cases():
        check_case(case, oracle, threads=(1, 256), names=fc.SA_NAMES)


# ---- 5. SA ---------------------------------------------------------------------------------------------------------------------------------------

def test_sa_text(oracle):
    case = fc.sa_case()
    exp = check_case(case, oracle, names=fc.SA_NAMES)
    vals = fx.sa_values(case.batch, case.lift, exp["item_flag"], fc.SA_NAMES)
    assert vals[0] is None and vals[1] == b"chrUn_last,10,-,10M,9,0;" and vals[2] == b"1,9,+,9M,0,0;"
    assert vals[3] == b"chr2,100,+,268435455M,99,0;1,999999,-,1M2I3D4N5S6H7P8=9X10B,100,0;"  # a reverse read: the flipped record is '+'
    assert vals[7].startswith(b"chrUn_last,1000000,+,,255,0;") and vals[6].startswith(b"1,2147483649,-,1M,0,0;" + b"x" * 40 + b",1,+,1M1I")  # an empty CIGAR
    n_tags = [sum(v is not None for v, r in zip(vals, exp["item_read"]) if r == k) for k in range(7)]
    assert n_tags == [0, 2, 3, 5, 2, 0, 0]
    assert vals[11] is None and vals[13] is None and vals[12] == b"chrUn_last,9,-,4M,7,0;" and vals[14] == b"1,99,+,4M,7,0;"  # 4 items, 2 lifted
    text = b"".join(v for v in vals if v)
    for s in (b",9,", b",10,", b",99,", b",100,", b",999999,", b",1000000,", b",2147483649,", b",0,0;", b",255,0;", b"9M", b"10I", b"99999999", b"268435455"):
        assert s in text, s


# ---- 6. AddressSanitizer + UBSan: every array a heap block of its exact size ------------------------------------------------------------------------

ASAN_FRONTS, ASAN_TAILS = (0, 3, 4), (0, 7, 8, 23, 24, 27, 28)


def asan_cases():
    """(case, thread counts, chromosome names or None): the placement grid with front and tail pads of 0 and at the kernel's constants (there
    the first and the last record touch the ends of their blocks), the packed batches, the item rows and the SA cases"""
    out = []
    for seq_fmt in FMTS:
        for k, case in fc.grid_cases(seq_fmt, fronts=ASAN_FRONTS, tails=ASAN_TAILS):
            out.append((case, fc.THREADS if k % 7 == 0 else (fc.THREADS[(k + k // 4) % 4],), None))
        for k, case in fc.grid_cases(seq_fmt, lengths=[fc.LONG_L], fronts=(0, 4), tails=(0, 8, 28)):
            out.append((case, (fc.THREADS[k % 4], 256), None))
        for one_buffer in (False, True):
            for shift in fc.SHIFTS:
                for ls in (fc.GRID_L, fc.GRID_L[::-1]):
                    out.append((fc.packed(ls, seq_fmt, shift=shift, seed=40 + shift, one_buffer=one_buffer), fc.THREADS, None))
        out.append((fc.flag_case(seq_fmt), (7,), None))
    out += [(fc.sa_case(), (7,), fc.SA_NAMES), (fc.primary_case(), (64,), fc.SA_NAMES), (fc.end_bin_case(), (1,), None),
            (fc.fault_case([fc.MISMATCH, fc.L_, fc.PANIC, fc.NOLIFT, fc.NEED]), (7,), fc.SA_NAMES)]
    out += [(c, (1, 256), fc.SA_NAMES) for c in fc.empty_cases()]
    return out


def test_sanitizer_program(tmp_path):
    """tests/emu/emu_finish.cpp: a load or store outside a block ends the program; its results are the reference's"""
    t0 = time.perf_counter()
    cases = asan_cases()
    rc, err_text, res = efl.run_asan(cases, str(tmp_path))
    assert rc == 0, err_text[-4000:]
    n = 0
    for (case, threads, names), (runs, sa) in zip(cases, res):
        exp = fx.finish(*case.fin())
        for t, got in zip(threads, runs):
            n += fx.compare(got, exp, "sanitizer program %s, %d threads" % (case.name, t))
        if names is not None:
            assert api.assemble_sa_values(sa[0], sa[1], exp["item_read"].astype(np.uint32)) == fx.sa_values(case.batch, case.lift, exp["item_flag"], names), case.name
    assert len(cases) > 18_000 and n > 35_000
    print("sanitizer program: %d batches, %d reversed records in %.1f s" % (len(cases), n, time.perf_counter() - t0))


# ---- 7. the device ---------------------------------------------------------------------------------------------------------------------------------
# plo_finish_batch_dev works on the context's own lift, so the items come from a real lift over finish_cases.lift_index().  Every test
# first holds the device lift against the oracle's and the item table against the one the case was built for.
# Only this leg runs: k_finish_items / k_finish_reads as kernels with the atomic fault count, the three scans and k_finish_offsets,
# k_revcomp's entry loop (flist, the grid stride) at 256 threads on real addresses, k_sa_len / k_sa_emit, and the host part of the refusal.

@pytest.fixture(scope="module")
def lift_ctx():
    ixd = fc.lift_index()
    index = api.Index(ixd, 0)
    yield ixd, index
    index.close()


def seg_for(name, at, flag, flip, ops=None):
    """a read segment on contig segment `name` whose record is flipped or not, as asked"""
    cfwd = fc.LIFT_SEGS[fc.INS_SEG if name == "ins" else name][2] if name != "gap" else 1
    rev = bool(flag & 0x10)
    sfwd = rev if (bool(flip) ^ (not cfwd)) else not rev
    return (name, at, int(sfwd), ops)


class DeviceCase:
    """a finish_cases.Case on the device: the arrays the views were cut from go up whole, the device tensors are sliced like the views"""

    def __init__(self, case):
        import ctypes as C

        import torch

        from portello_amd import devbatch

        self.case, b = case, case.batch
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).to("cuda")

        def up_view(view):
            base = view.base if view.base is not None else view
            shift = view.ctypes.data - base.ctypes.data
            whole = torch.from_numpy(base if len(base) >= 16 else np.concatenate([base, np.zeros(16, np.uint8)])).to("cuda")
            t = whole[shift:shift + len(view)]
            assert t.data_ptr() % 4 == shift % 4
            return whole, t

        self.seq_whole, self.seq = up_view(b.seq)
        self.qual_whole, self.qual = (self.seq_whole, self.seq) if case.qual.ctypes.data == b.seq.ctypes.data else up_view(case.qual)
        self.db = devbatch.DeviceBatch(read_is_reverse=up(b.read_is_reverse, np.uint8), read_seq_len=up(b.read_seq_len, np.int32), read_seq_off=up(b.read_seq_off, np.int64),
                                       seq=self.seq, seq_fmt=b.seq_fmt, seg_read=up(b.seg_read, np.int32), seg_contig=up(b.seg_contig, np.int32),
                                       seg_pos=up(b.seg_pos, np.int64), seg_is_fwd_strand=up(b.seg_is_fwd_strand, np.uint8),
                                       seg_cigar_off=up(b.seg_cigar_off, np.int32), cigar=up(b.cigar, np.int32))
        self.flags, self.qoff = up(case.flags, np.int16), up(case.qoff, np.int64)
        p = lambda t, ct: C.cast(C.c_void_p(t.data_ptr()), C.POINTER(ct))
        self.fin = abi.PloFinishIn(p(self.flags, C.c_uint16), p(self.qual, C.c_uint8), p(self.qoff, C.c_uint64), len(case.qual))
        self.desc = self.db.desc()
        assert self.desc.seq_bytes == len(b.seq)
        torch.cuda.synchronize()


def check_table(lift, batch, table):
    """the case did not degenerate: status, flip, MAPQ, chromosome and position of every item, hence the records per read"""
    assert lift.n_items == len(table), (lift.n_items, len(table))
    item_read = np.asarray(batch.seg_read)[lift.item_seg]
    for i, (r, st, flip, mq, chrom, pos) in enumerate(table):
        assert (int(item_read[i]), int(lift.item_status[i]), int(lift.item_mapq[i]), int(lift.item_chrom_index[i])) == (r, st, mq, chrom), (i, table[i])
        if st == fc.L_:
            assert (int(lift.item_need_flipped[i]), int(lift.item_ref_pos[i])) == (flip, pos), (i, table[i])


def lift_on_device(eng, dc, ixd, oracle, table):
    from portello_amd import devbatch

    out = eng.liftover_batch_dev(dc.desc)
    eng.compact_output_dev(out)
    lift = devbatch.download(eng, out)
    assert lift.canonical() == oracle.liftover_batch(ixd, dc.case.batch, abi.STAGES_ALL, 2).canonical()
    check_table(lift, dc.case.batch, table)
    return lift


def check_device(eng, case, table, ixd, oracle, sa=None):
    """lift, finish and SA text of one batch on the device against the reference (and the oracle against it) -> the reference's result"""
    from portello_amd import devbatch

    dc = DeviceCase(case)
    lift = lift_on_device(eng, dc, ixd, oracle, table)
    fo = eng.finish_batch_dev(dc.desc, dc.fin)
    got = devbatch.download_finish(eng, fo, lift.n_items, case.batch.n_reads)
    exp = fx.finish(case.batch, case.flags, case.qual, case.qoff, lift)
    fx.compare(got, exp, "device " + case.name)
    fx.compare(oracle.finish_batch(case.batch, case.flags, case.qual, case.qoff, lift), exp, "oracle " + case.name)
    assert fo.revcomp_ms >= 0 and (fo.n_items, fo.n_reads) == (lift.n_items, case.batch.n_reads)
    if sa is not None:
        off, text = devbatch.download_sa(eng, eng.sa_segments_dev(sa[0]))
        want = fx.sa_values(case.batch, lift, exp["item_flag"], fc.LIFT_NAMES)
        assert api.assemble_sa_values(off, text, exp["item_read"].astype(np.uint32)) == want, case.name
        assert oracle.sa_values(case.batch, lift, exp["item_flag"], fc.LIFT_NAMES) == want, case.name
        exp["sa"] = want
    return exp


def new_engine(index):
    import torch

    from portello_amd import devbatch

    eng = api.Engine(index, stream=torch.cuda.current_stream().cuda_stream)
    return eng, devbatch.sa_inputs(fc.LIFT_NAMES, "cuda")


def packed_reads(lengths):
    """as finish_cases.packed: even reads get a flipped record on A (every third a second one, not flipped, on the reverse segment B), odd
    reads are reverse and lie in the uncovered stretch, so that their unmapped copy is the flipped entry"""
    reads = []
    for r, L in enumerate(lengths):
        if r & 1:
            fl = 0x10 | (0x400 if r % 4 == 1 else 0)
            reads.append((L, fl, [seg_for("gap", 10 * r, fl, r % 4 == 1)]))
        else:
            segs = [seg_for("A", 1001 * r, 0x1, 1)]
            if r % 3 == 0:
                segs.append(seg_for("B", 50 * r, 0x1, 0))
            reads.append((L, 0x1, segs))
    return reads


@pytest.mark.gpu
@pytest.mark.parametrize("one_buffer", [False, True])
@pytest.mark.parametrize("seq_fmt", FMTS)
def test_device_packed_placement(lift_ctx, oracle, seq_fmt, one_buffer):
    ixd, index = lift_ctx
    eng, sa = new_engine(index)
    ls = [L for L in fc.GRID_L if L]
    n = 0
    for shift in fc.SHIFTS:
        for front, tail in ((0, 0), (3, 7), (4, 28)):
            for order in (ls, ls[::-1]):
                case, table = fc.lift_case(packed_reads(order), seq_fmt, front=front, tail=tail, shift=shift, one_buffer=one_buffer, seed=60 + n)
                exp = check_device(eng, case, table, ixd, oracle, sa)
                assert len(exp["entries"]) == len(ls)
                n += 1
    eng.close()


@pytest.mark.gpu
def test_device_single_read_batches(lift_ctx, oracle):
    ixd, index = lift_ctx
    eng, sa = new_engine(index)
    k = 0
    for L in (1, 15, 16, 17, 31, 32, 33, 40):
        for front in (0, 3, 4):
            for tail in (0, 7, 28):
                case, table = fc.lift_case([(L, 0, [seg_for("A", 77, 0, 1)])], BAM4, front=front, tail=tail, shift=k % 4, seed=k)
                assert len(check_device(eng, case, table, ixd, oracle)["entries"]) == 1
                k += 1
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seq_fmt", FMTS)
def test_device_long_flipped_read(lift_ctx, oracle, seq_fmt):
    """100 003 bases: several trips of the 256-thread loops, an odd tail, every slot of the unrolled groups with and without the early break"""
    ixd, index = lift_ctx
    eng, sa = new_engine(index)
    for shift, front, tail in ((1, 3, 7), (0, 0, 0)):
        case, table = fc.lift_case([(fc.LONG_L, 0x10, [seg_for("A", 5, 0x10, 1)]), (40, 0, [seg_for("B", 9, 0, 1)])], seq_fmt, front=front, tail=tail, shift=shift, seed=70)
        assert len(check_device(eng, case, table, ixd, oracle, sa)["entries"]) == 2
    eng.close()


@pytest.mark.gpu
def test_device_more_flipped_reads_than_workgroups(lift_ctx, oracle):
    """5 000 flipped reads of 1..40 bases: more entries than the n_cus * 16 workgroups of k_revcomp (4 096 at 256 CUs), so its grid-stride loop
    runs"""
    ixd, index = lift_ctx
    eng, sa = new_engine(index)
    reads = [(1 + r % 40, 0, [seg_for("A", 20 * r, 0, 1)]) for r in range(5000)]
    case, table = fc.lift_case(reads, BAM4, front=1, tail=2, shift=3, seed=71)
    assert len(check_device(eng, case, table, ixd, oracle)["entries"]) == 5000
    eng.close()


def row_reads():
    """the primary, flag and SA rows a real lift can produce.  -> (reads, {name: read index})"""
    reads, at = [], {}
    rich = list(cg.encode("3S4=1X2I5M1D6M7N5M"))  # 26 read bases

    def read(name, L, flag, placed):
        at[name] = len(reads)
        reads.append((L, flag, [seg_for(n, o, flag, f, ops) for n, o, f, ops in placed]))

    read("none first", 12, 0x10, [("gap", 0, 0, None)])
    read("60 60", 20, 0, [("A", 0, 0, None), ("B", 0, 1, None)])                                   # pos 8 -> "9"
    read("7 60 60", 21, 0x10, [("C", 8, 0, None), ("A", 1, 1, None), ("B", 3, 0, None)])           # pos 999 998, 9
    read("0 0 0", 9, 0, [("D", 0, 1, None), ("E", 0, 0, None), ("F", 0, 1, None)])                 # op length 9
    read("255 0", 10, 0, [("G", 0, 0, None), ("D", 5, 1, None)])                                   # op length 10
    read("0 255", 10, 0x10, [("D", 5, 1, None), ("G", 2000, 0, None)])
    read("nolift between", 16, 0, [("A", 500, 0, None), ("ins", 10, 0, None), ("B", 500, 1, None)])
    read("nolift first", 16, 0x10, [("ins", 20, 0, None), ("F", 10, 1, None), ("K", 10, 0, None)])
    read("none middle 1", 5, 0x10, [("gap", 9000, 1, None)])
    read("none middle 2", 6, 0x0, [("ins", 30, 0, None)])
    read("none middle 3", 7, 0x810, [("gap", 50, 0, None), ("ins", 40, 1, None)])
    read("five", 26, 0, [("H", 8, 0, rich), ("I", 100, 1, rich), ("J", 0, 0, None), ("ins", 50, 0, None), ("K", 0, 1, None), ("C", 9, 0, rich)])  # pos 98, 999 999
    read("h99", 11, 0x10, [("H", 9, 1, None), ("G", 9000, 0, None)])                               # pos 99 -> "100"
    read("seventy", 8, 0, [("A", 2000 + 10 * k, k & 1, None) if k % 5 else ("ins", k, 0, None) for k in range(70)])
    for pat in range(1 << len(fc.FLAG_BITS)):
        fl = sum(b for k, b in enumerate(fc.FLAG_BITS) if pat >> k & 1)
        L = 1 + pat % 37
        reads.append((L, fl, [seg_for("F", 5000 + pat, fl, 0)]))
        reads.append((L, fl, [seg_for("E", 5000 + pat, fl, 1)]))
        reads.append((L, fl, [seg_for("gap", 20 * pat, fl, 0)]))
        reads.append((L, fl, [seg_for("J", 100, fl, 0), seg_for("K", 100 + pat, fl, 1), seg_for("H", 100, fl, 0)]))
    read("none last", 13, 0x10, [("gap", 9900, 0, None)])
    return reads, at


@pytest.mark.gpu
def test_device_primary_flag_and_sa_rows(lift_ctx, oracle):
    ixd, index = lift_ctx
    eng, sa = new_engine(index)
    reads, at = row_reads()
    case, table = fc.lift_case(reads, BAM4, front=2, tail=1, shift=1, seed=72)
    exp = check_device(eng, case, table, ixd, oracle, sa)
    first = {int(r): i for i, r in reversed(list(enumerate(exp["item_read"])))}
    rel = lambda name: int(exp["read_primary_item"][at[name]]) - first[at[name]]
    assert [rel(n) for n in ("60 60", "7 60 60", "0 0 0", "255 0", "0 255", "nolift between", "nolift first", "five")] == [0, 1, 0, 0, 1, 0, 2, 4]
    nl = exp["read_n_lifted"]
    assert [int(nl[at[n]]) for n in ("none first", "none middle 1", "none middle 2", "none middle 3", "none last", "five", "seventy", "nolift between")] == [0, 0, 0, 0, 0, 5, 56, 2]
    vals = exp["sa"]
    i0 = first[at["60 60"]]
    assert vals[i0] == b"chr2,10031,-,20M,60,0;" and vals[i0 + 1] == b"1,9,+,20M,60,0;"
    text = b"".join(v for v in vals if v)
    for s in (b"1,9,", b"1,10,", b"chrUn_last,99,", b"chrUn_last,100,", b"x" * 40 + b",999999,", b"x" * 40 + b",1000000,", b",0,0;", b",9,0;", b",10,0;", b",99,0;", b",100,0;",
              b",255,0;", b",9M,", b",10M,"):
        assert s in text, s
    eng.close()


@pytest.mark.gpu
def test_device_refusal(lift_ctx, oracle):
    """a read whose CIGAR disagrees with read_seq_len ends LEN_MISMATCH in the lift (a data error it reports): plo_finish_batch_dev refuses the
    batch with the count, SA and records refuse behind it, and the context finishes the next good batch"""
    ixd, index = lift_ctx
    eng, sa = new_engine(index)
    good = [(30, 0, [seg_for("A", 10, 0, 1)]), (31, 0x10, [seg_for("B", 10, 0x10, 0), seg_for("C", 10, 0x10, 1)])]
    bad = good + [(32, 0, [seg_for("A", 300, 0, 0, [fc.M(31)]), seg_for("B", 300, 0, 1, [fc.M(30)]), seg_for("C", 300, 0, 0)]), (33, 0, [seg_for("F", 0, 0, 0, [fc.M(35)])])]
    case, table = fc.lift_case(bad, BAM4, seed=73)
    table = [(r, fc.MISMATCH if (r, k) in ((2, 3), (2, 4), (3, 6)) else st, fl, mq, ch, pos) for k, (r, st, fl, mq, ch, pos) in enumerate(table)]
    dc = DeviceCase(case)
    lift = lift_on_device(eng, dc, ixd, oracle, table)
    assert (lift.item_status == fc.MISMATCH).sum() == 3
    with pytest.raises(api.PortelloError, match=r"3 item\(s\) ended LEN_MISMATCH / PANIC") as e:
        eng.finish_batch_dev(dc.desc, dc.fin)
    assert e.value.status == abi.PLO_ERR_DATA
    with pytest.raises(api.PortelloError, match="plo_finish_batch_dev on the batch first") as e:
        eng.sa_segments_dev(sa[0])
    assert e.value.status == abi.PLO_ERR_INVALID_ARG
    with pytest.raises(api.PortelloError, match="no finishing result") as e:
        eng.records_build_dev(dc.desc, abi.PloRecordsIn())
    assert e.value.status == abi.PLO_ERR_INVALID_ARG
    case, table = fc.lift_case(good, BAM4, shift=2, seed=74)
    assert len(check_device(eng, case, table, ixd, oracle, sa)["entries"]) == 2
    eng.close()
