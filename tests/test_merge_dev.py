"""Sorted windows merged into large runs on the device: plo_runs_merge_plan_dev / plo_runs_merge_emit_dev (portello_amd/csrc/merge_core.hpp)
and run_bam_to_bam(sorted_runs=True, run_windows=K).

The yardstick is tests/merge_expect.py: the records numbered run-major, sorted(range(n), key=(key, g)), the concatenated bytes and offsets
and the greedy chunk table -- plain Python from the definition, not derived from the code under test.  All comparisons are of integers and
bytes.  The CPU tests run merge_core.hpp under the wave emulator (tests/emu/emu_merge.cpp), the two calls issued as engine.hip issues them,
with both thread orders -- every chunk's output between canary bytes, every byte of it watched to be stored exactly once -- and once more
in a program built with AddressSanitizer + UBSan where every array sits in a heap block of its exact size.  The GPU tests run the C ABI on
the device, against the yardstick and against plo_records_sort_dev over the runs' concatenation, and the pipeline mode."""
import os
import random

import numpy as np
import pytest

import bamcheck
import emu_merge_lib as eml
import merge_expect as mx
import sort_expect as sx
from portello_amd import abi, api, bam, bamsynth

T = 256  # MERGE_THREADS (test_block_size_runs asserts it)
OK, INVALID = abi.PLO_OK, abi.PLO_ERR_INVALID_ARG
rec = sx.make_record


def random_records(n, n_ref, seed, pos_span=40, max_payload=24):
    """n short records: few distinct keys (so that ties are many), an unplaced share, lengths over all residues mod 16"""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        ref = rng.choice([-1, 0, n_ref - 1, rng.randrange(n_ref)])
        out.append(rec(ref, rng.randrange(-1, pos_span), rng.choice([0, 16, 4, 1 | 16]), b"q%d_%d" % (seed, i), bytes(rng.randrange(256) for _ in range(rng.randrange(max_payload)))))
    return out


def in_order(recs, n_ref):
    return [recs[i] for i in sorted(range(len(recs)), key=lambda i: (sx.key_of(recs[i], n_ref), i))]


def sorted_run(n, n_ref, seed, **kw):
    return in_order(random_records(n, n_ref, seed, **kw), n_ref)


def as_runs(runs):
    return [sx.concat(r) for r in runs]


def check_plan(res, e, what=""):
    assert res["status"] == OK and res["err_run"] == res["err_record"] == 0xFFFFFFFF and res["err_kind"] == 0, (what, res["status"])
    assert res["n_records"] == len(e["src"]) and res["n_bytes"] == len(e["bytes"]) and res["n_mapped"] == e["n_mapped"], what
    assert res["n_chunks"] == len(e["chunks"]), what
    for name in ("src", "key", "record_off", "chunk_first", "chunk_off"):
        assert np.array_equal(res[name], e[name]), (what, name)


def check_emits(res, e, emits, what=""):
    assert len(res["emits"]) == len(emits)
    for c, got in zip(emits, res["emits"]):
        assert got["status"] == OK, (what, c, got["status"])
        assert got.get("check", 0) == 0, (what, c, got["check"])  # 2: a store outside the output or its piece, 3: a byte not stored exactly once
        want_bytes, want_off = e["chunks"][c]
        assert got["first"] == int(e["chunk_first"][c]) and got["n_records"] == len(want_off) - 1, (what, c)
        assert np.array_equal(got["record_off"], want_off) and got["bytes"] == want_bytes, (what, c)


def ok_case(runs, n_ref, chunk_bytes, seed=0, flags=0, emits=None):
    """-> (case, expectation, emit list): every chunk in order unless `emits` says otherwise"""
    rr = as_runs(runs)
    assert mx.first_offender(rr, n_ref) is None
    e = mx.expect(rr, n_ref, chunk_bytes)
    em = list(range(len(e["chunks"]))) if emits is None else emits
    return eml.case(rr, n_ref, chunk_bytes, em, e["bytes"], order_seed=seed, flags=flags), e, em


def run_ok(triples, runner=eml.run):
    res = runner([t[0] for t in triples])
    for k, (r, (c, e, em)) in enumerate(zip(res, triples)):
        check_plan(r, e, k)
        check_emits(r, e, em, k)
        if em == list(range(len(e["chunks"]))):
            assert b"".join(g["bytes"] for g in r["emits"]) == e["bytes"], k
    return res


# ---- the case families (shared by the emulator tests, the sanitizer program and the device test) ----------------------------------------------

def hand_case():
    """three runs, seven records, a tie across runs (a / c, b / f), one unplaced record; g = a0 b1 | c2 d3 u4 | e5 f6"""
    return [[rec(0, 5, 0, b"a"), rec(1, 3, 0, b"b")], [rec(0, 5, 0, b"c"), rec(0, 5, 16, b"d"), rec(-1, -1, 4, b"u")], [rec(0, 2, 0, b"e"), rec(1, 3, 0, b"f")]]


def run_count_cases():
    out = {}
    for k in (1, 2, 3, 4, 5, 8, 9, 17):
        out["%d runs" % k] = ([sorted_run(5 + (7 * r + k) % 23, 25, 1000 + 31 * k + r) for r in range(k)], 25)
    return out


def empty_run_cases():
    a, b = sorted_run(40, 25, 21), sorted_run(33, 25, 22)
    return {"empty first": ([[], a, b], 25), "empty middle": ([a, [], [], b], 25), "empty last": ([a, b, []], 25), "empty only": ([[]], 25),
            "all empty": ([[], [], []], 25), "no run": ([], 25)}


def key_cases():
    out = {}
    out["one key"] = ([[rec(2, 77, 0, b"k%d_%d" % (r, i), bytes(i % 19)) for i in range(20 + r)] for r in range(4)], 25)
    tie = lambda r: in_order([rec(1, 9, f, b"t%d%d" % (r, i)) for i, f in enumerate([0, 16, 0, 16, 16, 0])] + [rec(1, 8, 16, b"lo%d" % r), rec(1, 10, 0, b"hi%d" % r)], 25)  # noqa: E731
    out["ties across three runs on both strands"] = ([tie(0), tie(1), tie(2)], 25)
    out["an unplaced tail in every run"] = ([in_order(random_records(30, 25, 40 + r) + [rec(-1, 50 + i, 4, b"u%d%d" % (r, i), bytes(i)) for i in range(1 + r)], 25) for r in range(5)], 25)
    out["n_ref 1"] = ([sorted_run(50, 1, 50 + r) for r in range(3)], 1)
    out["n_ref 25"] = ([in_order(random_records(50, 25, 60 + r) + [rec(24, sx.POS_MAX, 16, b"last%d" % r), rec(-1, 0, 4, b"tail%d" % r)], 25) for r in range(3)], 25)
    return out


def big_record_runs():
    big = rec(0, 15, 0, b"big", np.random.default_rng(9).integers(0, 256, 200_003 - 36 - 3, dtype=np.uint8).tobytes())
    assert len(big) == 200_003
    return [sorted_run(60, 3, 70, max_payload=260), in_order(random_records(40, 3, 71, max_payload=260) + [big], 3), sorted_run(25, 3, 72, max_payload=260)]


def chunk_size_cases():
    runs = [sorted_run(300, 25, 80 + r, max_payload=260) for r in range(3)]
    total, largest = sum(len(x) for r in runs for x in r), max(len(x) for r in runs for x in r)
    assert total > 3 * 16384
    return {"4096": (runs, 4096), "16384": (runs, 16384), "one byte below the largest record": (runs, largest - 1), "above the total": (runs, total + 1)}


def refusals(n_ref=25):
    """name -> ([(data, off)], n_bytes or None, (run, place, kind)): an offender of each kind at place 7 (8 for kind 6) of run 0, of a middle
    run and of the last run of four, and a second, later offender so that "lowest" is tested"""
    out = {}
    for where, r in (("run 0", 0), ("a middle run", 2), ("the last run", 3)):
        for kind in range(1, 7):
            runs = [sorted_run(30, n_ref, 90 + k) for k in range(4)]
            at = 7
            if kind == sx.ERR_SHORT:
                runs[r][at] = rec(0, 1)[:35]
            elif kind == sx.ERR_BLOCK:
                runs[r][at] = rec(0, 1, 0, b"name", block_size=37)
            elif kind == sx.ERR_REFID:
                runs[r][at] = rec(n_ref, 1)
            elif kind == sx.ERR_POS:
                runs[r][at] = rec(0, -2)
            elif kind == mx.ERR_ORDER:
                at = next(i for i in range(7, 29) if sx.key_of(runs[r][i], n_ref) != sx.key_of(runs[r][i + 1], n_ref))
                runs[r][at], runs[r][at + 1] = runs[r][at + 1], runs[r][at]
                at += 1
            if r < 3:
                runs[r + 1][3] = rec(-2, 0)  # the later offender
            else:
                runs[r][25] = rec(-2, 0)
            rr = as_runs(runs)
            if kind == sx.ERR_OFFSET:
                off = rr[r][1].copy()
                off[at + 1] = off[at] - 1
                rr[r] = (rr[r][0], off)
            want = (r, at, kind)
            assert mx.first_offender(rr, n_ref) == want, (where, kind)
            out["kind %d in %s" % (kind, where)] = (rr, None, want)
    # the other two shapes of kind 1: record_off[0] != 0 in a middle run, record_off[n] != n_bytes in the last
    runs = as_runs([sorted_run(30, n_ref, 95 + k) for k in range(3)])
    off = runs[1][1].copy()
    off[0] = 1
    out["record_off[0] != 0"] = ([runs[0], (runs[1][0], off), runs[2]], None, (1, 0, sx.ERR_OFFSET))
    out["record_off[n] != n_bytes"] = (runs, [len(runs[0][0]), len(runs[1][0]), len(runs[2][0]) + 1], (2, 29, sx.ERR_OFFSET))
    return out


# ---- CPU: merge_core.hpp under the wave emulator ---------------------------------------------------------------------------------------------

def test_expectation_by_hand():
    """the yardstick itself, and the code under it, on an example small enough to merge by eye"""
    runs = hand_case()
    e = mx.expect(as_runs(runs), 2, 80)
    assert list(e["src"]) == [5, 0, 2, 3, 1, 6, 4] and e["n_mapped"] == 6
    assert list(e["key"]) == [6, 12, 12, 13, (1 << 32) | 8, (1 << 32) | 8, 2 << 32]
    flat = [x for r in runs for x in r]
    assert all(len(x) == 37 for x in flat) and e["bytes"] == b"".join(flat[g] for g in (5, 0, 2, 3, 1, 6, 4))
    assert list(e["chunk_first"]) == [0, 2, 4, 6, 7] and list(e["chunk_off"]) == [0, 74, 148, 222, 259]  # two records of 37 bytes keep to 80
    assert mx.chunk_table([37] * 7, 36) == list(range(8)) and mx.chunk_table([37] * 7, 259) == [0, 7] and mx.chunk_table([], 5) == [0]
    for seed in (0, 1):
        run_ok([ok_case(runs, 2, 80, seed)])


@pytest.mark.parametrize("name", sorted(run_count_cases()))
def test_run_counts(name):
    """n_runs around every power of two the rank rounds double over: a group without a sibling in some round, in every round, in none"""
    runs, n_ref = run_count_cases()[name]
    run_ok([ok_case(runs, n_ref, 4096, seed) for seed in (0, 1)])


@pytest.mark.parametrize("name", sorted(empty_run_cases()))
def test_empty_runs(name):
    """runs of 0 records as the first, middle, last and only run, their pointers given and NULL"""
    runs, n_ref = empty_run_cases()[name]
    res = run_ok([ok_case(runs, n_ref, 4096, 0), ok_case(runs, n_ref, 4096, 1, flags=eml.NULL_EMPTY)])
    if not any(runs):
        assert res[0]["n_chunks"] == 0 and list(res[0]["record_off"]) == [0]
        (r,) = eml.run([eml.case(as_runs(runs), n_ref, 4096, [0])])
        assert r["status"] == OK and r["emits"][0]["status"] == INVALID  # a plan without a chunk has none to emit


@pytest.mark.parametrize("n", [T - 1, T, T + 1])
def test_block_size_runs(n):
    """a run of the rank kernel's block size - 1, + 0, + 1 against a run of 1, on either side"""
    assert eml.threads() == T
    a, one = sorted_run(n, 25, 300 + n), [rec(0, 20, 0, b"one")]
    run_ok([ok_case([a, one], 25, 16384, 0), ok_case([one, a], 25, 16384, 1), ok_case([one, a, one], 25, 4096, 0)])


@pytest.mark.parametrize("name", sorted(key_cases()))
def test_key_shapes(name):
    runs, n_ref = key_cases()[name]
    res = run_ok([ok_case(runs, n_ref, 4096, seed) for seed in (0, 1)])
    if name == "one key":
        assert list(res[0]["src"]) == list(range(res[0]["n_records"]))  # ties in g order: the concatenation
    if name == "n_ref 1":
        assert 0 < res[0]["n_mapped"] < res[0]["n_records"]


def test_a_200_kb_record():
    """one 200 003-byte record among 36-300-byte ones: a chunk of its own with chunk_bytes 16 384, a dozen pieces"""
    runs = big_record_runs()
    res = run_ok([ok_case(runs, 3, 16384, 0), ok_case(runs, 3, 1 << 20, 1)])
    assert any(e["n_records"] == 1 and len(e["bytes"]) == 200_003 for e in res[0]["emits"]) and res[1]["n_chunks"] == 1


@pytest.mark.parametrize("name", sorted(chunk_size_cases()))
def test_chunk_sizes(name):
    runs, chunk_bytes = chunk_size_cases()[name]
    res = run_ok([ok_case(runs, 25, chunk_bytes, seed) for seed in (0, 1)])
    if name == "above the total":
        assert res[0]["n_chunks"] == 1
    if name == "one byte below the largest record":
        assert any(e["n_records"] == 1 and len(e["bytes"]) == chunk_bytes + 1 for e in res[0]["emits"])


def test_chunks_out_of_order_and_twice():
    runs, chunk_bytes = chunk_size_cases()["4096"]
    e = mx.expect(as_runs(runs), 25, chunk_bytes)
    n = len(e["chunks"])
    assert n > 8
    order = list(range(n - 1, -1, -1)) + [3, 3, 0, n - 1, 5, 3]
    run_ok([ok_case(runs, 25, chunk_bytes, seed, emits=order) for seed in (0, 1)])


@pytest.mark.parametrize("name", sorted(refusals()))
def test_refusal(name):
    """every check refuses, names the LOWEST offending g by run and place and the first kind it breaks; a refused plan is no plan"""
    rr, n_bytes, want = refusals()[name]
    for seed in (0, 1):
        (r,) = eml.run([eml.case(rr, 25, 4096, [0], order_seed=seed, n_bytes=n_bytes)])
        assert (r["status"], r["err_run"], r["err_record"], r["err_kind"]) == (INVALID,) + want, name
        assert "src" not in r and r["emits"][0]["status"] == INVALID


def argument_refusals():
    """name -> (case, plan status or None for no plan, emit statuses)"""
    good = as_runs([sorted_run(20, 25, 1), sorted_run(20, 25, 2)])
    e = mx.expect(good, 25, 4096)
    one = sx.concat([rec(0, 1, 0, b"x")])
    empty = sx.concat([])
    out = {}
    out["n_runs 4097"] = (eml.case([one] + [empty] * 4096, 25, 4096, [0]), INVALID, [INVALID])
    out["n_runs 4096"] = (eml.case([empty] * 4095 + [one], 25, 4096, [0], one[0]), OK, [OK])
    out["chunk_bytes 0"] = (eml.case(good, 25, 0, [0]), INVALID, [INVALID])
    out["emit without a plan"] = (eml.case(good, 25, 4096, [0], flags=eml.NO_PLAN), -1, [INVALID])
    out["emit past n_chunks"] = (eml.case(good, 25, 4096, [0, len(e["chunks"]), 0xFFFFFFFF, len(e["chunks"]) - 1], e["bytes"]), OK, [OK, INVALID, INVALID, OK])
    out["a NULL run table"] = (eml.case(good, 25, 4096, [0], flags=eml.NULL_TABLE), INVALID, [INVALID])
    out["bytes without a record"] = (eml.case([good[0], empty], 25, 4096, [0], n_bytes=[len(good[0][0]), 4]), INVALID, [INVALID])
    return out


@pytest.mark.parametrize("name", sorted(argument_refusals()))
def test_argument_refusal(name):
    assert eml.max_runs() == mx.MAX_RUNS == abi.PLO_MERGE_MAX_RUNS
    c, plan, emits = argument_refusals()[name]
    (r,) = eml.run([c])
    assert r["status"] == plan and [e["status"] for e in r["emits"]] == emits
    assert all(e.get("check", 0) == 0 for e in r["emits"])


def test_asan_program(tmp_path):
    """the same cases through a stand-alone program with ASan + UBSan, every array in a heap block of its exact size, no guard bytes"""
    triples = [ok_case(hand_case(), 2, 80, 1)]
    for fam in (run_count_cases(), empty_run_cases(), key_cases()):
        for name, (runs, n_ref) in sorted(fam.items()):
            triples.append(ok_case(runs, n_ref, 4096, len(triples) & 1, flags=eml.NULL_EMPTY if len(triples) & 2 else 0))
    for n in (T - 1, T, T + 1):
        triples.append(ok_case([sorted_run(n, 25, 300 + n), [rec(0, 20, 0, b"one")]], 25, 16384, n & 1))
    triples.append(ok_case(big_record_runs(), 3, 16384, 0))
    for name, (runs, chunk_bytes) in sorted(chunk_size_cases().items()):
        triples.append(ok_case(runs, 25, chunk_bytes, 1))
    runs, chunk_bytes = chunk_size_cases()["4096"]
    triples.append(ok_case(runs, 25, chunk_bytes, 0, emits=[9, 2, 2, 0, 9]))
    for t in triples:
        t[0]["guard"] = 0
    bad = [(eml.case(rr, 25, 4096, [0], guard=0, n_bytes=nb), want) for name, (rr, nb, want) in sorted(refusals().items())]
    args = [(dict(c, guard=0), plan, emits) for name, (c, plan, emits) in sorted(argument_refusals().items())]
    cases = [t[0] for t in triples] + [b[0] for b in bad] + [a[0] for a in args]
    rc, err, res = eml.run_asan(cases, str(tmp_path))
    assert rc == 0, err[-3000:]
    assert "ERROR" not in err and "runtime error" not in err, err[-3000:]
    run_ok(triples, runner=lambda _: res[:len(triples)])
    for r, (_, want) in zip(res[len(triples):], bad):
        assert (r["status"], r["err_run"], r["err_record"], r["err_kind"]) == (INVALID,) + want and r["emits"][0]["status"] == INVALID
    for r, (_, plan, emits) in zip(res[len(triples) + len(bad):], args):
        assert r["status"] == plan and [e["status"] for e in r["emits"]] == emits


# ---- CPU: the pipeline's option ------------------------------------------------------------------------------------------------------------

def test_run_windows_option_validation(tmp_path):
    """run_windows != 1 needs sorted_runs, is no negative number, and the budget and chunk sizes are positive: refused before any device use"""
    from portello_amd import pipeline

    out = str(tmp_path / "x.bam")
    for k in (0, 2):
        with pytest.raises(ValueError, match="run_windows"):
            pipeline.run_bam_to_bam("in.bam", out, None, None, [], [], [], device_records=True, run_windows=k)
    for kw in (dict(run_windows=-1), dict(run_windows=2, run_chunk_bytes=0), dict(run_windows=2, run_budget_bytes=0)):
        with pytest.raises(ValueError, match="run_"):
            pipeline.run_bam_to_bam("in.bam", out, None, None, [], [], [], device_records=True, sorted_runs=True, **kw)
    assert not os.path.exists(out)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------

class DevMerger:
    """hand-made runs, each in a device allocation of its own, through Engine.runs_merge_plan_dev / runs_merge_emit_dev"""

    def __init__(self):
        import torch

        import test_records_dev as trd

        self.torch = torch
        self.dev = torch.device("cuda", 0)
        self.index = api.Index(trd.hand_index(), 0)
        self.eng = api.Engine(self.index)

    def upload(self, rr):
        t, held, runs = self.torch, [], []
        for data, off in rr:
            n = len(off) - 1
            if not n:
                runs.append((0, 0, 0, 0))
                continue
            raw = t.from_numpy(np.frombuffer(data, np.uint8).copy()).to(self.dev)
            offs = t.from_numpy(np.ascontiguousarray(off, np.uint64).view(np.int64)).to(self.dev)
            held += [raw, offs]
            runs.append((raw.data_ptr(), len(data), n, offs.data_ptr()))
        t.cuda.synchronize()
        return held, runs

    def check(self, runs, n_ref, chunk_bytes, what=""):
        rr = as_runs(runs)
        e = mx.expect(rr, n_ref, chunk_bytes)
        n, nb, dl = len(e["src"]), len(e["bytes"]), self.eng.download
        assert n <= 2000
        held, druns = self.upload(rr)
        po = self.eng.runs_merge_plan_dev(druns, n_ref, chunk_bytes)
        nc = int(po.n_chunks)
        res = {"status": OK, "err_run": int(po.err_run), "err_record": int(po.err_record), "err_kind": int(po.err_kind), "n_records": int(po.n_records),
               "n_bytes": int(po.n_bytes), "n_mapped": int(po.n_mapped), "n_chunks": nc, "src": dl(po.src, np.uint32, n), "key": dl(po.key, np.uint64, n),
               "record_off": dl(po.record_off, np.uint64, n + 1), "chunk_first": np.ctypeslib.as_array(po.chunk_first, (nc + 1,)).copy(),
               "chunk_off": np.ctypeslib.as_array(po.chunk_off, (nc + 1,)).copy()}
        check_plan(res, e, what)
        assert po.plan_ms > 0
        order = list(range(nc)) + [nc - 1, 0]  # and out of order, twice
        emits = []
        for c in order:
            co = self.eng.runs_merge_emit_dev(c)
            emits.append({"status": OK, "first": int(co.first_record), "n_records": int(co.n_records),
                          "record_off": dl(co.record_off, np.uint64, int(co.n_records) + 1), "bytes": dl(co.bytes, np.uint8, int(co.n_bytes)).tobytes()})
            assert co.emit_ms > 0
        res["emits"] = emits
        check_emits(res, e, order, what)
        assert b"".join(g["bytes"] for g in emits[:nc]) == e["bytes"], what
        with pytest.raises(api.PortelloError) as err:
            self.eng.runs_merge_emit_dev(nc)
        assert err.value.status == INVALID
        # plo_records_sort_dev over the concatenation on the same device: byte for byte
        data, off = sx.concat([x for r in runs for x in r])
        craw = self.torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(self.dev)
        coff = self.torch.from_numpy(off.view(np.int64)).to(self.dev)
        self.torch.cuda.synchronize()
        so = self.eng.records_sort_dev(craw.data_ptr(), len(data), n, coff.data_ptr(), n_ref)
        assert dl(so.bytes, np.uint8, nb).tobytes() == e["bytes"] and np.array_equal(dl(so.perm, np.uint32, n), e["src"]), what
        assert np.array_equal(dl(so.record_off, np.uint64, n + 1), e["record_off"]) and int(so.n_mapped) == e["n_mapped"], what
        for (d0, o0), (p, _, _, po_) in zip([x for x in rr if len(x[1]) > 1], [x for x in druns if x[2]]):  # the runs are unchanged
            assert dl(p, np.uint8, len(d0)).tobytes() == d0 and np.array_equal(dl(po_, np.uint64, len(o0)), o0), what
        del held

    def refuse(self, rr, n_bytes, want):
        held, druns = self.upload(rr)
        if n_bytes is not None:
            druns = [(p, nb, n, o) for (p, _, n, o), nb in zip(druns, n_bytes)]
        with pytest.raises(api.PortelloError, match=r"run %d record %d .*kind %d" % want) as e:
            self.eng.runs_merge_plan_dev(druns, 25, 4096)
        assert e.value.status == INVALID and (e.value.err_run, e.value.err_record, e.value.err_kind) == want
        with pytest.raises(api.PortelloError) as e:  # a refused plan is no plan
            self.eng.runs_merge_emit_dev(0)
        assert e.value.status == INVALID

    def close(self):
        self.eng.close()
        self.index.close()


@pytest.mark.gpu
def test_device_merge_against_the_expectation_and_the_sort():
    """the C ABI on the device against merge_expect and against plo_records_sort_dev over the concatenation, one context for all"""
    dm = DevMerger()
    with pytest.raises(api.PortelloError) as e:
        dm.eng.runs_merge_emit_dev(0)  # no plan yet
    assert e.value.status == INVALID
    tie = lambda r: in_order(random_records(257 + r, 3, 500 + r, pos_span=12), 3)  # noqa: E731
    dm.check([tie(r) for r in range(5)], 3, 4096, "5 runs of about 257 records with ties")
    dm.check([sorted_run(300, 25, 511), [rec(0, 20, 0, b"one")], []], 25, 4096, "runs of 300 / 1 / 0 records")
    big = [rec(0, 15 + i, 0, b"big%d" % i, np.random.default_rng(i).integers(0, 256, 40_000, dtype=np.uint8).tobytes()) for i in range(2)]
    dm.check([in_order(random_records(80, 3, 520) + big[:1], 3), sorted_run(60, 3, 521), in_order(random_records(50, 3, 522) + big[1:], 3)], 3, 16384, "two 40 kB records")
    r = refusals()
    for name in ("kind 6 in a middle run", "kind 3 in the last run"):
        dm.refuse(*r[name])
        dm.check(hand_case(), 2, 80, "after " + name)
    for bad in (dict(chunk_bytes=0), dict(n_runs=mx.MAX_RUNS + 1)):
        with pytest.raises(api.PortelloError) as e:
            dm.eng.runs_merge_plan_dev([(0, 0, 0, 0)] * bad.get("n_runs", 1), 25, bad.get("chunk_bytes", 4096))
        assert e.value.status == INVALID
    po = dm.eng.runs_merge_plan_dev([], 25, 4096)
    assert int(po.n_records) == int(po.n_chunks) == 0 and list(dm.eng.download(po.record_off, np.uint64, 1)) == [0]
    dm.close()


@pytest.fixture(scope="module")
def window_bam(tmp_path_factory):
    from portello_amd import synth

    d = tmp_path_factory.mktemp("mergedev")
    w = synth.generate(synth.config("tiny", n_reads=450, seed=418, split_read_frac=0.3, sorted_reads=True))
    path = str(d / "reads.bam")
    meta = bamsynth.write_read_bam(w, path, level=6, n_unmapped=4)
    return w, path, meta


def record_stream(paths, tmp, name):
    """the inflated record stream of bam.merge_runs over `paths`"""
    out = os.path.join(tmp, name)
    bam.merge_runs(paths, out)
    return bamcheck.read_bam(out)


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [dict(), dict(device_bgzf=True, level=1)], ids=["plain", "device_bgzf"])
def test_bam_to_bam_run_windows(window_bam, tmp_path, extra):
    """run_bam_to_bam(sorted_runs=True, index_runs=True, run_windows=1 / 2 / 0, and a budget between one and two windows): every run is a
    complete sorted BAM with the runs' header, the merge of each configuration's runs is the record stream of run_windows=1's, with 0 the
    one run stands at out_path and IS that stream, every .bai answers region queries as a brute-force scan does, run_groups is the split"""
    import index_expect as ix
    import test_index_dev as tid
    from portello_amd import pipeline

    w, path, meta = window_bam
    ixd = w.index_data()
    index = api.Index(ixd, 0)
    cn, rn = meta["contig_names"], bamsynth.ref_names(w)
    lens = [len(s) for s in ixd.chrom_seq]
    kw = dict(window_reads=90, ramp=False, n_workers=2, io_threads=4, device_records=True, device_batch=True, sorted_runs=True, index_runs=True, **extra)
    hdr = bam.output_header(rn, lens, sort_order="coordinate")
    stats, streams = {}, {}
    for name, more in (("k1", dict(run_windows=1)), ("k2", dict(run_windows=2)), ("k0", dict(run_windows=0)), ("k2_small_chunks", dict(run_windows=2, run_chunk_bytes=20_000))):
        (tmp_path / name).mkdir()
        st = stats[name] = pipeline.run_bam_to_bam(path, str(tmp_path / name / "lifted.bam"), index, ixd, cn, rn, lens, **more, **kw)
        assert st.out_paths == sorted(st.out_paths) and st.index_paths == [p + ".bai" for p in st.out_paths]
        assert sorted(os.listdir(str(tmp_path / name))) == sorted(os.path.basename(p) for p in st.out_paths + st.index_paths)
        for p in st.out_paths:
            text, refs, recs = bamcheck.read_bam(p)  # (bamcheck accepts the run)
            assert text == hdr and refs == list(zip(rn, lens)) and recs
            keys = [sx.key_of(r, len(rn)) for r in recs]
            assert keys == sorted(keys)
            blob, bai_blob = open(p, "rb").read(), open(p + ".bai", "rb").read()
            assert bai_blob == ix.expected_bai(blob), p
            tid.check_bam_queries(blob, bai_blob, lens, n=25)
        streams[name] = record_stream(st.out_paths, str(tmp_path), name + ".merged.bam")
    n_win = len(stats["k1"].out_paths)
    assert n_win >= 5 and stats["k1"].run_groups == [1] * n_win and stats["k1"].merge_plan_device_ms == 0
    assert [os.path.basename(p) for p in stats["k1"].out_paths] == ["lifted.r00w%06d.bam" % k for k in range(n_win)]
    for name in ("k2", "k0", "k2_small_chunks"):
        assert streams[name] == streams["k1"], name
        assert stats[name].records_out == stats["k1"].records_out == len(streams["k1"][2]) and stats[name].reads == stats["k1"].reads
        assert stats[name].merge_plan_device_ms > 0 and stats[name].merge_emit_device_ms > 0 and stats[name].index_device_ms > 0
    for name in ("k2", "k2_small_chunks"):
        assert stats[name].run_groups == [2] * (n_win // 2) + [1] * (n_win % 2)
        assert [os.path.basename(p) for p in stats[name].out_paths] == ["lifted.r00m%06d.bam" % k for k in range((n_win + 1) // 2)]
    # 0: exactly one run, at out_path; its record stream is that merge's without any merging, its header the runs'
    st0 = stats["k0"]
    assert st0.out_paths == [str(tmp_path / "k0" / "lifted.bam")] and st0.run_groups == [n_win]
    assert bamcheck.read_bam(st0.out_paths[0]) == streams["k1"]
    # a budget between one and two windows' sizes: groups of one window each
    sizes = [sum(len(r) for r in bamcheck.read_bam(p)[2]) for p in stats["k1"].out_paths]
    one, two = max(sizes), min(a + b for a, b in zip(sizes, sizes[1:]))
    assert one < two, sizes
    (tmp_path / "budget").mkdir()
    stb = pipeline.run_bam_to_bam(path, str(tmp_path / "budget" / "lifted.bam"), index, ixd, cn, rn, lens, run_windows=0, run_budget_bytes=(one + two) // 2, **kw)
    assert stb.run_groups == [1] * n_win and [os.path.basename(p) for p in stb.out_paths] == ["lifted.r00m%06d.bam" % k for k in range(n_win)]
    assert [bamcheck.read_bam(p)[2] for p in stb.out_paths] == [bamcheck.read_bam(p)[2] for p in stats["k1"].out_paths]
    index.close()


def test_abi_structs():
    """the ctypes structs have the header's layout on LP64 (engine.hip asserts plo_merge_run against the device's MergeRun)"""
    import ctypes as C

    assert C.sizeof(abi.PloMergeRun) == 32 and abi.PloMergeRun.record_off.offset == 24
    assert C.sizeof(abi.PloMergeIn) == 24 and abi.PloMergeIn.chunk_bytes.offset == 16
    assert C.sizeof(abi.PloMergeOut) == 80 and abi.PloMergeOut.chunk_first.offset == 48 and abi.PloMergeOut.plan_ms.offset == 76
    assert C.sizeof(abi.PloMergeChunkOut) == 40 and abi.PloMergeChunkOut.record_off.offset == 24 and abi.PloMergeChunkOut.emit_ms.offset == 32
