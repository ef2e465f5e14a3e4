"""The liftover stage -- a read's CIGAR composed through a contig segment's block map: lane_tile (lane_core.hpp), wave B of the streaming
kernel (lane_stream.hpp), the scan formulation (lift_core.hpp), and the window search of build_item_desc (enumerate.hpp) in front of them --
on hand-built block maps at the staging and map edges (tests/liftover_cases.py).

Voices: the hand-written expectations of family P, a plain-Python restatement written from the Rust text (tests/liftover_expect.py), the C
oracle, every emulator route, and the card.  The restatement and the hand values speak for the stage set STRAND | LIFTOVER, where the
catalogue's (start, CIGAR) reach the liftover as written; under STAGES_ALL the oracle is the expectation.

The streaming kernel takes STAGES_ALL only (other stage sets go to the window route, in the engine and in the emulator's harness): this is
the one place that says so, ROUTES below carries it as `all_only`.

The staging rule restated here (predict_split) is coupled to LANE_KVS = 128 (lane_core.hpp) and to lane_region_gap's two ops per key
(enumerate.hpp, PLO_LANE_GAP_HALVES = 4): a change of either moves the borders the S cases stand on, and this file with them."""
import json
import os

import numpy as np
import pytest

import emu_lib
import emu_liftover_lib
import liftover_cases as lc
import liftover_expect as lx
from portello_amd import abi, api
from portello_amd import cigar as cg
from variants import HEAVY_VARIANTS

IX = lc.INDEX
LANE_KVS = 128      # lane_core.hpp
LANE_MAX_W = 192    # the engine's default weight limit of the light classes
STAGE_SETS = (abi.STAGES_ALL, lc.STRAND_LIFT)

# emulator routes: name -> (arguments of emu_lib.liftover_batch, PLO_EMU_H16, all_only)
ROUTES = {
    "scan_tiles": (dict(), "0", False),
    "scan_big": (dict(big_thresh=8), "0", False),
    "scan_mid8": (dict(big_thresh=40, mid_waves=8), "0", False),
    "lanes32": (dict(lane_max_w=LANE_MAX_W), "0", False),
    "lanes16": (dict(lane_max_w=LANE_MAX_W), "1", False),
    "lanes32_seed": (dict(lane_max_w=LANE_MAX_W, order_seed=4), "0", False),
    "window64": (dict(lane_max_w=lc.HEAVY_MAX_W, lane_heavy_per=64), "0", False),
    "window5": (dict(lane_max_w=lc.HEAVY_MAX_W, lane_heavy_per=5, order_seed=8), "0", False),
    # (a team of the harness is 64 lanes wide whatever the count: 1024 = one team for all items of a class, whose lanes take second items;
    # 64 = teams of 64 items.  Teams of 5 items cost a whole emulated team each -- 47 s for the catalogue -- and run on the card only.)
    "stream1": (dict(lane_max_w=lc.HEAVY_MAX_W, lane_heavy_per=1024, lane_stream=1), "0", True),
    "stream2": (dict(lane_max_w=lc.HEAVY_MAX_W, lane_heavy_per=1024, lane_stream=2), "0", True),
    "stream1_seed": (dict(lane_max_w=lc.HEAVY_MAX_W, lane_heavy_per=64, lane_stream=1, order_seed=5), "0", True),
    "stream2_seed": (dict(lane_max_w=lc.HEAVY_MAX_W, lane_heavy_per=1024, lane_stream=2, order_seed=7), "0", True),
}


@pytest.fixture(scope="module")
def cases():
    return lc.all_cases(LANE_KVS)


@pytest.fixture(scope="module")
def refs(cases, oracle):
    """{(case name, stages): the oracle's result}: computed once, shared by the CPU and the GPU legs, never changed"""
    return {(c.name, st): oracle.liftover_batch(IX, c.batch, st, 1) for c in cases for st in STAGE_SETS}


_RUNS = {}


def _emu(route, c, stages):
    """one emulator run per (route, case, stage set), shared by the tests: (rc, result, counters, staging counters, descriptors)"""
    key = (route, c.name, stages)
    if key not in _RUNS:
        kw, h16, _ = ROUTES[route]
        old = os.environ.get("PLO_EMU_H16")
        os.environ["PLO_EMU_H16"] = h16
        try:
            rc, res, cnt = emu_lib.liftover_batch(IX, c.batch, stages=stages, **kw)
        finally:
            if old is None:
                del os.environ["PLO_EMU_H16"]
            else:
                os.environ["PLO_EMU_H16"] = old
        _RUNS[key] = (rc, res, cnt, emu_lib.kv_stats(), emu_lib.last_windows(res.n_items))
    return _RUNS[key]


_RESTATED = {}


def _restated(c, stages=lc.STRAND_LIFT):
    if (c.name, stages) not in _RESTATED:
        _RESTATED[(c.name, stages)] = _restate(c, stages)
    return _RESTATED[(c.name, stages)]


def _restate(c, stages):
    """per item (status, pos, CIGAR, (w0, w1), keys) by the restatement, in the restated item order"""
    return [lx.lift_item(IX, c.batch, s, g, stages) for s, g in lx.item_list(IX, c.batch)]


def _rows(res):
    return [(int(res.item_status[i]), int(res.item_ref_pos[i]), lx.fmt(lx.from_words(res.item_cigar(i)))) if int(res.item_status[i]) in (0, 2) else
            (int(res.item_status[i]), None, None) for i in range(res.n_items)]


# ---- the restatement and the hand values ---------------------------------------------------------------------------------------------

def test_restatement_on_the_reference_vectors(golden):
    """every liftover and tree-map vector of the Rust unit tests"""
    for v in golden["liftover"]:
        keys, vals = lx.tree_map(v["map"]["pos"], lx.parse(v["map"]["cigar"])) if v["map"] else ([], [])
        got, _ = lx.liftover_read_alignment(keys, vals, v["start"], lx.parse(v["cigar"]))
        want = None if v["expect"] is None else (v["expect"]["pos"], v["expect"]["cigar"])
        assert (None if got is None else (got[0], lx.fmt(got[1]))) == want, v["id"]
    for v in golden["tree_map"]:
        keys, vals = lx.tree_map(v["pos"], lx.parse(v["cigar"]), v["ignore_hard_clip"])
        for q, want in v["lookups"]:
            assert lx.get_ref_pos(keys, vals, q) == want, v["id"]
        i0, i1 = lx.get_ref_range(keys, v["range"]["a"], v["range"]["b"])
        assert [[keys[i], vals[i]] for i in range(i0, i1)] == v["range"]["expect"], v["id"]
    v = golden["compress"][0]
    assert lx.fmt(lx.compress_cigar(lx.parse(v["cigar"]))) == v["expect"]
    v = golden["edge_cleanup"][0]
    ops = lx.parse(v["cigar"])
    assert lx.clean_up_cigar_edge_indels(ops) == v["expect_shift"] and lx.fmt(ops) == v["expect"]


def test_restatement_on_the_hand_vectors():
    """tests/golden/liftover_vectors.json holds the catalogue's hand-written expectations, and the restatement gives every one"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "liftover_vectors.json")) as fh:
        g = json.load(fh)
    assert g == json.loads(json.dumps(lc.golden_vectors()))
    assert len(g["liftover"]) >= 50 and len({v["id"] for v in g["liftover"]}) == len(g["liftover"])
    for v in g["liftover"]:
        m = g["maps"][v["map"]]
        keys, vals = lx.tree_map(m["pos"], lx.parse(m["cigar"]))
        assert 0 <= len(keys) <= 45, v["id"]
        got, win = lx.liftover_read_alignment(keys, vals, v["start"], lx.parse(v["cigar"]))
        want = None if v["expect"] is None else (v["expect"]["pos"], v["expect"]["cigar"])
        assert (None if got is None else (got[0], lx.fmt(got[1]))) == want, (v["id"], v["why"])
        # the union of the ops' range queries is the query of the whole span: what build_item_desc searches for
        assert win == lx.get_ref_range(keys, v["start"], v["start"] + lx.ref_span(lx.parse(v["cigar"]))), v["id"]
    # the keys the catalogue's comments name
    assert lx.tree_map(lc.MAPS["J"][0], lx.parse(lc.MAPS["J"][1])) == ([0, 10, 20, 30], [1000, 1011, 11021, None])
    assert lx.tree_map(lc.MAPS["U"][0], lx.parse(lc.MAPS["U"][1])) == ([5, 15, 20, 30, 33, 43, 49, 59], [2000, None, 2010, None, 2022, None, 2036, None])
    assert lx.tree_map(lc.MAPS["Z"][0], lx.parse(lc.MAPS["Z"][1])) == ([], [])
    assert len(lx.tree_map(lc.MAPS["A"][0], lx.parse(lc.MAPS["A"][1]))[0]) == 300 and len(lx.tree_map(lc.MAPS["B"][0], lx.parse(lc.MAPS["B"][1]))[0]) == 40
    assert lc.KV0[("B", 1)] == lc.KV0[("A", 1)] + 300 and lc.KV0[("B", 0)] == lc.KV0[("A", 0)] + 300 and lc.KV0[("B", 0)] + 40 == lc.N_KV


def test_hand_values_restatement_and_oracle_agree(cases, refs, oracle):
    """STRAND | LIFTOVER: hand value == restatement == oracle.liftover_read_alignment == oracle.liftover_batch for every item of every case
    (family S has no hand values: restatement against the two oracle entries)"""
    n_hand = 0
    for c in cases:
        ref = refs[(c.name, lc.STRAND_LIFT)]
        items = lx.item_list(IX, c.batch)
        assert list(zip(ref.item_seg.tolist(), ref.item_cseg.tolist())) == items, c.name
        rows = _rows(ref)
        for i, ((s, g), (st, pos, ops, _, _)) in enumerate(zip(items, _restated(c))):
            got = (st, pos, None if ops is None else lx.fmt(ops))
            assert got == rows[i], (c.name, i, got, rows[i])
            if c.expected is not None:
                e = c.expected[i]
                assert got == ((lx.NO_LIFTOVER, None, None) if e is None else (lx.LIFTED, e[0], e[1])), (c.name, c.names[i])
                n_hand += 1
            # the pure function of the oracle on the restated map
            gs = int(IX.contig_seg_off[int(c.batch.seg_contig[s])]) + g
            keys, vals = lx.segment_map(IX, gs)
            o = int(c.batch.seg_cigar_off[s])
            words = c.batch.cigar[o:int(c.batch.seg_cigar_off[s + 1])]
            p1 = int(c.batch.seg_pos[s])
            if not int(IX.seg_is_fwd_strand[gs]):
                p1, words = int(IX.contig_len[int(c.batch.seg_contig[s])]) - (p1 + cg.ref_len(words)), words[::-1]
            r = oracle.liftover_read_alignment(np.array(keys, np.uint64), np.array([abi.NONE_VAL if v is None else v for v in vals], np.int64), p1, words)
            assert (None if r is None else (r[0], cg.decode(r[1]))) == (None if pos is None else (pos, got[2])), (c.name, i)
        # with the length check: every read is as long as its CIGAR's read span, so nothing changes
        assert [(r[0], r[1]) for r in _restated(c, lc.STRAND_LIFT | abi.STAGE_LENCHECK)] == [(r[0], r[1]) for r in rows], c.name
    assert n_hand == 2 * len(lc.P)


def test_the_reverse_contig_shifts_in_front_of_the_liftover(cases, refs):
    """family P on the reverse contigs under STAGES_ALL: the left shift strips the leading D of shift_past_*, the start moves past one / two
    keys and the result differs from the unshifted one (the oracle's, which the emulator routes below must reproduce)"""
    by = {c.name: c for c in cases}
    for name, start in (("shift_past_one_key", 5010), ("shift_past_two_keys", 5012)):
        i = lc.P_NAMES.index(name)
        rev, fwd = _rows(refs[("P_rev", abi.STAGES_ALL)])[i], _rows(refs[("P_fwd", abi.STAGES_ALL)])[i]
        e = by["P_rev"].expected[i]
        assert rev == (0, start, lc._k(5)), (name, rev)   # the D is gone before the lift: no jump deletion in front, no lead shift
        assert fwd == (0, e[0], e[1]), (name, fwd)        # the forward contig has no shift stage: as written


# ---- emulator routes -------------------------------------------------------------------------------------------------------------------

def _runs_on(route, stages):
    return not (ROUTES[route][2] and stages != abi.STAGES_ALL)


@pytest.mark.parametrize("route", list(ROUTES))
def test_emulator_routes(cases, refs, route):
    """every case through one route, item by item against the oracle, both stage sets (the streaming routes: STAGES_ALL); the case with the
    most output ops per key is lifted by the lane kernel itself (no retry), and so is every other item of the catalogue"""
    n_run = 0
    for c in cases:
        ran = False
        for stages in STAGE_SETS:
            if not _runs_on(route, stages):
                continue
            rc, res, cnt, _, _ = _emu(route, c, stages)
            assert rc == 0, (c.name, stages)
            assert res.canonical() == refs[(c.name, stages)].canonical(), (c.name, stages, route)
            if route.startswith(("lanes", "window", "stream")):
                assert cnt[emu_lib.CNT_NRETRY] == 0, (c.name, stages, route, "items on the retry list", cnt[emu_lib.CNT_NRETRY])
                if not c.heavy and not c.stream and route.startswith("lanes"):
                    assert cnt[emu_lib.CNT_LANE_ITEMS] == res.n_items, (c.name, "light items", cnt[emu_lib.CNT_LANE_ITEMS])
            ran = True
        n_run += ran
    assert 10 * n_run >= 9 * len(cases), (route, n_run, len(cases))


# ---- proof that the edges are reached ---------------------------------------------------------------------------------------------------

def n_merged(words):
    """ops once neighbouring M = X are one (what lane_tile's LOAD stores for stage sets with the liftover)"""
    n, prev = 0, False
    for w in words:
        m = (int(w) & 15) in (0, 7, 8)
        n += 0 if (m and prev) else 1
        prev = m
    return n


_WINDOWS = {}


def windows(c):
    """per item, restated: absolute (W0, W1, kv0, kv1), the region's dwords and whether the contig segment is reverse"""
    if c.name in _WINDOWS:
        return _WINDOWS[c.name]
    out = []
    for (s, g), (_, _, _, (w0, w1), nk) in zip(lx.item_list(IX, c.batch), _restated(c)):
        m, f = lc._ORDER[int(c.batch.seg_contig[s])]
        kv0 = lc.KV0[(m, f)]
        words = c.batch.cigar[int(c.batch.seg_cigar_off[s]):int(c.batch.seg_cigar_off[s + 1])]
        region = n_merged(words) + 2 * max(0, w1 - w0) + 2  # enumerate.hpp lane_region_dwords: n + lane_region_gap + LANE_SLACK
        out.append((kv0 + w0, kv0 + w1, kv0, kv0 + nk, region, not f))
    _WINDOWS[c.name] = out
    return out


def predict_split(c, stages, max_w, heavy_per, kvs=LANE_KVS):
    """The staging rule of lane_tile restated from the restated windows (COUPLED TO LANE_KVS): a group stages `cnt` = min(top - base, kvs)
    entries from base = its lowest W0, top = its highest need_hi, need_hi = min(kv1, W1 + 2); an item is staged when need_hi <= base + cnt;
    a group whose items are all staged runs the all-staged loop, any other the mixed loop, where every unstaged item fetches the entries
    [W0, need_hi) from global memory.  Groups: the class order (forward / shifted, light then heavy), 64 consecutive light items, `heavy_per`
    consecutive heavy ones.  -> (all-staged groups, mixed groups, entries from global memory)"""
    w = windows(c)
    cls = [(1 if (stages & abi.STAGE_LSHIFT) and rev else 0) + (2 if region > max_w else 0) for (_, _, _, _, region, rev) in w]
    all_lds = mixed = fetched = 0
    for k in range(4):
        members = [w[i] for i in range(len(w)) if cls[i] == k]
        per = 64 if k < 2 else heavy_per
        if k >= 2 and not heavy_per:
            continue
        for lo in range(0, len(members), per):
            grp = members[lo:lo + per]
            need = [min(kv1, w1 + 2) for (_, w1, _, kv1, _, _) in grp]
            base, top = min(g[0] for g in grp), max(need)
            cnt = max(0, min(top - base, kvs))
            out = [(g[0], nh) for g, nh in zip(grp, need) if nh > base + cnt]
            all_lds, mixed = all_lds + (not out), mixed + bool(out)
            fetched += sum(max(0, nh - w0) for w0, nh in out)
    return all_lds, mixed, fetched


# what the S cases are there for, by hand: (all-staged groups, mixed groups, entries from global memory) of the light routes
BY_HAND = {"S_near63_far1_m1": (1, 0, 0), "S_near63_far1_eq": (1, 0, 0), "S_near63_far1_p1": (0, 1, 3),
           "S_near1_far63_m1": (1, 0, 0), "S_near1_far63_eq": (1, 0, 0), "S_near1_far63_p1": (0, 1, 3),
           "S_nearA_farB_m1": (1, 0, 0), "S_nearA_farB_eq": (1, 0, 0), "S_nearA_farB_p1": (0, 1, 3),
           "S_map_end_A": (1, 0, 0), "S_map_end_B": (1, 0, 0)}


@pytest.mark.parametrize("route", ["lanes32", "lanes16", "lanes32_seed"])
def test_light_groups_split_as_predicted(cases, route):
    """the emulator's counters (EmuKvStats, PLO_EMULATOR only) against the restated rule for every case, and against the hand-written split
    for the 127 / 128 / 129 cases: 128 is the last staged entry, 129 the first item that is not staged"""
    seen = set()
    for c in cases:
        if c.heavy or c.stream:
            continue
        for stages in STAGE_SETS:
            rc, res, _, st, _ = _emu(route, c, stages)
            assert rc == 0
            got = (st["all_lds"], st["mixed"], st["global_kv"])
            assert got == predict_split(c, stages, LANE_MAX_W, 0), (c.name, stages, got)
            hand = BY_HAND.get(c.name.rsplit("_", 1)[0])
            if hand is not None:
                assert got == hand, (c.name, stages, got, hand)
                seen.add(c.name)
            if c.light:
                assert st["all_lds"] + st["mixed"] == 1, (c.name, "one group")
    assert len(seen) == 2 * len(BY_HAND)


@pytest.mark.parametrize("per", [64, 5])
def test_heavy_groups_split_as_predicted(cases, per):
    """the window route: a single item that needs 126 .. 128 entries is staged, one that needs 129 or 200 fetches all of them from global
    memory, alone and beside 63 short items"""
    n = 0
    for c in cases:
        if c.stream:
            continue
        for stages in STAGE_SETS:
            rc, res, cnt, st, _ = _emu(f"window{per}", c, stages)
            assert rc == 0
            got = (st["all_lds"], st["mixed"], st["global_kv"])
            assert got == predict_split(c, stages, lc.HEAVY_MAX_W, per), (c.name, stages, got)
            if c.heavy:
                assert cnt[emu_lib.CNT_LANE_ITEMS] == 0, c.name
                need = int(c.name.split("need")[1].split("_")[0])
                n_groups = 1 if "alone" in c.name else -(-64 // per)
                assert got == ((n_groups, 0, 0) if need <= LANE_KVS else (n_groups - 1, 1, need)), (c.name, got)  # (by hand)
                n += 1
    assert n == 40


def test_stream_restages_under_a_running_item(cases, refs):
    """the streaming kernel stages again whenever items start: the long item's kv_lds flips off when its neighbours restart below it and on
    again when they restart above it, in the middle of its walk, and the result is the oracle's"""
    n = 0
    for c in cases:
        if not c.stream:
            continue
        for route in ("stream1", "stream2", "stream2_seed"):
            rc, res, cnt, st, _ = _emu(route, c, abi.STAGES_ALL)
            assert rc == 0 and res.canonical() == refs[(c.name, abi.STAGES_ALL)].canonical(), (c.name, route)
            assert st["s_mid"] >= 2 and st["s_flip_off"] >= 1 and st["s_flip_on"] >= 1 and st["s_global_kv"] > 0, (c.name, route, st)
            assert cnt[emu_lib.CNT_NRETRY] == 0, (c.name, route)
            n += 1
    assert n == 6


def test_descriptors_hold_the_restated_windows(cases):
    """w0 / w1 / kv0 / kv1 as the emulator's build_item_desc stores them against the restatement's window for every item of every case, and the
    region's dwords against the restated bound (two ops per key of the window)"""
    for c in cases:
        for stages in STAGE_SETS:
            rc, res, _, _, d = _emu("lanes32", c, stages)
            assert rc == 0
            for i, (w0, w1, kv0, kv1, region, rev) in enumerate(windows(c)):
                got = tuple(int(d[k][i]) for k in ("w0", "w1", "kv0", "kv1", "region"))
                assert got == (w0, w1, kv0, kv1, region), (c.name, stages, i, got, (w0, w1, kv0, kv1, region))
                assert int(d["cls"][i]) == (1 if (stages & abi.STAGE_LSHIFT) and rev else 0) + (2 if region > LANE_MAX_W else 0), (c.name, i)
    # the case with the most output ops per key attains the gap exactly: 68 ops out of a window of 34 keys
    p = [c for c in cases if c.name == "P_fwd"][0]
    i = lc.P_NAMES.index("most_ops_per_key")
    w0, w1, _, _, region, _ = windows(p)[i]
    assert w1 - w0 == 34 and region == 1 + 68 + 2 and len(lx.parse(p.expected[i][1])) == 68


def test_asan_program(tmp_path, cases, refs):
    """the whole catalogue through lane_tile (32- and 16-bit), the window route and the streaming route (STAGES_ALL) in a host-only program,
    every array in a heap block of its exact size, AddressSanitizer and UBSan on: clean exit, and every result the oracle's.  (STRAND |
    LIFTOVER too for family P and the map-end cases, whose cursors differ without the shift stage.)"""
    todo = [(c, st) for c in cases for st in STAGE_SETS if st == abi.STAGES_ALL or c.family == "P" or "map_end" in c.name]
    rc, err, res = emu_liftover_lib.run_asan(IX, [(c.batch, st) for c, st in todo], tmp_path, lc.HEAVY_MAX_W)
    assert rc == 0, err[-3000:]
    for (c, st), modes in zip(todo, res):
        assert len(modes) == (len(emu_liftover_lib.MODES) if st == abi.STAGES_ALL else 3)
        for name, (erc, n_retry, got) in zip(emu_liftover_lib.MODES, modes):
            assert erc == 0 and n_retry == 0, (c.name, st, name, erc, n_retry)
            assert got.canonical() == refs[(c.name, st)].canonical(), (c.name, st, name)


# ---- GPU legs ---------------------------------------------------------------------------------------------------------------------------

_MID = {"PLO_WINDOW": "256", "PLO_BIG_THRESH": "176", "PLO_CAP": "320"}  # (test_synthetic_indel_dense_large_item_kernels' geometry)
_HEAVY = {"PLO_LANE_HEAVY_MIN": "0", "PLO_LANE_MAX_W": str(lc.HEAVY_MAX_W)}
# name -> (environment, kvs the S cases are generated from, weight limit of the light classes, kind of the expected plo_timing counts)
ENVS = {
    "default": ({}, 128, LANE_MAX_W, "tiles"),
    "h16_kvs64": ({"PLO_LANE_H16": "1", "PLO_LANE_KVS": "64"}, 64, LANE_MAX_W, "tiles"),
    "h16_kvs512": ({"PLO_LANE_H16": "1", "PLO_LANE_KVS": "512"}, 128, LANE_MAX_W, "tiles"),
    "kvs64": ({"PLO_LANE_KVS": "64"}, 64, LANE_MAX_W, "tiles"),  # 32-bit regions: the S borders stand at 63 / 64 / 65
    "mid16": ({**_MID, "PLO_MID_WAVES": "16"}, 128, LANE_MAX_W, "mid"),
    "mid8": ({**_MID, "PLO_MID_WAVES": "8"}, 128, LANE_MAX_W, "mid"),
    "mid8_cap512": ({**_MID, "PLO_MID_WAVES": "8", "PLO_MID_CAP": "512"}, 128, LANE_MAX_W, "mid_cap"),
    "big": ({**_MID, "PLO_MID_WAVES": "0"}, 128, LANE_MAX_W, "big"),
}
for _v, _e in HEAVY_VARIANTS.items():
    for _per in ("64", "5") + (("1024",) if _v == "stream" else ()):  # (1024: one team holds the restaging case, lanes take second items)
        ENVS[f"{_v}_per{_per}"] = ({**_e, **_HEAVY, "PLO_LANE_HEAVY_PER": _per}, 128, lc.HEAVY_MAX_W, "heavy")


@pytest.fixture(scope="module")
def card():
    index = api.Index(IX)
    yield index
    index.close()


def _timing_row(t):
    return {k: int(getattr(t, k)) for k in ("n_items", "n_lane_items", "n_heavy_lane_items", "n_retry_items", "n_mid_items", "n_big_items", "host_syncs")}


@pytest.mark.gpu
@pytest.mark.parametrize("env", list(ENVS))
def test_catalogue_on_the_card(card, oracle, refs, env, monkeypatch):
    """the whole catalogue, one fresh context per environment (a context reads its environment when it is created, the heavy switches at
    every call), item by item against the oracle; plo_timing proves the route.  Expected counts, per call:
      n_lane_items        the items whose restated region (ops + two per key of the window + 2) is within the weight limit
      n_retry_items       0 where the lane kernels take every item: every region holds its item (the bound of two ops per key is
                          attained, not exceeded)
      tiles (default)     the others go to the tile kernels: n_heavy_lane_items 0 (below the lane kernels' batch size), handed on at most all
      heavy               PLO_LANE_HEAVY_MIN=0, PLO_LANE_MAX_W=4: the others ALL go to the heavy lane kernel, none to mid / big
      mid / big           PLO_BIG_THRESH=176: a heavy item weighs ops + 2 (keys + 1) -- 243 (120M) .. 399 (198M), so each is handed to the
                          workgroup-per-item kernel (PLO_MID_WAVES=0: to the one-wave kernel); PLO_MID_CAP=512 hands on what weighs more than
                          (512 - 64) 4 / 5 = 358, the 198M item alone"""
    environ, kvs, max_w, kind = ENVS[env]
    for k, v in environ.items():
        monkeypatch.setenv(k, v)
    eng = api.Engine(card)
    n_calls = 0
    for c in lc.all_cases(kvs):
        for stages in STAGE_SETS:
            ref = refs.get((c.name, stages)) or oracle.liftover_batch(IX, c.batch, stages, 1)
            got = eng.liftover_batch(c.batch, stages)
            t = _timing_row(eng.timing())
            print(env, c.name, stages, t)
            assert got.canonical() == ref.canonical(), (env, c.name, stages)
            regions = [w[4] for w in windows(c)]
            light = sum(r <= max_w for r in regions)
            heavy = len(regions) - light
            assert t["n_items"] == len(regions) and t["n_lane_items"] == light, (env, c.name, stages, t, light)
            if heavy == 0 or kind == "heavy":  # (what the tile kernels re-run when a slice overflows is their geometry's affair)
                assert t["n_retry_items"] == 0, (env, c.name, stages, t)
            if kind == "heavy":
                assert (t["n_heavy_lane_items"], t["n_mid_items"], t["n_big_items"]) == (heavy, 0, 0), (env, c.name, stages, t, heavy)
            else:
                assert t["n_heavy_lane_items"] == 0, (env, c.name, stages, t)
                if kind == "tiles":
                    assert t["n_mid_items"] + t["n_big_items"] <= heavy, (env, c.name, stages, t, heavy)
                else:
                    assert heavy <= 1  # (the long item of a heavy or restaging case)
                    over = int(c.heavy and "need200" in c.name)
                    want = {"mid": (heavy, 0), "mid_cap": (heavy - over, over), "big": (0, heavy)}[kind]  # (n_mid_items: what that kernel kept)
                    assert (t["n_mid_items"], t["n_big_items"]) == want, (env, c.name, stages, t, want)
            n_calls += 1
    eng.close()
    assert n_calls == 2 * len(lc.all_cases(kvs))


@pytest.mark.gpu
@pytest.mark.parametrize("kvs", [128, 64])
def test_light_groups_careful_then_armed(card, oracle, kvs, monkeypatch):
    """the one-round-trip path: each light S group twice on one context -- the first call careful, the second armed (one host round trip) --
    with the same result, the oracle's"""
    from dev_arrays import DevArrays
    from portello_amd import devbatch

    monkeypatch.setenv("PLO_LANE_KVS", str(kvs))
    n = 0
    for c in lc.cases_s_light(kvs):
        ref = oracle.liftover_batch(IX, c.batch, abi.STAGES_ALL, 1).canonical()
        eng = api.Engine(card)
        arrays = DevArrays(c.batch)
        syncs = []
        for _ in range(2):
            got = devbatch.download(eng, eng.liftover_batch_dev(arrays.desc, abi.STAGES_ALL))
            assert got.canonical() == ref, c.name
            t = _timing_row(eng.timing())
            syncs.append(t["host_syncs"])
            assert t["n_items"] == t["n_lane_items"] == len(ref) and t["n_retry_items"] == 0, (c.name, t)
        print(c.name, kvs, syncs)
        assert syncs[0] >= 3 and syncs[1] == 1, (c.name, syncs)
        eng.close()
        n += 1
    assert n == 2 * (9 + 2)
