"""The front of every plo_liftover_batch* call -- the batch checks, the item count and list, the scans and the class order (k_seg_count,
k_scan_*, k_item_emit, k_item_desc, k_cls_hist, k_permute2, k_permute2_s in engine.hip) -- on hand-built batches at their edges
(tests/enumerate_cases.py) against a plain restatement of the rule (tests/enumerate_expect.py), the C oracle and the emulator.

k_seg_count is a lane-parallel restatement of the serial functions of enumerate.hpp and exists on the GPU only, so the CPU legs hold the
restatement, the oracle and the emulator's serial functions to each other -- what the card's counts must equal -- and the GPU legs hold the
card to them.  Family E (read segments that leave their contig) goes through the emulated device code in a sanitizer program first; what
it showed in bounds goes to the card, all of it by name (E_CASES_ON_THE_CARD)."""
import pytest

import emu_enumerate_lib
import emu_lib
import enumerate_cases as ec
import enumerate_expect as ex
from dev_arrays import DevArrays
from portello_amd import abi, api

IX = ec.INDEX
MSG = {abi.PLO_ERR_INVALID_ARG: "an index points outside its array", abi.PLO_ERR_RANGE: "a CIGAR spanning 2^30 bases or more"}

# Family E on the card: every case -- the sanitizer program lifts all of them in bounds (test_family_e_in_a_sanitizer_program).  The four
# with a negative rev_pos are refused there (PLO_ERR_RANGE), the others are accepted and compared with the oracle.
E_CASES_ON_THE_CARD = ("E_end_on_contig_end", "E_end_on_contig_end_explicit", "E_end_on_contig_end_indels", "E_one_past_contig_end",
                       "E_one_past_contig_end_explicit", "E_one_past_contig_end_indels", "E_far_past_contig_end", "E_past_end_forward_segment",
                       "E_wholly_behind", "E_wholly_behind_far")


def _small_cases():
    return ec.accepted_small() + [c for c in ec.cases_leaving() if c.verdict == ex.OK]


def _big_cases():
    return ([ec.case_scan(n) for n in ec.SCAN_SIZES] + [ec.case_classes(n) for n in ec.CLASS_SIZES] +
            [ec.case_classes(n, light_only=True) for n in ec.CLASS_SIZES])


@pytest.fixture(scope="module")
def accepted(oracle):
    """[(case, oracle result)]: computed once, shared by the CPU and the GPU legs, never changed"""
    return [(c, oracle.liftover_batch(IX, c.batch, c.stages, 1)) for c in _small_cases() + _big_cases()]


def _pairs(res):
    return list(zip(res.item_seg.tolist(), res.item_cseg.tolist()))


# ---- CPU legs ---------------------------------------------------------------------------------------------------------------------------

def test_restatement_gives_every_hand_written_verdict():
    cases = ec.cases_walk() + ec.cases_merge() + ec.cases_overlap() + ec.cases_verdict() + [ec.case_read_span_wraps()] + ec.cases_leaving() + _big_cases()
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    for c in cases:
        assert ex.verdict(IX, c.batch, c.stages) == c.verdict, (c.name, c.why)
    assert sum(c.verdict == ex.INVALID_ARG for c in cases) >= 20 and sum(c.verdict == ex.RANGE for c in cases) >= 30
    assert {c.name for c in ec.cases_leaving()} == set(E_CASES_ON_THE_CARD)


def test_restatement_on_hand_worked_segments():
    """the restatement itself, on values worked out by hand"""
    op = ex.op
    ops = [op(5, ex.OP_M), op(0, ex.OP_EQ), op(2, ex.OP_X), op(3, ex.OP_I), op(4, ex.OP_D), op(6, ex.OP_N), op(7, ex.OP_S), op(8, ex.OP_H), op(9, ex.OP_P), op(1, ex.OP_M)]
    assert ex.ref_span(ops) == 5 + 0 + 2 + 4 + 6 + 1 and ex.read_span(ops) == 5 + 0 + 2 + 3 + 7 + 8 + 1 and ex.n_merged(ops) == 8
    assert ex.read_span_sat([op((1 << 28) - 1, ex.OP_S)] * 16) == 16 * ((1 << 28) - 1) and ex.read_span_sat([op((1 << 28) - 1, ex.OP_S)] * 17) == 0xFFFFFFFF
    assert ex.n_merged([]) == 0 and ex.n_merged([op(1, ex.OP_M)] * 5) == 1 and ex.n_merged([op(1, ex.OP_M), op(1, ex.OP_P), op(1, ex.OP_M)]) == 3
    assert ex.region_dwords(188, 0, 1) == 192 == ex.LANE_MAX_W and ec.N_LIGHT_MAX == 188 and ex.region_dwords(10, 3, 6) == 10 + 6 + 2
    assert ex.block_map_keys(IX, 0) == [0, 1000] and ex.block_map_keys(IX, 2) == [100, 900] and ex.block_map_keys(IX, 4) == [400, 700]
    assert ex.sparse_header_bytes(0) == 0 and ex.sparse_header_bytes(1) == 16 and ex.sparse_header_bytes(2048) == 16 and ex.sparse_header_bytes(2049) == 32
    # merged counts of the padded segments, by their construction: total - (run - 1)
    for at, run in ec.merge_layouts():
        assert ex.n_merged(ec.padded_ops(200, at, run)) == 200 - (run - 1)


def test_three_voices_agree_on_accepted_cases(accepted):
    """restatement, C oracle and emulator: the item list, every status, flip, mapq, chromosome, position and CIGAR; the emulator's count of
    light items (its serial segment_n_merged and build_item_desc) equals the restated classes"""
    for c, ref in accepted:
        assert _pairs(ref) == ex.item_list(IX, c.batch), c.name
        mixed = c.name.startswith("D_classes") and not c.name.endswith("_light")
        # (the emulator takes minutes for thousands of heavy items through the tile code: there they go through the lane code, with an LDS
        # slice that holds a group of them)
        kw = dict(lane_max_w=256, lane_capw=16384) if mixed else dict(lane_max_w=ex.LANE_MAX_W)
        rc, res, cnt = emu_lib.liftover_batch(IX, c.batch, stages=c.stages, **kw)
        assert rc == 0, c.name
        assert res.canonical() == ref.canonical(), c.name
        cls = ex.class_counts(IX, c.batch) if c.batch.item_seg is None and c.stages == abi.STAGES_ALL else None
        if cls is not None and not mixed:
            assert cnt[23] == cls[0] + cls[1], (c.name, cnt[23], cls)
        if c.n_lane_items is not None:
            assert cls[0] + cls[1] == c.n_lane_items, (c.name, cls)  # (the hand-written count)
    # the scan formulation on the families whose items are few
    for c, ref in accepted:
        if c.family in ("A", "B", "E"):
            rc, res, _ = emu_lib.liftover_batch(IX, c.batch, stages=c.stages)
            assert rc == 0 and res.canonical() == ref.canonical(), c.name


def test_read_span_is_observed(accepted):
    by = {c.name: ref for c, ref in accepted}
    st = by["A_read_span"].item_status.tolist()
    assert st == [abi.ITEM_LIFTED, abi.ITEM_LEN_MISMATCH, abi.ITEM_LEN_MISMATCH] * 4, st
    assert by["C_read_span_wraps"].item_status.tolist() == [abi.ITEM_LIFTED, abi.ITEM_LEN_MISMATCH]
    # each op code alone: lifted or not, never a length mismatch (read_seq_len is the restated span)
    assert abi.ITEM_LEN_MISMATCH not in by["A_one_op_each"].item_status.tolist()
    assert by["A_one_op_beside_a_match"].item_status.tolist() == [abi.ITEM_LIFTED] * 9
    # the walk's segments astride the strand border: two items each, the second on the reverse contig segment
    walk = by["A_walk_mid"]
    assert (walk.item_cseg == 1).sum() >= 56 and (walk.item_status == abi.ITEM_LIFTED).sum() >= 100


def test_family_e_in_a_sanitizer_program(tmp_path, oracle):
    """read segments that leave their contig through the emulated lane code and the scan formulation, every array in a heap block of its
    exact size, AddressSanitizer and UBSan on: clean exit for all of them; the accepted ones equal the oracle, and the emulator reports the
    card's refusal (3, after lifting) for exactly the cases whose hand-written verdict is PLO_ERR_RANGE"""
    cases = ec.cases_leaving() + ec.cases_overlap()
    rc, err, res = emu_enumerate_lib.run_asan(IX, [(c.batch, c.stages) for c in cases], tmp_path)
    assert rc == 0, err[-3000:]
    for c, modes in zip(cases, res):
        for erc, lanes, got in modes:
            assert erc == (0 if c.verdict == ex.OK else 3), (c.name, erc)
            if c.verdict == ex.OK:
                assert got.canonical() == oracle.liftover_batch(IX, c.batch, c.stages, 1).canonical(), c.name


# ---- GPU legs ---------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def card():
    index = api.Index(IX)
    keys = {}

    def keys_of(g):
        if g not in keys:
            keys[g] = [int(k) for k in index.segment_map(g)[0]]
        return keys[g]

    yield index, keys_of
    index.close()


def _run_dev(eng, c):
    from portello_amd import devbatch

    arrays = DevArrays(c.batch)
    out = eng.liftover_batch_dev(arrays.desc, c.stages)
    return devbatch.download(eng, out)


def _check_counts(eng, c, ref, keys_of):
    """plo_timing's counts against the restatement.  n_items: the restated item list.  n_in_ops: "input CIGAR ops over all items", the ops of
    every item's read segment.  n_out_ops: "output CIGAR ops", the ops of every CIGAR handed out.  n_miss_items: 0, no batch here is sparse.
    n_lane_items: the restated light classes.  The heavy items have no count of their own unless a lane kernel takes them (then
    n_heavy_lane_items is all of them: the choice is a sizing rule of the engine, so 0 or all); the tile kernel that takes them otherwise
    counts only those it hands on (n_mid_items, n_big_items: at most the heavy ones).  An item of the catalogue has 1 .. 200 ops: none is
    handed on for its size, so equality with 0 would be the expectation, but when an LDS slice overflows is the engine's affair."""
    t = eng.timing()
    items = ex.item_list(IX, c.batch)
    print(c.name, "n_items", int(t.n_items), "lane", int(t.n_lane_items), "heavy_lane", int(t.n_heavy_lane_items), "mid", int(t.n_mid_items), "big",
          int(t.n_big_items), "retry", int(t.n_retry_items), "miss", int(t.n_miss_items), "in", int(t.n_in_ops), "out", int(t.n_out_ops), "syncs", int(t.host_syncs))
    assert int(t.n_items) == ref.n_items == len(items), c.name
    assert int(t.n_in_ops) == sum(len(ex.seg_ops(c.batch, s)) for s, _ in items), c.name
    assert int(t.n_out_ops) == int(ref.item_cigar_len.sum()), c.name
    assert int(t.n_miss_items) == 0, c.name
    if c.batch.item_seg is None and c.stages == abi.STAGES_ALL:
        cls = ex.class_counts(IX, c.batch, keys_of)
        heavy = cls[2] + cls[3]
        assert int(t.n_lane_items) == cls[0] + cls[1], (c.name, int(t.n_lane_items), cls)
        assert int(t.n_heavy_lane_items) in (0, heavy), (c.name, int(t.n_heavy_lane_items), cls)
        assert int(t.n_mid_items) + int(t.n_big_items) <= heavy, c.name
        if int(t.host_syncs) == 1:  # the one-round-trip path: light items only
            assert heavy == 0, c.name
    if c.n_lane_items is not None:
        assert int(t.n_lane_items) == c.n_lane_items, (c.name, int(t.n_lane_items))


@pytest.mark.gpu
def test_block_map_keys_on_the_card(card):
    """the restated keys are the keys the classes are restated with on the card"""
    index, keys_of = card
    for g in range(IX.n_segments):
        assert keys_of(g) == ex.block_map_keys(IX, g), g


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["host", "dev"])
def test_accepted_cases_on_the_card(card, accepted, entry):
    """every accepted case (family E's among them: E_CASES_ON_THE_CARD) through plo_liftover_batch / plo_liftover_batch_dev on ONE context, so
    that careful and one-round-trip calls alternate as the batches' classes decide: item by item against the oracle, n_items and
    n_lane_items against the restated classes"""
    index, keys_of = card
    eng = api.Engine(index)
    for c, ref in accepted:
        got = eng.liftover_batch(c.batch, c.stages) if entry == "host" else _run_dev(eng, c)
        assert _pairs(got) == _pairs(ref), c.name
        assert got.canonical() == ref.canonical(), c.name
        _check_counts(eng, c, ref, keys_of)
    eng.close()


@pytest.mark.gpu
def test_light_only_batches_careful_then_armed(card, accepted):
    """the light-only batches of family D three times on one context: once careful, twice on the one-round-trip path (host_syncs as
    test_one_host_round_trip_path expects), the same results each time"""
    index, keys_of = card
    n = 0
    for c, ref in accepted:
        if not (c.family == "D" and (c.name.startswith("D_scan") or c.name.endswith("_light"))):
            continue
        eng = api.Engine(index)
        arrays = DevArrays(c.batch)
        from portello_amd import devbatch

        syncs = []
        for _ in range(3):
            got = devbatch.download(eng, eng.liftover_batch_dev(arrays.desc, c.stages))
            assert got.canonical() == ref.canonical(), c.name
            t = eng.timing()
            syncs.append(int(t.host_syncs))
            assert int(t.n_items) == ref.n_items == int(t.n_lane_items), c.name
        if ref.n_items:
            assert syncs[0] >= 3 and syncs[1] == 1 and syncs[2] == 1, (c.name, syncs)
        eng.close()
        n += 1
    assert n == len(ec.SCAN_SIZES) + len(ec.CLASS_SIZES)


@pytest.mark.gpu
def test_refused_cases_on_the_card(card, oracle):
    """every refused case once on a fresh context and once on a context armed for the one-round-trip path (where the lift kernels run before
    the host sees the flags): status and message, and a good batch lifts on the same context afterwards.  The caller-owned arrays carry a
    spare tail, so a check that failed to fire would still read inside an allocation."""
    from portello_amd import devbatch

    index, _ = card
    good = ec.Case("good", ec.base_batch(ec.N_BASE).batch(), ex.OK, "")
    good_ref = oracle.liftover_batch(IX, good.batch, abi.STAGES_ALL, 1).canonical()
    good_dev = DevArrays(good.batch)
    armed = api.Engine(index)

    def lift_good(eng):
        got = devbatch.download(eng, eng.liftover_batch_dev(good_dev.desc))
        assert got.canonical() == good_ref
        return int(eng.timing().host_syncs)

    lift_good(armed)
    assert lift_good(armed) == 1
    cases = ec.refused()
    assert len(cases) >= 60
    for c in cases:
        arrays = DevArrays(c.batch)
        fresh = api.Engine(index)
        for eng, kind in ((fresh, "fresh"), (armed, "armed")):
            with pytest.raises(api.PortelloError) as e:
                eng.liftover_batch_dev(arrays.desc, c.stages)
            assert e.value.status == c.verdict, (c.name, kind, c.why)
            assert MSG[c.verdict] in str(e.value), (c.name, kind, str(e.value))
            lift_good(eng)
        fresh.close()
        assert lift_good(armed) == 1, c.name  # (armed again for the next refusal)
    armed.close()
