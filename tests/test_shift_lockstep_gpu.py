"""The hand-built items of tests/shift_cases.py through the C ABI on the card against the C oracle: the shift stage's lockstep loop
switched on (the default) and off (PLO_LANE_LOCKSTEP=0, read when a context is created) in one process.  The CPU legs
(tests/test_shift_lockstep.py) hold the catalogue to what it claims."""
import pytest

import shift_cases as sc
from portello_amd import abi, api

pytestmark = pytest.mark.gpu


def _lift(index, batch, stages, monkeypatch, lockstep):
    if lockstep:
        monkeypatch.delenv("PLO_LANE_LOCKSTEP", raising=False)
    else:
        monkeypatch.setenv("PLO_LANE_LOCKSTEP", "0")
    ix = api.Index(index, 0)
    try:
        eng = api.Engine(ix)
        try:
            res = eng.liftover_batch(batch, stages)
            n_lane = eng.timing().n_lane_items
        finally:
            eng.close()
    finally:
        ix.close()
    return res, n_lane


def _check(items, stages, oracle, monkeypatch, seq_fmt=abi.SEQ_ASCII):
    index, batch = sc.build(items, stages, seq_fmt)
    want = oracle.liftover_batch(index, batch, stages, 1).canonical()
    for lockstep in (True, False):
        res, n_lane = _lift(index, batch, stages, monkeypatch, lockstep)
        assert n_lane == len(items), (lockstep, n_lane)  # every item through k_lift_lanes
        for g, w in zip(res.canonical(), want):
            assert g == w, (lockstep, items[w[0]].name, items[w[0]].why)


@pytest.mark.parametrize("stages", sc.STAGE_SETS)
@pytest.mark.parametrize("seq_fmt", [abi.SEQ_ASCII, abi.SEQ_BAM4])
def test_edges_of_the_lockstep_loop(oracle, monkeypatch, stages, seq_fmt):
    _check(sc.edge_items(), stages, oracle, monkeypatch, seq_fmt)


@pytest.mark.parametrize("stages", sc.STAGE_SETS)
def test_every_reason_for_the_walk(oracle, monkeypatch, stages):
    _check(sc.unclean_items(), stages, oracle, monkeypatch)


def test_position_that_panics_in_the_reference(oracle, monkeypatch):
    _check(sc.panic_items() + sc.edge_items()[:3], abi.STAGE_LSHIFT, oracle, monkeypatch)


@pytest.mark.parametrize("stages", sc.STAGE_SETS)
@pytest.mark.parametrize("seq_fmt", [abi.SEQ_ASCII, abi.SEQ_BAM4])
def test_mixed_wave(oracle, monkeypatch, stages, seq_fmt):
    _check(sc.mixed_items(), stages, oracle, monkeypatch, seq_fmt)
