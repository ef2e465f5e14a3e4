"""The shift stage of the lane-per-item kernel on hand-built items (tests/shift_cases.py): the lockstep loop for clean items -- ops that
alternate match / lone indel between clips --, the streaming pass for lanes whose shift empties a match, and the event-aligned walk for
everything else, under the wave emulator against the C oracle.  Stage sets: all stages, the shift alone, strand + shift.

Which path an item takes is decided by the kernel's LOAD pass; the catalogue states it per item (shift_cases.is_clean, restated from
the rule) and its closed form for clean items is held against the oracle here, so that an item the catalogue calls clean and shifted
by h really is."""
import numpy as np
import pytest

import emu_lib
import shift_cases as sc
from portello_amd import abi, synth

LANE_W = 192  # the production bound of a light item's region


def _run(items, stages, **kw):
    ix, b = sc.build(items, stages, kw.pop("seq_fmt", abi.SEQ_ASCII))
    rc, res, cnt = emu_lib.liftover_batch(ix, b, stages=stages, lane_max_w=LANE_W, **kw)
    assert rc == 0
    return ix, b, res, cnt


@pytest.fixture(scope="module")
def edge():
    return sc.edge_items()


@pytest.fixture(scope="module")
def mixed():
    return sc.mixed_items()


def test_catalogue_is_what_it_says(edge, oracle):
    """every edge item is clean and has the property it was chosen for; the closed form equals the oracle's shift for the items no
    match of which is emptied"""
    by = {it.name: (it, sc.model(it)) for it in edge}
    assert len(by) == len(edge) and all(cl is not None for _, cl in by.values())
    cl = by["partial_del"][1]
    assert 0 < cl[0].h < cl[0].a
    assert any(c.bound == c.h for c in by["eat_middle"][1][1:]) and by["eat_first_del"][1][0].bound == by["eat_first_del"][1][0].h
    c2 = by["chain_clamp_inside"][1][1]
    assert c2.a <= 2 and c2.a < c2.h < c2.bound
    c2 = by["chain_clamp_hit"][1][1]
    assert c2.a <= 2 and c2.raw > c2.bound == c2.h > c2.a
    assert by["h16"][1][0].h == 16 and by["h_over_16"][1][0].h > 16 and by["h_over_32"][1][0].h > 33
    assert by["to_contig_start"][1][0].raw == by["to_contig_start"][1][0].rs and by["to_read_start"][1][0].raw == by["to_read_start"][1][0].qs
    assert by["window_outside"][1][0].re < 16 and by["window_outside"][1][0].h > 0
    assert all(c.panic for it in sc.panic_items() for c in sc.model(it)[-1:])
    assert not any(sc.is_clean(it.ops) for it in sc.unclean_items())
    keep = [it for it, cl in by.values() if all(c.bound - c.h > 0 for c in cl)]
    assert len(keep) >= 18
    ix, b = sc.build(keep, abi.STAGE_LSHIFT)
    ref = oracle.liftover_batch(ix, b, abi.STAGE_LSHIFT, 1)
    for i in range(ref.n_items):
        it = keep[int(ref.item_seg[i])]
        assert int(ref.item_status[i]) == abi.ITEM_LIFTED and int(ref.item_ref_pos[i]) == it.pos, it.name
        assert ref.item_cigar(i).tolist() == sc.shifted_ops(it), it.name


@pytest.mark.parametrize("stages", sc.STAGE_SETS)
@pytest.mark.parametrize("seq_fmt", [abi.SEQ_ASCII, abi.SEQ_BAM4])
def test_edges_of_the_lockstep_loop(edge, oracle, stages, seq_fmt):
    ix, b, res, cnt = _run(edge, stages, seq_fmt=seq_fmt)
    ref = oracle.liftover_batch(ix, b, stages, 1)
    assert cnt[7] == 0 and cnt[23] == len(edge)  # all through the lane code, nothing on the retry list
    got, want = res.canonical(), ref.canonical()
    for g, w in zip(got, want):
        assert g == w, (edge[w[0]].name, edge[w[0]].why)
    assert set(ref.item_status.tolist()) == {abi.ITEM_LIFTED}


@pytest.mark.parametrize("stages", sc.STAGE_SETS)
def test_every_reason_for_the_walk(oracle, stages):
    items = sc.unclean_items()
    ix, b, res, cnt = _run(items, stages)
    ref = oracle.liftover_batch(ix, b, stages, 1)
    for g, w in zip(res.canonical(), ref.canonical()):
        assert g == w, (items[w[0]].name, items[w[0]].why)


def test_position_that_panics_in_the_reference(oracle):
    """(without the strand stage: in walking coordinates the item leaves its contig)"""
    items = sc.panic_items() + sc.edge_items()[:3]
    ix, b, res, cnt = _run(items, abi.STAGE_LSHIFT)
    ref = oracle.liftover_batch(ix, b, abi.STAGE_LSHIFT, 1)
    assert res.canonical() == ref.canonical() and cnt[7] == 0
    assert ref.item_status.tolist()[:2] == [abi.ITEM_PANIC] * 2 and set(ref.item_status.tolist()[2:]) == {abi.ITEM_LIFTED}


@pytest.mark.parametrize("stages", sc.STAGE_SETS)
@pytest.mark.parametrize("order_seed,capw", [(0, 3072), (1, 3072), (7, 3072), (13, 3072), (5, 700)])
def test_mixed_wave(mixed, oracle, stages, order_seed, capw):
    """clean lanes, lanes that empty a match, unclean lanes and forward contigs side by side; lane orders shuffled; an LDS slice that
    holds a group only in several rounds"""
    ix, b, res, cnt = _run(mixed, stages, order_seed=order_seed, lane_capw=capw)
    ref = oracle.liftover_batch(ix, b, stages, 1)
    assert cnt[7] == 0 and cnt[23] == len(mixed)
    for g, w in zip(res.canonical(), ref.canonical()):
        assert g == w, (mixed[w[0]].name, mixed[w[0]].why)


def test_mixed_wave_holds_every_kind(mixed):
    cl = [sc.model(it) for it in mixed]
    assert len(mixed) >= 66 and sum(c is None for c in cl) >= 8 and sum(it.fwd_contig for it in mixed) >= 8
    assert sum(c is not None and len(c) > 0 and all(x.bound > x.h for x in c) for c in cl) >= 8
    assert sum(c is not None and any(x.bound == x.h for x in c) for c in cl) >= 8
    assert {it.flip for it in mixed} == {0, 1}


def test_differential_indel_dense_two_letters(oracle):
    """the indel-dense profile of test_lane_path_indel_dense over a two-letter alphabet: long homologies, many emptied matches"""
    n_seeds = 40  # (about a second and a half each)
    for seed in range(n_seeds):
        cfg = synth.config("tiny", n_reads=48, seed=500 + seed, read_len_mean=1500, read_len_sd=300,
                           read_rates=synth.EditRates(mismatch=5e-3, ins=2.5e-2, dele=2.5e-2, hpol_frac=0.5, min_gap=1),
                           contig_rates=synth.EditRates(mismatch=1e-3, ins=3e-3, dele=3e-3, hpol_frac=0.3, big_indel_prob=0.02))
        w = synth.generate(cfg)
        ix, b = w.index_data(), w.batch_data()
        # A C G T -> A T A T: closed under complement, so a reverse-complemented read keeps its homologies
        two = np.zeros(256, np.uint8)
        for ch, to in zip(b"ACGTN", b"ATATA"):
            two[ch] = to
        nib = np.array([0] + [8 if v in (2, 8) else 1 for v in range(1, 16)], np.uint8)  # BAM4 codes: A 1, C 2, G 4, T 8
        assert b.seq_fmt == abi.SEQ_BAM4
        b.seq = (nib[b.seq >> 4] << 4) | nib[b.seq & 15]
        ix.rev_contig_seq = [None if s is None else two[s] for s in ix.rev_contig_seq]
        ix.chrom_seq = [two[s] for s in ix.chrom_seq]
        for stages in sc.STAGE_SETS:
            rc, res, cnt = emu_lib.liftover_batch(ix, b, stages=stages, lane_max_w=100000, lane_capw=60000, order_seed=seed)
            assert rc == 0
            assert res.canonical() == oracle.liftover_batch(ix, b, stages, 1).canonical(), (seed, stages)


def test_in_a_sanitizer_program(tmp_path, oracle, edge, mixed):
    """the hand-built items through the emulated lane code in the stand-alone sanitizer program of tests/emu_enumerate_lib.py (a main of its
    own, every array in a heap block of its exact size, AddressSanitizer and UBSan on): clean exit, results equal to the oracle"""
    import emu_enumerate_lib

    for k, (items, stages) in enumerate([(edge, abi.STAGES_ALL), (edge, abi.STAGE_LSHIFT), (mixed, abi.STAGES_ALL), (sc.unclean_items(), abi.STAGES_ALL),
                                         (sc.panic_items(), abi.STAGE_LSHIFT)]):
        ix, b = sc.build(items, stages)
        rc, err, res = emu_enumerate_lib.run_asan(ix, [(b, stages)], tmp_path, name=f"shift{k}")
        assert rc == 0, err[-3000:]
        want = oracle.liftover_batch(ix, b, stages, 1).canonical()
        for erc, lanes, got in res[0]:
            assert erc == 0 and got.canonical() == want, (k, lanes)
