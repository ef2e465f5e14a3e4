"""Bases other than A C G T: N gaps and IUPAC codes in reference and contigs, N / IUPAC / '=' (and lowercase, in ASCII) in reads.
The reference compares bases byte by byte after decoding ("=ACMGRSVTWYHKDBN") and comp_base (seq_util.rs:1-15: A C G T N and
their lowercase kept, everything else -> N), so a read N matches a reference N, a read R matches a reference R only while the
read is not flipped, and indels next to N runs shift across them.  CPU: the device code under the emulator / on the host vs the
oracle.  GPU: HIP vs oracle."""
import numpy as np
import pytest

import emu_lib
import fuzz_cases
from portello_amd import abi

CODES = fuzz_cases.BAM4_CODES


def _oracle_read(oracle, seq, off, n, fmt, flip) -> bytes:
    """the read as the reference sees it: decoded, and reverse-complemented when flipped"""
    s = oracle.decode_bam4(seq[off:], n) if fmt == abi.SEQ_BAM4 else bytes(seq[off: off + n])
    return oracle.rev_comp(s) if flip else s


def _aligned(n, shift):
    """n bytes starting `shift` bytes past a 64-byte boundary"""
    buf = np.zeros(n + 128, dtype=np.uint8)
    a = (-buf.ctypes.data) % 64 + shift
    return buf[a: a + n]


@pytest.mark.parametrize("seq_fmt", [abi.SEQ_BAM4, abi.SEQ_ASCII])
def test_read_decode_paths_vs_oracle(oracle, seq_fmt):
    """xor_window16, xw16_issue + xw16_decode and read_base against ref byte ^ oracle base: every read code, every byte alignment of
    both windows, both nibble parities, flipped and not, windows at the first and last bases of both buffers"""
    rng = np.random.default_rng(77 + seq_fmt)
    ref_len, L = 70, 61
    ref_letters = np.frombuffer(CODES + b"acgtn" if seq_fmt == abi.SEQ_ASCII else CODES, dtype=np.uint8)
    if seq_fmt == abi.SEQ_BAM4:
        codes = np.concatenate([rng.permutation(16), rng.integers(0, 16, L - 16)]).astype(np.uint8)
        ascii_read = np.frombuffer(CODES, dtype=np.uint8)[codes]
        packed = fuzz_cases.pack_bam4(ascii_read.tobytes())
    else:  # every code letter, lowercase, and bytes no base table knows
        letters = np.frombuffer(CODES + b"acgtnmrwsykvhdb" + b"\x00\xff*.Xx", dtype=np.uint8)
        ascii_read = np.concatenate([rng.permutation(letters), letters[rng.integers(0, len(letters), L - len(letters))]]).astype(np.uint8)
        packed = ascii_read
    n_ok = np.zeros(2, dtype=np.int64)
    n_cases = n_xor_nonzero = 0
    for rshift in range(4):
        ref = _aligned(ref_len, rshift)
        ref[:] = ref_letters[rng.integers(0, len(ref_letters), ref_len)]
        # the read's stored bases: some bytes before it (all four alignments) and either room behind it or none
        for seq_off, tail in ((0, 0), (1, 24), (2, 0), (3, 24), (5, 7)):
            seq = _aligned(seq_off + len(packed) + tail, (rshift + seq_off) & 3)
            seq[:] = 0x5a
            seq[seq_off: seq_off + len(packed)] = packed
            for flip in (False, True):
                view = np.frombuffer(_oracle_read(oracle, seq, seq_off, L, seq_fmt, flip), dtype=np.uint8)
                for q0 in range(-1, L - 14):
                    for r0 in {-1, 0, 1, 2, 3, (q0 * 7) % (ref_len - 15), ref_len - 17, ref_len - 16, ref_len - 15, ref_len - 14}:
                        X, ok = emu_lib.xor_windows(ref, r0, seq, seq_off, L, seq_fmt, flip, q0)
                        exp = np.zeros(16, dtype=np.uint8)
                        t = np.arange(16)
                        valid = (r0 + t >= 0) & (r0 + t < ref_len) & (q0 + t >= 0) & (q0 + t < L)
                        exp[valid] = ref[(r0 + t)[valid]] ^ view[(q0 + t)[valid]]
                        tag = f"fmt {seq_fmt} flip {flip} ref shift {rshift} seq_off {seq_off} tail {tail} r0 {r0} q0 {q0}"
                        assert (X[2] == exp).all(), f"read_base: {tag}\n got {X[2]}\n exp {exp}"
                        for k, name in ((0, "xor_window16"), (1, "xw16_decode")):
                            if ok[k]:
                                assert valid.all(), f"{name} took a window outside a buffer: {tag}"
                                assert (X[k] == exp).all(), f"{name}: {tag}\n got {X[k]}\n exp {exp}"
                        n_ok += ok
                        n_cases += 1
                        n_xor_nonzero += int(valid.all() and (exp == 0).any())
    # the window paths took a good share of the windows (not all: some lie at the buffers' edges), and matching bytes were among them
    assert (n_ok > n_cases // 4).all() and (n_ok < n_cases).all(), (n_ok, n_cases)
    assert n_xor_nonzero > 100


# ---- synthetic workloads with N gaps, IUPAC codes and N / '=' read calls (synth.Ambiguity) ----------------------------------------

def _amb_config(seed, seq_fmt=abi.SEQ_BAM4, n_reads=120, **over):
    from portello_amd import synth

    kw = dict(n_reads=n_reads, seed=seed, split_read_frac=0.2, read_len_mean=3000, read_len_sd=900, seq_fmt=seq_fmt,
              ambiguity=synth.Ambiguity(seed=seed, gaps_per_mb=40.0, iupac_frac=2e-3, read_call_frac=3e-3))
    kw.update(over)
    return synth.config("tiny", **kw)


def _read_letters(b) -> np.ndarray:
    """the stored read bases as letters (BAM 4-bit reads decoded read by read)"""
    if b.seq_fmt == abi.SEQ_ASCII:
        return np.asarray(b.seq, dtype=np.uint8)
    codes = np.frombuffer(CODES, dtype=np.uint8)
    out = []
    for r in range(b.n_reads):
        o, n = int(b.read_seq_off[r]), int(b.read_seq_len[r])
        p = np.asarray(b.seq[o: o + (n + 1) // 2], dtype=np.uint8)
        out.append(codes[np.stack([p >> 4, p & 15], 1).reshape(-1)[:n]])
    return np.concatenate(out)


def _assert_every_code(b):
    """the reads carry every one of the 16 BAM base codes, and not just now and then"""
    letters = _read_letters(b)
    got = set(letters.tolist())
    assert got >= set(CODES), sorted(set(CODES) - got)
    assert (~np.isin(letters, np.frombuffer(b"ACGT", np.uint8))).mean() > 0.02


@pytest.mark.parametrize("seq_fmt", [abi.SEQ_BAM4, abi.SEQ_ASCII])
def test_finish_device_code_on_host_ambiguous_bases(oracle, seq_fmt):
    """finish_core.hpp on the host (k_revcomp's comp8 / comp_nibble on every 4-bit code, the ASCII complement) against the oracle, on
    reads that carry all 16 codes, at every length residue mod 16, both strands"""
    from portello_amd import synth
    from test_finish import _compare_finish

    residues, strands = set(), set()
    for seed, nthreads in ((511, 7), (512, 64)):
        w = synth.generate(_amb_config(seed, seq_fmt))
        b = w.batch_data()
        _assert_every_code(b)
        rng = np.random.default_rng(seed)
        lens = b.read_seq_len.astype(np.int64)
        qoff = np.cumsum(lens) - lens
        qual = rng.integers(0, 94, size=int(lens.sum()), dtype=np.uint8)
        flags = (b.read_is_reverse.astype(np.uint16) * 0x10) | (rng.integers(0, 2, size=b.n_reads).astype(np.uint16) * 0x400)
        lift = oracle.liftover_batch(w.index_data(), b, abi.STAGES_ALL, 1)
        ref = oracle.finish_batch(b, flags, qual, qoff, lift)
        got = emu_lib.finish_batch(b, flags, qual, qoff, lift, nthreads=nthreads)
        assert _compare_finish(got, ref, lift, b, seq_fmt) > 20
        flipped = np.nonzero(ref["item_seq_off"] != abi.NO_FLIP)[0]
        reads = np.concatenate([b.seg_read[lift.item_seg][flipped], np.nonzero(ref["read_seq_off"] != abi.NO_FLIP)[0]])
        residues |= set((b.read_seq_len[reads] % 16).tolist())
        strands |= set(b.read_is_reverse[reads].tolist())
    # the flipped records cover every length residue and both read strands
    assert residues == set(range(16)) and strands == {0, 1}


@pytest.fixture(scope="module")
def amb_contig_bam(tmp_path_factory):
    from portello_amd import bamsynth, synth

    d = tmp_path_factory.mktemp("p1amb")
    w = synth.generate(_amb_config(531, n_reads=50, chrom_lens=(600_000, 400_000), n_contigs_per_hap=6, max_segments=4,
                                   ambiguity=synth.Ambiguity(seed=531, gaps_per_mb=30.0, iupac_frac=3e-3)), keep_contigs=True)
    path = str(d / "asm.bam")
    meta = bamsynth.write_contig_bam(w, path, seed=9, perturb=True)
    return w, path, meta


def test_phase1_ambiguous_bases(oracle, amb_contig_bam):
    """phase 1 on contigs with N gaps, IUPAC codes and N joins: the segments equal oracle/pyphase1.py's, every byte of rev_contig_seq
    is the reference's reverse complement of the contig (IUPAC -> N)"""
    import bamcheck
    from oracle import pyphase1 as p1
    from portello_amd import bam
    from test_phase1 import _norm_clip, _segments_of

    w, path, meta = amb_contig_bam
    cn = meta["contig_names"]
    ph = bam.Phase1(path, cn, [int(x) for x in w.contig_len], n_threads=2)
    got = ph.index_data([s.numpy() for s in w.chrom_seq])
    _, _, recs = bamcheck.read_bam(path)
    exp = p1.scan_contig_bam(recs, meta["ref_names"], cn)
    assert _segments_of(got) == [[(s.seq_order_read_start, s.seq_order_read_end, s.chrom_index, s.pos, s.is_fwd_strand, s.mapq, _norm_clip(s.cigar))
                                  for s in segs] for segs in exp.contigs]
    n_rev = n_iupac = 0
    for c in range(len(cn)):
        a, e = got.rev_contig_seq[c], exp.rev_contig_seq[c]
        assert (a is None) == (e is None) and (a is None or a.tobytes() == e)
        if a is not None:
            fwd = w.contig_fwd[c].numpy()
            assert a.tobytes() == oracle.rev_comp(fwd)
            n_rev += 1
            n_iupac += int(np.isin(fwd, np.frombuffer(b"MRWSYKVHDB", np.uint8)).sum())
    assert n_rev >= 2 and n_iupac > 20
    ph.close()


@pytest.mark.parametrize("is_target_region", [False, True])
def test_record_bytes_ambiguous_bases(oracle, tmp_path, is_target_region):
    """plo_records_build (host revcomp_packed, record assembly) against the Python restatement on a read BAM with N / IUPAC / '='"""
    import struct

    import bamcheck
    from oracle.expect import expected_records
    from portello_amd import bam, bamsynth, synth

    w = synth.generate(_amb_config(541, n_reads=300, split_read_frac=0.3, sorted_reads=True))
    _assert_every_code(w.batch_data())
    path = str(tmp_path / "reads.bam")
    meta = bamsynth.write_read_bam(w, path, level=6, n_unmapped=4)
    ix = w.index_data()
    _, _, recs = bamcheck.read_bam(path)
    prim = [r for r in recs if not (struct.unpack_from("<H", r, 18)[0] & 0x804)]
    rd = bam.BamReader(path, 2)
    win = rd.read_window(100_000)
    b = win.batch_data()
    res = oracle.liftover_batch(ix, b, abi.STAGES_ALL, 2)
    o, keep = abi.out_from_result(res)
    cn, rn = meta["contig_names"], bamsynth.ref_names(w)
    data, off, n_lift, _ = win.build_records(o, ix.to_desc(), cn, rn, is_target_region=is_target_region, n_threads=3)
    exp = expected_records(prim, ix, cn, rn, res, is_target_region)
    got = [data[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]
    assert len(got) == len(exp) and n_lift > 100
    for i, (a, e) in enumerate(zip(got, exp)):
        assert a == e, i
    assert (res.item_need_flipped[res.item_status == abi.ITEM_LIFTED] == 1).sum() > 20
    win.close()
    rd.close()


# ---- GPU: HIP vs oracle ------------------------------------------------------------------------------------------------------------

def _same(ref, got, tag):
    a, c = ref.canonical(), got.canonical()
    assert len(a) == len(c), tag
    bad = [i for i, (x, y) in enumerate(zip(a, c)) if x != y]
    assert not bad, f"{tag}: {len(bad)} of {len(a)} items differ, first {a[bad[0]][:7]} vs {c[bad[0]][:7]}"


def _n_changed(oracle, ix, b, ref):
    """items whose oracle result changes when the reads' non-ACGT bases become C (homology / shifting crossed them)"""
    from test_fuzz_parity import _non_acgt_read_bases

    _, b2 = _non_acgt_read_bases(b)
    return sum(x != y for x, y in zip(ref.canonical(), oracle.liftover_batch(ix, b2, abi.STAGES_ALL, 16).canonical()))


@pytest.mark.gpu
@pytest.mark.parametrize("seq_fmt", [abi.SEQ_BAM4, abi.SEQ_ASCII])
def test_gpu_every_item_of_an_ambiguous_workload(oracle, seq_fmt):
    """every item of a 20 k-read workload with N gaps, IUPAC codes and N / '=' calls: host API, device-resident API (the second call
    on the one-round-trip path), and (BAM 4-bit) sparse bases at margin 0, where a base the batch lacks reads as N -- with N in the
    reference only the miss flag keeps such a probe from matching"""
    import torch

    from portello_amd import api, bam, devbatch, synth

    w = synth.generate(_amb_config(551 + seq_fmt, seq_fmt, n_reads=20_000, chrom_lens=(1_000_000,), n_contigs_per_hap=4), device="cuda")
    ix, b = w.index_data(), w.batch_data()
    _assert_every_code(b)
    ref = oracle.liftover_batch(ix, b, abi.STAGES_ALL, 16)
    assert _n_changed(oracle, ix, b, ref) > 20
    index = api.Index(ix)
    eng = api.Engine(index)
    _same(ref, eng.liftover_batch(b), "host API")
    if seq_fmt == abi.SEQ_BAM4:
        sp = bam.sparse_pack(b, 0)
        got = abi.result_from_out(eng.liftover_batch_host(sp.to_desc()))
        assert eng.timing().n_miss_items > 0
        _same(ref, got, "sparse bases, margin 0")
    eng.close()
    index.close()
    dindex = api.Index(w.index_data_device())
    deng = api.Engine(dindex, stream=torch.cuda.current_stream().cuda_stream)
    db = devbatch.DeviceBatch.from_workload(w)
    _same(ref, devbatch.run_and_download(deng, db), "device-resident API")
    got = devbatch.run_and_download(deng, db)
    assert int(deng.timing().host_syncs) == 1
    _same(ref, got, "device-resident API, one round trip")
    deng.close()
    dindex.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seq_fmt", [abi.SEQ_BAM4, abi.SEQ_ASCII])
@pytest.mark.parametrize("route", ["mid", "big", "retry"])
def test_gpu_scan_formulation_ambiguous_bases(oracle, monkeypatch, route, seq_fmt):
    """indel-dense reads over N gaps / IUPAC codes / N and '=' calls through the scan formulation (the fixed geometry of
    test_synthetic_indel_dense_large_item_kernels: workgroup-per-item and one-wave-per-item kernels), and through the retry list"""
    from portello_amd import api, synth

    if route == "retry":  # heavy items longer than their regions (test_heavy_items_longer_than_their_region_are_handed_on)
        env = {"PLO_LANE_STREAM": "0", "PLO_LANE_HEAVY_MIN": "0", "PLO_LANE_HEAVY_STRIDE": "640", "PLO_LANE_MAX_W": "150"}
    else:
        env = {"PLO_WINDOW": "256", "PLO_BIG_THRESH": "176", "PLO_CAP": "320", "PLO_MID_WAVES": "8" if route == "mid" else "0",
               "PLO_MID_CAP": "512"}
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    w = synth.generate(_amb_config(561 + seq_fmt, seq_fmt, n_reads=200, read_len_mean=6000, read_len_sd=1500,
                                   read_rates=synth.EditRates(mismatch=5e-3, ins=2.5e-2, dele=2.5e-2, hpol_frac=0.5, min_gap=1),
                                   contig_rates=synth.EditRates(mismatch=1e-3, ins=3e-3, dele=3e-3, hpol_frac=0.3, big_indel_prob=0.02)))
    ix, b = w.index_data(), w.batch_data()
    ref = oracle.liftover_batch(ix, b, abi.STAGES_ALL, 8)
    assert _n_changed(oracle, ix, b, ref) > 5
    index = api.Index(ix)
    eng = api.Engine(index)
    got = eng.liftover_batch(b)
    t = eng.timing()
    counters = dict(mid=int(t.n_mid_items), big=int(t.n_big_items), retry=int(t.n_retry_items), heavy=int(t.n_heavy_lane_items))
    assert counters[route] > 0, counters
    _same(ref, got, f"{route} {counters}")
    eng.close()
    index.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seq_fmt", [abi.SEQ_BAM4, abi.SEQ_ASCII])
def test_gpu_finish_ambiguous_bases(oracle, seq_fmt):
    """k_revcomp (comp8 on every 4-bit code, the ASCII complement) and the other finishing kernels against the oracle"""
    import torch

    from portello_amd import api, devbatch, synth
    from test_finish import _compare_finish

    w = synth.generate(_amb_config(571 + seq_fmt, seq_fmt, n_reads=400, read_len_sd=1200), device="cuda")
    _assert_every_code(w.batch_data())
    index = api.Index(w.index_data_device())
    eng = api.Engine(index, stream=torch.cuda.current_stream().cuda_stream)
    db = devbatch.DeviceBatch.from_workload(w)
    desc = db.desc()
    fin, keep = devbatch.finish_inputs(w, db, seed=9)
    torch.cuda.synchronize()
    out = eng.liftover_batch_dev(desc)
    fo = eng.finish_batch_dev(desc, fin)
    lift = devbatch.download(eng, out)
    got = devbatch.download_finish(eng, fo, lift.n_items, db.n_reads)
    b = w.batch_data()
    ref = oracle.finish_batch(b, keep["flags"].cpu().numpy().view(np.uint16), keep["qual"].cpu().numpy(), keep["qoff"].cpu().numpy(),
                              oracle.liftover_batch(w.index_data(), b, abi.STAGES_ALL, 2))
    assert _compare_finish(got, ref, lift, b, seq_fmt) > 50
    eng.close()
    index.close()


@pytest.mark.gpu
def test_gpu_bams_in_lifted_bam_out_ambiguous_bases(oracle, tmp_path):
    """test_bams_in_lifted_bam_out on an assembly and reads with N gaps, IUPAC codes and N / '=' calls: phase 1 from the assembly BAM,
    HIP liftover of the read BAM's window, record bytes equal to the Python expectation"""
    import struct as st

    import bamcheck
    from oracle.expect import expected_records
    from portello_amd import api, bam, bamsynth, synth

    w = synth.generate(_amb_config(581, n_reads=800, sorted_reads=True, read_len_mean=15_000, read_len_sd=3_000))
    _assert_every_code(w.batch_data())
    asm, reads = str(tmp_path / "asm.bam"), str(tmp_path / "reads.bam")
    m1 = bamsynth.write_contig_bam(w, asm, seed=3)
    m2 = bamsynth.write_read_bam(w, reads, level=1)
    rd = bam.BamReader(reads, 2)
    ph = bam.Phase1(asm, rd.ref_names, rd.ref_lens, n_threads=2)
    ix = ph.index_data([s.numpy() for s in w.chrom_seq])
    index = api.Index(ix)
    eng = api.Engine(index)
    ixd = ix.to_desc()
    _, _, recs = bamcheck.read_bam(reads)
    prim = [r for r in recs if not (st.unpack_from("<H", r, 18)[0] & 0x804)]
    win = rd.read_window(10_000)
    lift = eng.liftover_batch_host(win.batch_desc())
    data, off, n_lift, _ = win.build_records(lift, ixd, rd.ref_names, ph.ref_names)
    # (against phase 1's index: with the N runs at the contigs' joins, the joiner may merge neighbouring segments of the workload)
    res = oracle.liftover_batch(ix, win.batch_data(), abi.STAGES_ALL, 4)
    exp = expected_records(prim, ix, m2["contig_names"], m1["ref_names"], res)
    assert n_lift > 400
    assert [data[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)] == exp
    win.close()
    rd.close()
    ph.close()
    eng.close()
    index.close()
