"""NM:i of the lifted records counted on the device (plo_nm_dev, portello_amd/csrc/nm_core.hpp) and written by plo_records_build_dev.

The yardstick is plo_records_build on the same window (the host builder writes no NM) plus tests/nm_expect.py, a restatement of samtools
calmd's rule over an output record's own bytes: neither touches the code under test.  All comparisons are of integers and bytes.  The CPU
tests run nm_core.hpp and records_core.hpp under the wave emulator (tests/emu/emu_nm.cpp), with shuffled lane and item orders, and the
hand-made cases once more in a program built with AddressSanitizer + UBSan where every array sits in a heap block of its exact size; the
GPU tests run the C ABI on the device and the pipeline mode."""
import struct

import numpy as np
import pytest

import emu_nm_lib as enl
import emu_records_lib as erl
import nm_expect as nx
import test_records_dev as trd
from portello_amd import abi, api, bam, bamsynth, synth
from portello_amd import cigar as cg

SMALL_SEED = 411  # the small_bam recipe of tests/test_records_dev.py; test_small_bam_items asserts that the sample is not vacuous


@pytest.fixture(scope="module")
def small_bam(tmp_path_factory):
    d = tmp_path_factory.mktemp("nmdev")
    w = synth.generate(synth.config("tiny", n_reads=300, seed=SMALL_SEED, split_read_frac=0.3, sorted_reads=True))
    path = str(d / "reads.bam")
    meta = bamsynth.write_read_bam(w, path, level=6, n_unmapped=4)
    return w, path, meta


def lifted_records(recs):
    """the lifted records among a window's output records (the unmapped copies carry flag 0x4), in order = the LIFTED items in item order"""
    return [r for r in recs if not struct.unpack_from("<H", r, 18)[0] & 4]


def expected_nm(lift, recs, chroms):
    """nm_expect over the host builder's records -> [n_items] (0 for items that are not LIFTED), the bases compared"""
    want = np.zeros(lift.n_items, np.uint32)
    lr = lifted_records(recs)
    idx = np.flatnonzero(lift.item_status == abi.ITEM_LIFTED)
    assert len(lr) == len(idx)
    n_cmp = 0
    for i, r in zip(idx, lr):
        tid, pos, _, ops, codes = nx.record_alignment(r)
        assert tid == int(lift.item_chrom_index[i]) and pos == int(lift.item_ref_pos[i])
        want[i], c = nx.nm_counts(ops, codes, chroms[tid], pos)
        n_cmp += c
    return want, n_cmp


def with_nm(recs, item_nm, lift):
    """the host builder's records with NM:i spliced behind ZM:C of every lifted one -> (records, record_off)"""
    vals = iter(int(item_nm[i]) for i in np.flatnonzero(lift.item_status == abi.ITEM_LIFTED))
    out = [r if struct.unpack_from("<H", r, 18)[0] & 4 else nx.splice_nm(r, next(vals)) for r in recs]
    off = np.zeros(len(out) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in out])
    return out, off


class Emulated:
    """a window lifted by `lift`, finished under the emulator; the host builder's records of it"""

    def __init__(self, win, ix, lift, cn, rn, target=False):
        import dataclasses

        self.ix, self.lift, self.cn, self.target = ix, lift, cn, target
        self.rw = trd.RawWindow(win)
        rw = self.rw
        self.vb = dataclasses.replace(rw.batch, seq=rw.raw, read_seq_off=np.ascontiguousarray(rw.seq_off, np.uint64), seq_fmt=abi.SEQ_BAM4)
        self.f = erl.emu_lib.finish_batch(self.vb, rw.flags, rw.raw, rw.qual_off, lift)
        self.sa_off, self.sa_text, _ = erl.emu_lib.sa_segments(self.vb, lift, self.f["item_flag"], self.f["read_n_lifted"], rn)
        hdata, self.hoff, self.hnl, self.hnu = trd.host_records(win, ix, lift, cn, rn, target)
        self.hdata = hdata
        self.host = trd._split(hdata, self.hoff)

    def nm(self, order_seed=0, item_seed=0):
        return enl.nm_batch(self.ix, self.vb, self.lift, self.f["item_seq_off"], self.f["rev_seq"], order_seed, item_seed)

    def records(self, item_nm, vec=True, nthreads=7, order_seed=0):
        return enl.records_with_nm(self.ix, self.vb, self.rw.raw, self.rw.rec_off, self.lift, self.f, self.sa_off, self.sa_text, self.cn, item_nm, self.target, vec,
                                   nthreads, order_seed)


def check_records(em: Emulated, item_nm, **kw):
    """4. records_core.hpp with item_nm = the host builder + splice; without = the host builder byte for byte"""
    want, woff = with_nm(em.host, item_nm, em.lift)
    st, data, off, nl, nu = em.records(item_nm, **kw)
    assert st == 0 and (nl, nu) == (em.hnl, em.hnu) and np.array_equal(off, woff)
    for i, (a, e) in enumerate(zip(trd._split(data, off), want)):
        assert a == e, (i, a[-60:], e[-60:])
    assert data == b"".join(want)
    st, data, off, nl, nu = em.records(None, **kw)
    assert st == 0 and data == em.hdata and np.array_equal(off, em.hoff) and (nl, nu) == (em.hnl, em.hnu)
    return want


# ---- 1. the small_bam recipe ----------------------------------------------------------------------------------------------------------

def test_small_bam_items(small_bam, oracle):
    w, path, meta = small_bam
    ix = w.index_data()
    rd, win = trd.open_window(path)
    lift = oracle.liftover_batch(ix, win.batch_data(), abi.STAGES_ALL, 2)
    em = Emulated(win, ix, lift, meta["contig_names"], bamsynth.ref_names(w))
    want, n_cmp = expected_nm(lift, em.host, ix.chrom_seq)
    for order_seed, item_seed in ((0, 0), (7, 3)):  # the ticket loop in lane order; shuffled lanes, shuffled items
        st, got, cmp_, err = em.nm(order_seed, item_seed)
        assert st == abi.PLO_OK and err == 0xFFFFFFFF
        bad = np.flatnonzero(got != want)
        assert not len(bad), (order_seed, item_seed, bad[:10], got[bad[:10]], want[bad[:10]])
        assert cmp_ == n_cmp
    # the sample is not vacuous
    lifted = np.flatnonzero(lift.item_status == abi.ITEM_LIFTED)
    assert len(lifted) > 100
    assert (em.f["item_seq_off"][lifted] != abi.NO_FLIP).any(), "no flipped item"
    has = lambda i, t: any((int(c) & 15) == t for c in lift.cigar[int(lift.item_cigar_off[i]):int(lift.item_cigar_off[i]) + int(lift.item_cigar_len[i])])
    assert any(has(i, 1) for i in lifted), "no item with an insertion"
    assert any(has(i, 2) for i in lifted), "no item with a deletion"
    assert any(want[i] > 0 and (has(i, 0) or has(i, 7)) for i in lifted), "no item with NM > 0 and matching stretches"
    # 4. the records
    check_records(em, want)
    check_records(em, want, vec=False, nthreads=3, order_seed=9)
    win.close()
    rd.close()


# ---- 2. hand-made items ---------------------------------------------------------------------------------------------------------------

ACGT = np.frombuffer(b"ACGT", np.uint8)
IUPAC_REF = np.frombuffer(nx.TABLE + b"nZ\x00\xff", np.uint8)


def near(ref_bytes, rng, rate=0.1):
    """4-bit codes that agree with the reference bytes but for `rate` of the positions"""
    c = nx.CODE_OF[ref_bytes].copy()
    m = rng.random(len(c)) < rate
    c[m] = rng.integers(0, 16, int(m.sum()), dtype=np.uint8)
    return c


def hand_cases():
    rng = np.random.default_rng(12)
    ref = ACGT[rng.integers(0, 4, 3000)].copy()
    ref[rng.integers(0, 3000, 40)] = ord("N")
    out = []
    M = lambda s: np.array(cg.encode(s), np.uint32)
    # one M of every length around the 16-base pieces and the 8-byte words, at an odd reference position
    for l in (1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1025):
        out.append(enl.Case(f"{l}M", M(f"{l}M"), near(ref[5:5 + l], rng), ref, 5, front=l % 8))
    # a match that starts on an odd read position, on every reference residue; the bases on every residue of their 8-byte words
    for p in range(16):
        codes = np.concatenate([[3], near(ref[p:p + 200], rng)]).astype(np.uint8)
        out.append(enl.Case(f"1S200M@{p}", M("1S200M"), codes, ref, p, front=p % 8))
    for front in range(8):
        out.append(enl.Case(f"front{front}", M("77M"), near(ref[32:32 + 77], rng), ref, 32, front=front))
    # a flipped item with odd l_seq (its bases come from the finishing's buffer)
    out.append(enl.Case("flipped 77", M("2S75M"), np.concatenate([[1, 2], near(ref[100:175], rng)]).astype(np.uint8), ref, 100, flip=True))
    # 200 alternating 1M1I / 1M1D ops
    ops = np.array(list(cg.encode("1M1I")) * 50 + list(cg.encode("1M1D")) * 50, np.uint32)
    out.append(enl.Case("1M1I 1M1D", ops, rng.integers(0, 16, 150, dtype=np.uint8), ref, 9))
    # only S and I
    out.append(enl.Case("S + I", M("5S10I3S"), rng.integers(0, 16, 18, dtype=np.uint8), ref, 40))
    # a reference skip
    codes = np.concatenate([near(ref[7:57], rng), near(ref[1057:1107], rng)])
    out.append(enl.Case("N op", M("50M1000N50M"), codes, ref, 7))
    # = and X, H and P
    out.append(enl.Case("= X", M("3H30=1X40=2X1P20="), near(ref[11:104], rng), ref, 11))
    # more than 65535 ops (the recipe of test_more_than_65535_cigar_ops): 1M1I ... 1M
    long_ref = ACGT[rng.integers(0, 4, 35_040)].copy()
    codes = rng.integers(1, 9, 70_001, dtype=np.uint8)
    out.append(enl.Case("70001 ops", trd.long_cigar(70_001), codes, long_ref, 17))
    # an item that ends exactly at chrom_len
    out.append(enl.Case("ends at chrom_len", M("10S300M5D100M"), np.concatenate([np.zeros(10, np.uint8), near(ref[2595:2895], rng), near(ref[2900:3000], rng)]), ref, 2595))
    # every code against N, IUPAC letters, lower case and bytes outside the table
    n = len(IUPAC_REF)
    iu_ref = np.tile(IUPAC_REF, 16)
    iu_codes = np.repeat(np.arange(16, dtype=np.uint8), n)
    for p in (0, 3):
        out.append(enl.Case(f"iupac@{p}", M(f"{16 * n - p}M"), iu_codes[p:], iu_ref, p))
    # the op search over several trips with many ops per trip: two steps of 64 ops, some three pieces for each of a step's 32 M ops
    codes = np.concatenate([np.concatenate([near(ref[5 + 40 * i:45 + 40 * i], rng), rng.integers(0, 16, 1, dtype=np.uint8)]) for i in range(64)])
    out.append(enl.Case("40M1I x 64", np.array(list(cg.encode("40M1I")) * 64, np.uint32), codes, ref, 5))
    # the same with D ops between the matches (MD deals their pieces too)
    codes = np.concatenate([near(ref[11 + 19 * i:28 + 19 * i], rng) for i in range(40)])
    out.append(enl.Case("17M2D x 40", np.array(list(cg.encode("17M2D")) * 40, np.uint32), codes, ref, 11))
    return out


def refusal_cases():
    rng = np.random.default_rng(13)
    ref = ACGT[rng.integers(0, 4, 500)].copy()
    M = lambda s: np.array(cg.encode(s), np.uint32)
    codes = rng.integers(0, 16, 300, dtype=np.uint8)
    return [enl.Case("one past chrom_len", M("300M"), codes, ref, 201), enl.Case("one past chrom_len, D", M("100M200D1M"), codes[:101], ref, 200),
            enl.Case("one past chrom_len, far", M("100M"), codes[:100], ref, 401), enl.Case("pos behind chrom_len", M("1M"), codes[:1], ref, 501),
            enl.Case("one read base too many", M("200M101I"), codes, ref, 0), enl.Case("one read base too many, M", M("150S151M"), codes, ref, 0),
            enl.Case("too many in a later step", np.array(list(cg.encode("1M1I")) * 150 + list(cg.encode("1M")), np.uint32), codes, ref, 0)]


def test_rule_by_hand():
    code = {ch: i for i, ch in enumerate(nx.TABLE.decode())}
    one = lambda c, r: nx.nm_slow(cg.encode("1M"), np.array([c], np.uint8), np.frombuffer(r, np.uint8), 0)
    assert one(code["N"], b"N") == 1 and one(code["R"], b"R") == 0 and one(0, b"A") == 0 and one(0, b"#") == 0
    assert one(code["A"], b"A") == 0 and one(code["A"], b"a") == 1 and one(code["A"], b"C") == 1 and one(code["A"], b"=") == 1 and one(code["N"], b"#") == 1


def test_hand_made_items(tmp_path):
    cases = hand_cases()
    want = []
    for c in cases:
        nm, n_cmp = nx.nm_counts(c.ops, c.codes, c.ref, c.pos)
        if len(c.ops) < 1000:
            assert nm == nx.nm_slow(c.ops, c.codes, c.ref, c.pos), c.name
        want.append((abi.PLO_OK, nm, n_cmp))
        for seed in ((0, 5) if len(c.ops) < 1000 else (0,)):  # (the sanitizer program below runs every case with shuffled lanes)
            assert enl.nm_one(c, seed) == want[-1], (c.name, seed)
    assert sum(1 for w in want if 0 < w[1] < w[2]) > 20  # matches and mismatches side by side
    # 3. refusals: nothing counted, PLO_ERR_RANGE
    bad = refusal_cases()
    for c in bad:
        with pytest.raises(IndexError):
            nx.nm_counts(c.ops, c.codes, c.ref, c.pos)
        for seed in (0, 5):
            assert enl.nm_one(c, seed)[0] == abi.PLO_ERR_RANGE, c.name
    # all of them once more under AddressSanitizer + UBSan, every array in a heap block of its exact size
    rc, err_text, res = enl.run_asan(cases + bad, str(tmp_path), order_seed=3)
    assert rc == 0, err_text[-3000:]
    assert [tuple(r) for r in res[:len(cases)]] == want
    assert all(r[0] == abi.PLO_ERR_RANGE for r in res[len(cases):])


def real_hand_index(seed=21):
    """trd.hand_index with bases on its two chromosomes"""
    rng = np.random.default_rng(seed)
    ix = trd.hand_index()
    ix.chrom_seq = [ACGT[rng.integers(0, 4, 4000)].copy() for _ in range(2)]
    return ix


def test_refusal_names_the_lowest_item(tmp_path):
    lens = [40, 41, 42, 43, 44, 45]
    recs = [trd.make_record(k, l) for k, l in enumerate(lens)]
    rd, win = trd.write_window(tmp_path, recs)
    ix = real_hand_index()
    M = lambda s: cg.encode(s)
    L = abi.ITEM_LIFTED
    # item 2: one base past chrom_len; item 3 (flipped): one read base too many; item 4: both; items 0, 1, 5: fine (5 ends at chrom_len)
    items = [(0, 0, L, 0, 50, 0, 100, M("40M")), (1, 0, L, 0, 50, 0, 3000, M("41M")), (2, 0, L, 0, 50, 0, 3959, M("42M")), (3, 1, L, 1, 20, 1, 10, M("43M1I")),
             (4, 0, L, 0, 50, 0, 3990, M("45M")), (5, 0, L, 0, 50, 0, 3955, M("45M"))]
    em = Emulated(win, ix, trd.hand_lift(items), trd.CN, trd.RN)
    for order_seed, item_seed in ((0, 0), (4, 9), (1, 2)):
        st, _, _, err = em.nm(order_seed, item_seed)
        assert st == abi.PLO_ERR_RANGE and err == 2
    win.close()
    rd.close()


def test_records_with_more_than_65535_ops_and_a_second_record(tmp_path):
    """NM:i sits behind ZM:C and in front of SA:Z and CG:B,I; a read whose items are not all LIFTED; an unmapped copy without NM"""
    from oracle import pyrecords as pr

    n = 70_001
    cig = trd.long_cigar(n)
    rng = np.random.default_rng(5)
    sp = rng.integers(0, 256, (n + 1) // 2, dtype=np.uint8)
    sp[-1] &= 0xF0
    src = pr.Record(0, 10, 60, 0, 0, -1, -1, 0, b"long", [int(x) for x in cig], sp.tobytes(), n, bytes(n), [(b"rq", b"f" + struct.pack("<f", 1.0)), (b"NM", b"C\x07")])
    rd, win = trd.write_window(tmp_path, [src.to_bytes(), trd.make_record(1, 33, aux=b"ZMC\x05XXZkeep\0"), trd.make_record(2, 20), trd.make_record(3, 21, flag=0x10)])
    ix = trd.hand_index()
    rng = np.random.default_rng(6)
    ix.chrom_seq = [ACGT[rng.integers(0, 4, 36_000)].copy() for _ in range(2)]
    ix.chrom_len = np.array([36_000, 36_000], np.int64)
    L = abi.ITEM_LIFTED
    lift = trd.hand_lift([(0, 0, L, 0, 50, 0, 77, cig), (0, 1, L, 1, 20, 1, 99, cig), (1, 0, L, 0, 50, 0, 5, cg.encode("33M")), (1, 1, abi.ITEM_NO_LIFTOVER, 0, 0, 0, 0, []),
                          (2, 0, abi.ITEM_NO_LIFTOVER, 0, 0, 0, 0, []), (3, 1, L, 1, 20, 1, 35_979, cg.encode("21M"))])
    em = Emulated(win, ix, lift, trd.CN, trd.RN)
    want, _ = expected_nm(lift, em.host, ix.chrom_seq)
    st, got, _, _ = em.nm(3, 5)
    assert st == abi.PLO_OK and np.array_equal(got, want) and want[3] == want[4] == 0 and want[0] > 35_000
    recs = check_records(em, want)
    check_records(em, want, vec=False)
    assert len(recs) == 5 and struct.unpack_from("<H", recs[3], 18)[0] & 4 and b"NMi" not in recs[3][-40:]
    tags = [t for _, _, t, _ in nx.aux_fields(recs[0])]
    assert tags[-4:] == [b"ZM", b"NM", b"SA", b"CG"] and b"NMC\x07" not in recs[0], tags
    assert [t for _, _, t, _ in nx.aux_fields(recs[2])][-2:] == [b"ZM", b"NM"]
    for r, i in ((recs[0], 0), (recs[1], 1), (recs[2], 2), (recs[4], 5)):
        assert nx.strip_nm(r)[1] == [int(want[i])]
    win.close()
    rd.close()


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------

def device_nm(run):
    no = run.eng.nm_dev(run.ddesc)
    return run.eng.download(no.item_nm, np.uint32, int(no.n_items)), no


def check_device_records(run, win, ixd, cn, rn, item_nm, lift, target=False):
    """plo_records_build_dev = the host builder (+ splice when item_nm is given)"""
    rec = run.records()
    hdata, hoff, hnl, hnu = trd.host_records(win, ixd, lift, cn, rn, target)
    host = trd._split(hdata, hoff)
    want, woff = with_nm(host, item_nm, lift) if item_nm is not None else (host, hoff)
    assert rec.n_records == len(want) and (rec.n_lifted, rec.n_unmapped_copies) == (hnl, hnu)
    assert np.array_equal(rec.record_off, woff)
    data = rec.data()
    for i, (a, e) in enumerate(zip(trd._split(data, rec.record_off), want)):
        assert a == e, (i, a[-60:], e[-60:])
    assert data == b"".join(want)
    return host


@pytest.mark.gpu
def test_device_nm_and_records_of_the_small_bam(small_bam):
    """5. item_nm and n_cmp_bases of plo_nm_dev; 8. the records behind it carry NM:i, the same context's next batch without plo_nm_dev
    equals the host builder exactly"""
    w, path, meta = small_bam
    ixd = w.index_data()
    index = api.Index(ixd, 0)
    cn, rn = meta["contig_names"], bamsynth.ref_names(w)
    rd, win = trd.open_window(path)
    run = trd.DeviceRun(win, index, cn, rn, False)
    run.finish()
    run.sa()
    lift = run.lift_result()
    hdata, hoff, _, _ = trd.host_records(win, ixd, lift, cn, rn, False)
    want, n_cmp = expected_nm(lift, trd._split(hdata, hoff), ixd.chrom_seq)
    got, no = device_nm(run)
    bad = np.flatnonzero(got != want)
    assert not len(bad), (bad[:10], got[bad[:10]], want[bad[:10]])
    assert int(no.n_cmp_bases) == n_cmp and int(no.err_item) == 0xFFFFFFFF and no.nm_ms > 0
    assert (want > 0).any()  # (every item of this sample is LIFTED; an item that is not is among the hand-made ones below)
    host = check_device_records(run, win, ixd, cn, rn, want, lift)
    assert sum(1 for r in host if struct.unpack_from("<H", r, 18)[0] & 4) > 0  # (unmapped copies: no NM on them)
    # the next batch on the same context, without plo_nm_dev: today's bytes
    run.out = run.eng.liftover_batch_dev(run.ddesc)
    run.eng.compact_output_dev(run.out)
    run.finish()
    run.sa()
    check_device_records(run, win, ixd, cn, rn, None, run.lift_result())
    run.eng.close()
    win.close()
    rd.close()
    index.close()


def one_to_one_index(chrom, contig_len, seg_pos):
    return abi.IndexData(contig_len=np.array([contig_len]), contig_seg_off=np.array([0, 1], np.uint32), seg_chrom_index=np.zeros(1, np.uint32),
                         seg_pos=np.array([seg_pos]), seg_is_fwd_strand=np.ones(1, np.uint8), seg_mapq=np.array([33], np.uint8),
                         seg_seq_order_start=np.zeros(1), seg_seq_order_end=np.array([contig_len]), seg_cigar_off=np.array([0, 1], np.uint32),
                         seg_cigar=np.array(cg.encode(f"{contig_len}="), np.uint32), chrom_seq=[chrom], rev_contig_seq=[None])


def case_record(k, c, pos):
    ops = c.ops[~np.isin(c.ops & 15, (5, 6))]  # (H and P stay with the emulated cases: the lift's length check refuses the read)
    if len(ops) > 65535:
        from oracle import pyrecords as pr
        return pr.Record(0, pos, 60, 0, 0, -1, -1, 0, b"r%d" % k, [int(x) for x in ops], c.packed().tobytes(), c.l_seq, bytes(c.l_seq), []).to_bytes()
    return bamsynth.encode_record(0, pos, 37, 0, b"r%d" % k, ops, c.packed().tobytes(), c.l_seq, bytes(c.l_seq), b"XXZkeep\0")


def hand_window(tmp_path):
    """the hand-made cases as reads of one BAM: -> (index, path, cases)"""
    SEG_POS = 37
    cases = [c for c in hand_cases() if not c.flip]
    # one chromosome: the cases' references side by side, every case at its own position in its own stretch
    starts, parts, at = [], [ACGT[np.zeros(64, np.int64)]], 64
    for c in cases:
        starts.append(at)
        parts.append(c.ref)
        at += len(c.ref)
    chrom = np.concatenate(parts + [ACGT[np.zeros(64, np.int64)]])
    ixd = one_to_one_index(chrom, len(chrom) - SEG_POS, SEG_POS)
    recs, order = [], sorted(range(len(cases)), key=lambda k: starts[k] + cases[k].pos)
    for k in order:
        p = starts[k] + cases[k].pos - SEG_POS
        assert p >= 0
        recs.append(case_record(k, cases[k], p))
    path = str(tmp_path / "hand.bam")
    wr = bam.BamWriter(path, "@HD\tVN:1.6\n", trd.CN, [len(chrom) - SEG_POS], level=1)
    wr.write(b"".join(recs))
    wr.close()
    return ixd, path, cases


@pytest.mark.gpu
def test_device_hand_made_items(tmp_path):
    """6. the hand-made items in one batch through the C ABI: the contig is the chromosome from SEG_POS on, base for base, so a read's
    CIGAR against the contig is lifted onto the chromosome as the lift stages leave it -- whatever they make of it, NM is nm_expect's over
    the host builder's record"""
    ixd, path, cases = hand_window(tmp_path)
    index = api.Index(ixd, 0)
    rd, win = trd.open_window(path)
    assert win.n_records == len(cases)
    run = trd.DeviceRun(win, index, trd.CN, ["chr1"], False)
    run.finish()
    run.sa()
    lift = run.lift_result()
    lifted = lift.item_status == abi.ITEM_LIFTED
    assert lifted.sum() == len(cases) - 1 and int(lift.item_cigar_len.max()) > 65535  # (the read of S and I alone has nothing to lift: its item is not LIFTED, NM 0)
    hdata, hoff, _, _ = trd.host_records(win, ixd, lift, trd.CN, ["chr1"], False)
    want, n_cmp = expected_nm(lift, trd._split(hdata, hoff), ixd.chrom_seq)
    got, no = device_nm(run)
    bad = np.flatnonzero(got != want)
    assert not len(bad), (bad[:10], got[bad[:10]], want[bad[:10]])
    assert int(no.n_cmp_bases) == n_cmp and (want > 0).sum() > 20 and not got[~lifted].any()
    check_device_records(run, win, ixd, trd.CN, ["chr1"], want, lift)
    run.eng.close()
    win.close()
    rd.close()
    index.close()


class Steps:
    """lift -> compact -> finish of several windows on ONE context"""

    def __init__(self, index):
        import torch

        self.dev = torch.device("cuda", 0)
        self.eng = api.Engine(index)

    def lift(self, win, stages=abi.STAGES_ALL, finish=True):
        import torch

        from portello_amd import devbatch
        b, f, r = win.batch_raw()
        self.up = devbatch.upload_raw_window(b, f, r, self.dev)
        torch.cuda.synchronize()
        self.ddesc = self.up.batch.desc()
        self.out = self.eng.liftover_batch_dev(self.ddesc, stages)
        self.eng.compact_output_dev(self.out)
        if finish:
            self.eng.finish_batch_dev(self.ddesc, self.up.finish_in())
        return devbatch.download(self.eng, self.out)


@pytest.mark.gpu
def test_device_nm_refusals(small_bam, tmp_path):
    """7. out of order and sparse: PLO_ERR_INVALID_ARG; a CIGAR past the chromosome's end: PLO_ERR_RANGE with err_item, by a check -- the
    context lifts the next batch correctly"""
    import torch

    from portello_amd import devbatch
    w, path, meta = small_bam
    rd, win = trd.open_window(path)
    index = api.Index(w.index_data(), 0)
    st = Steps(index)
    b, f, r = win.batch_raw()
    up = devbatch.upload_raw_window(b, f, r, st.dev)
    torch.cuda.synchronize()
    with pytest.raises(api.PortelloError, match="no lift result") as e:
        st.eng.nm_dev(up.batch.desc())
    assert e.value.status == abi.PLO_ERR_INVALID_ARG
    st.lift(win, finish=False)
    with pytest.raises(api.PortelloError, match="no finishing result") as e:
        st.eng.nm_dev(st.ddesc)
    assert e.value.status == abi.PLO_ERR_INVALID_ARG
    sp = bam.sparse_pack(win.batch_data())
    db = devbatch.DeviceBatch.from_batch_data(sp, st.dev)
    torch.cuda.synchronize()
    sdesc = db.desc()
    st.eng.liftover_batch_dev(sdesc)
    with pytest.raises(api.PortelloError, match="sparse") as e:
        st.eng.nm_dev(sdesc)
    assert e.value.status == abi.PLO_ERR_INVALID_ARG
    st.eng.close()
    win.close()
    rd.close()
    index.close()
    # a contig that maps 1:1 onto the chromosome but is 50 bases longer than the chromosome has room for: the reads on its end lift to
    # CIGARs that run past chrom_len.  (Strand and liftover stages only: no stage of the lift looks at the chromosome's bases.)
    SEG_POS, C = 100, 3000
    rng = np.random.default_rng(31)
    chrom = ACGT[rng.integers(0, 4, C)].copy()
    ixd = one_to_one_index(chrom, C - SEG_POS + 50, SEG_POS)
    assert len(ixd.chrom_seq[0]) == C
    stages = abi.STAGE_STRAND | abi.STAGE_LIFTOVER | abi.STAGE_LENCHECK

    def window_of(name, starts, l=60):
        recs = [bamsynth.encode_record(0, p, 37, 0, b"q%d" % k, np.array(cg.encode(f"{l}M"), np.uint32), rng.integers(0, 256, l // 2, dtype=np.uint8).tobytes(), l, bytes(l), b"")
                for k, p in enumerate(starts)]
        pth = str(tmp_path / name)
        wr = bam.BamWriter(pth, "@HD\tVN:1.6\n", trd.CN, [C - SEG_POS + 50], level=1)
        wr.write(b"".join(recs))
        wr.close()
        return trd.open_window(pth)

    inside = C - SEG_POS - 60  # a read that starts here ends exactly at chrom_len
    rd_a, win_a = window_of("past.bam", [10, 500, inside, inside + 1, inside + 30])
    rd_b, win_b = window_of("inside.bam", [10, 500, inside - 7, inside])
    index = api.Index(ixd, 0)
    st = Steps(index)
    lift = st.lift(win_a, stages)
    assert (lift.item_status == abi.ITEM_LIFTED).all() and lift.n_items == 5
    ends = lift.item_ref_pos + np.array([sum(int(c) >> 4 for c in lift.item_cigar(i)) for i in range(5)])
    assert list(ends > C) == [False, False, False, True, True] and int(ends[2]) == C
    with pytest.raises(api.PortelloError, match="consumes more reference") as e:
        st.eng.nm_dev(st.ddesc)
    assert e.value.status == abi.PLO_ERR_RANGE and e.value.err_item == 3
    # the next batch on the same context
    lift = st.lift(win_b, stages)
    hdata, hoff, _, _ = trd.host_records(win_b, ixd, lift, trd.CN, ["chr1"], False)
    want, n_cmp = expected_nm(lift, trd._split(hdata, hoff), ixd.chrom_seq)
    no = st.eng.nm_dev(st.ddesc)
    assert np.array_equal(st.eng.download(no.item_nm, np.uint32, int(no.n_items)), want) and int(no.n_cmp_bases) == n_cmp == 4 * 60
    st.eng.close()
    for x in (win_a, rd_a, win_b, rd_b):
        x.close()
    index.close()


@pytest.mark.gpu
def test_bam_to_bam_with_nm(tmp_path):
    """9. run_bam_to_bam(device_records=True, device_batch=True, emit_nm=True) on a 2 000-read synthetic BAM"""
    from oracle import expect
    from portello_amd import pipeline

    w = synth.generate(synth.config("chr20", n_reads=2_000), device="cuda")
    inp, unp = str(tmp_path / "reads.bam"), str(tmp_path / "unassembled.bam")
    meta = bamsynth.write_read_bam(w, inp, level=1, n_threads=8)
    ixd = w.index_data()
    index = api.Index(w.index_data_device())
    cn, rn = meta["contig_names"], bamsynth.ref_names(w)
    lens = [int(s.numel()) for s in w.chrom_seq]
    with pytest.raises(ValueError, match="device_records"):
        pipeline.run_bam_to_bam(inp, str(tmp_path / "x.bam"), index, ixd, cn, rn, lens, emit_nm=True)
    kw = dict(window_reads=700, n_workers=2, io_threads=8, device_records=True)
    outs = {}
    for name, extra in (("nm", dict(device_batch=True, emit_nm=True, unassembled_path=unp)), ("off", dict(device_batch=True, emit_nm=False)), ("plain", dict())):
        outp = str(tmp_path / f"{name}.bam")
        st = pipeline.run_bam_to_bam(inp, outp, index, ixd, cn, rn, lens, **kw, **extra)
        assert st.reads == w.n_reads
        outs[name] = (outp, st)
    assert outs["nm"][1].nm_device_ms > 0 and outs["nm"][1].lift_detail_s.get("nm", 0) > 0
    assert outs["off"][1].nm_device_ms == 0 and "nm" not in outs["off"][1].lift_detail_s

    import bamcheck

    records_of = lambda path: bamcheck.read_bam(path)[2]

    # emit_nm=False gives the file of the parent commit's route: the same records as device_records=True alone (windows may leave in
    # another order: the records are compared as sorted lists)
    off_recs, plain_recs = records_of(outs["off"][0]), records_of(outs["plain"][0])
    assert sorted(off_recs) == sorted(plain_recs) and len(off_recs) == outs["off"][1].records_out
    # every lifted record carries exactly one NM:i = nm_expect; unmapped copies carry none; without the field the records are the others'
    nm_recs = records_of(outs["nm"][0])
    assert len(nm_recs) == len(off_recs) == outs["nm"][1].records_out
    chroms = ixd.chrom_seq
    stripped, n_lifted, n_pos = [], 0, 0
    for r in nm_recs:
        bare, vals = nx.strip_nm(r)
        stripped.append(bare)
        if struct.unpack_from("<H", r, 18)[0] & 4:
            assert vals == []
            continue
        n_lifted += 1
        assert vals == [nx.nm_of_record(bare, chroms)]
        n_pos += vals[0] > 0
        tags = [t for _, _, t, _ in nx.aux_fields(r)]
        assert tags[tags.index(b"NM") - 1] == b"ZM"
    assert n_lifted == outs["nm"][1].lifted > 1000 and n_pos > 0
    assert sorted(stripped) == sorted(off_recs)
    # with the field removed the file passes the existing record comparison
    bare_path = str(tmp_path / "bare.bam")
    wr = bam.BamWriter(bare_path, bam.output_header(rn, lens), rn, lens, level=1)
    wr.write(b"".join(stripped))
    wr.close()
    v = expect.verify_lifted_bam(inp, [bare_path], ixd, cn, rn, window=1000, every=1, threads=8, unassembled_bam=unp)
    assert v["ok"] and v["reads_verified"] == w.n_reads and v["records_verified"] == outs["nm"][1].records_out == v["records_in_output"], v
    index.close()
