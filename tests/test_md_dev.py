"""MD:Z of the lifted records written on the device (plo_md_dev, portello_amd/csrc/md_core.hpp) and put into the records by
plo_records_build_dev, which then also cuts the MD the source record carried.

The yardstick is plo_records_build on the same window (the host builder writes no MD and cuts none) plus tests/md_expect.py, a restatement
of samtools calmd's rule over an output record's own bytes: neither touches the code under test.  All comparisons are of integers and
bytes.  The CPU tests run md_core.hpp and records_core.hpp under the wave emulator (tests/emu/emu_md.cpp), with shuffled lane and item
orders, and the hand-made cases once more in a program built with AddressSanitizer + UBSan where every array sits in a heap block of its
exact size; the GPU tests run the C ABI on the device and the pipeline mode."""
import re
import struct

import numpy as np
import pytest

import emu_md_lib as eml
import emu_nm_lib as enl
import md_expect as mx
import nm_expect as nx
import test_nm_dev as tnd
import test_records_dev as trd
from portello_amd import abi, api, bam, bamsynth, synth
from portello_amd import cigar as cg

# the small_bam recipe of tests/test_nm_dev.py.  Seed 411 holds all four kinds of item test_small_bam_items asks for (a flipped item, a text
# with '^', one with 0 between two letters, one with a number of three or more digits): the test asserts it.
SMALL_SEED = 411
ACGT = tnd.ACGT


@pytest.fixture(scope="module")
def small_bam(tmp_path_factory):
    d = tmp_path_factory.mktemp("mddev")
    w = synth.generate(synth.config("tiny", n_reads=300, seed=SMALL_SEED, split_read_frac=0.3, sorted_reads=True))
    path = str(d / "reads.bam")
    meta = bamsynth.write_read_bam(w, path, level=6, n_unmapped=4)
    return w, path, meta


def is_unmapped(rec):
    return bool(struct.unpack_from("<H", rec, 18)[0] & 4)


def expected_md(lift, recs, chroms):
    """md_expect over the host builder's records -> (the texts [n_items], b"" for items that are not LIFTED; item_md_off [n_items + 1])"""
    texts = [b""] * lift.n_items
    lr = tnd.lifted_records(recs)
    idx = np.flatnonzero(lift.item_status == abi.ITEM_LIFTED)
    assert len(lr) == len(idx)
    for i, r in zip(idx, lr):
        tid, pos, _, ops, codes = nx.record_alignment(r)
        assert tid == int(lift.item_chrom_index[i]) and pos == int(lift.item_ref_pos[i])
        texts[i] = mx.md_text(ops, codes, chroms[tid], pos)
        assert mx.GRAMMAR.fullmatch(texts[i])
    off = np.zeros(lift.n_items + 1, np.uint64)
    off[1:] = np.cumsum([len(t) for t in texts])
    return texts, off


def with_tags(recs, lift, item_nm, texts):
    """the host builder's records as plo_records_build_dev writes them while the context holds an NM result (item_nm), an MD result (texts),
    both or neither (None): with an MD result the first source MD is cut from the lifted records and MD:Z stands behind ZM:C / NM:i
    -> (records, record_off)"""
    it = iter(np.flatnonzero(lift.item_status == abi.ITEM_LIFTED))
    out = []
    for r in recs:
        if not is_unmapped(r):
            i = int(next(it))
            if texts is not None:
                r = mx.cut_first_md(r)
            if item_nm is not None:
                r = nx.splice_nm(r, int(item_nm[i]))
            if texts is not None:
                r = mx.splice_md(r, texts[i])
        out.append(r)
    off = np.zeros(len(out) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in out])
    return out, off


def emu_md(em, order_seed=0, item_seed=0):
    return eml.md_batch(em.ix, em.vb, em.lift, em.f["item_seq_off"], em.f["rev_seq"], order_seed, item_seed)


def emu_records(em, item_nm, off, text, **kw):
    return eml.records_with_md(em.ix, em.vb, em.rw.raw, em.rw.rec_off, em.lift, em.f, em.sa_off, em.sa_text, em.cn, item_nm, off, text, em.target, **kw)


def check_records(em, item_nm, texts, off, **kw):
    """6. records_core.hpp under the emulator with an MD result only, with NM and MD, with neither, with NM only: byte for byte"""
    text = b"".join(texts)
    res = {}
    for name, nm, md in (("md", None, texts), ("both", item_nm, texts), ("neither", None, None), ("nm", item_nm, None)):
        want, woff = with_tags(em.host, em.lift, nm, md)
        st, data, roff, nl, nu = emu_records(em, nm, off if md is not None else None, text if md is not None else None, **kw)
        assert st == 0 and (nl, nu) == (em.hnl, em.hnu) and np.array_equal(roff, woff), name
        for i, (a, e) in enumerate(zip(trd._split(data, roff), want)):
            assert a == e, (name, i, a[-80:], e[-80:])
        assert data == b"".join(want), name
        res[name] = want
    assert b"".join(res["neither"]) == em.hdata
    assert res["nm"] == tnd.with_nm(em.host, item_nm, em.lift)[0]  # what tests/test_nm_dev.py expects
    return res


# ---- 1. the rule by hand --------------------------------------------------------------------------------------------------------------

CODE = {ch: i for i, ch in enumerate(nx.TABLE.decode())}


def by_hand(cigar, read, ref, pos=0):
    return enl.Case(cigar, np.array(cg.encode(cigar), np.uint32), np.array([CODE[c] for c in read], np.uint8), np.frombuffer(ref, np.uint8), pos)


def test_rule_by_hand():
    worked = [(by_hand("4M2D4M", "ACGATTAC", b"ACGTACGTAC"), b"3T0^AC0G3", 4), (by_hand("3M1I3M", "ACGTACG", b"ACGACG"), b"6", 1),
              (by_hand("5S2M100N2M", "TTTTTACGT", b"AC" + b"T" * 100 + b"GT"), b"4", 0),
              (by_hand("1M", "N", b"N"), b"0N0", 1), (by_hand("3M", "=A=", b"#AN"), b"3", 0),
              (by_hand("4M", "CCCC", b"a#\x00\xff"), b"0A0N0N0N0", 4), (by_hand("2M2D", "AC", b"ACg\x80"), b"2^GN0", 2)]
    for c, text, nm in worked:
        assert mx.md_text(c.ops, c.codes, c.ref, c.pos) == text == mx.md_slow(c.ops, c.codes, c.ref, c.pos), c.name
        assert nx.nm_counts(c.ops, c.codes, c.ref, c.pos)[0] == nm, c.name
        for seed in (0, 5):
            assert eml.md_one(c, seed) == (abi.PLO_OK, len(text), text), (c.name, seed)


# ---- 2. hand-made items ---------------------------------------------------------------------------------------------------------------

OTHER = np.zeros(16, np.uint8)
OTHER[[1, 2, 4, 8]] = [2, 4, 8, 1]  # A -> C -> G -> T -> A


def exact(ref_bytes, mismatches=()):
    """the codes of the reference's own letters (A, C, G, T only), another letter at the positions given"""
    c = nx.CODE_OF[ref_bytes].copy()
    for p in mismatches:
        c[p] = OTHER[c[p]]
    return c


def md_cases():
    """-> [(case, a pattern its text must match in full)], every one from explicit bases"""
    rng = np.random.default_rng(14)
    ref = ACGT[rng.integers(0, 4, 3000)].copy()
    long_ref = ACGT[rng.integers(0, 4, 100_100)].copy()
    M = lambda s: np.array(cg.encode(s), np.uint32)
    out = []

    def add(name, cigar, pos, mism, pattern, r=ref):
        ops = M(cigar) if isinstance(cigar, str) else cigar
        t, l = ops & 15, (ops >> 4).astype(np.int64)
        parts, at = [], pos  # the reference letters under the read, an A for every inserted or clipped base
        for tt, ll in zip(t, l):
            if tt in (0, 7, 8):
                parts.append(r[at:at + ll])
            elif tt in (1, 4):
                parts.append(ACGT[np.zeros(ll, np.int64)])
            if tt in (0, 2, 3, 7, 8):
                at += ll
        out.append((enl.Case(name, ops, exact(np.concatenate(parts), mism), r, pos), re.compile(pattern)))

    # mismatches in a row: 0 between the letters
    for k in (2, 3, 17):
        add(f"{k} in a row", "60M", 3, range(20, 20 + k), rb"20([A-Z]0){%d}[A-Z]%d" % (k - 1, 40 - k))
    # a mismatch as the first and as the last base of an op; the run closed at the item's end
    add("first and last of an op", "20M5I20M", 7, (0, 19, 25, 44), rb"0[A-Z]18[A-Z]0[A-Z]18[A-Z]0")
    # a mismatch directly behind a D (the run open at the item's end), a D directly behind a mismatch
    add("mismatch behind D", "10M3D10M", 5, (10,), rb"10\^[A-Z]{3}0[A-Z]9")
    add("D behind mismatch", "10M3D10M", 6, (9,), rb"9[A-Z]0\^[A-Z]{3}10")
    add("D I D", "10M2D3I2D10M", 8, (), rb"10\^[A-Z]{2}0\^[A-Z]{2}10")
    add("D N D", "10M2D50N2D10M", 9, (), rb"10\^[A-Z]{2}0\^[A-Z]{2}10")
    # a D of 1, 15, 16, 17 and 1025 bases starting on every residue of the reference's 16-byte lines
    for l in (1, 15, 16, 17, 1025):
        for p in range(16):
            add(f"{l}D@{p}", f"20M{l}D20M", p, (3,) if p & 1 else (), (rb"3[A-Z]16" if p & 1 else rb"20") + rb"\^[A-Z]{%d}20" % l)
    # a match run that crosses an I, an N and a 64-op step boundary
    add("run across I, N, a step", np.concatenate([np.tile(M("3M1I"), 40), M("5M50N5M")]), 11, (), rb"130")
    # runs of exactly so many matches, between two mismatches
    for run in (9, 10, 99, 100, 999, 1000, 9999, 10_000, 100_000):
        add(f"run of {run}", f"{run + 2}M", 13, (0, run + 1), rb"0[A-Z]%d[A-Z]0" % run, r=ref if run < 2900 else long_ref)
    return out


def all_cases():
    """test_nm_dev.hand_cases() and the cases above -> [(case, pattern or None)]"""
    return [(c, None) for c in tnd.hand_cases()] + md_cases()


def check_case(c, pattern, got, seed):
    st, ln, text = got
    want = mx.md_text(c.ops, c.codes, c.ref, c.pos)
    assert st == abi.PLO_OK, (c.name, seed, st)  # (-2: a store outside the item's slot, -3: a byte of it unwritten, -4: count and emit differ)
    assert ln == len(text) and text == want, (c.name, seed, text[:80], want[:80])


def test_hand_made_items(tmp_path):
    cases = all_cases()
    wants = []
    for c, pattern in cases:
        want = mx.md_text(c.ops, c.codes, c.ref, c.pos)
        assert want == mx.md_slow(c.ops, c.codes, c.ref, c.pos), c.name
        assert mx.GRAMMAR.fullmatch(want), c.name
        if pattern is not None:
            assert pattern.fullmatch(want), (c.name, want[:120])  # the case produces what it was made for
        # the letters of the text plus the inserted bases are the item's NM
        n_ins = int((c.ops >> 4)[(c.ops & 15) == 1].sum())
        assert mx.n_letters(want) + n_ins == nx.nm_counts(c.ops, c.codes, c.ref, c.pos)[0], c.name
        wants.append(want)
        for seed in ((0, 5) if len(c.ops) < 1000 and c.l_seq < 300 else (0,)):  # (the sanitizer program below runs every case with shuffled lanes)
            check_case(c, pattern, eml.md_one(c, seed), seed)
    by_name = {c.name: w for (c, _), w in zip(cases, wants)}
    assert by_name["S + I"] == b"0" and len(by_name["70001 ops"]) > 35_000 and b"^" in by_name["ends at chrom_len"] and by_name["flipped 77"] != b"75"
    # 3. refusals: PLO_ERR_RANGE, nothing written
    bad = tnd.refusal_cases()
    for c in bad:
        with pytest.raises(IndexError):
            mx.md_text(c.ops, c.codes, c.ref, c.pos)
        for seed in (0, 5):
            assert eml.md_one(c, seed) == (abi.PLO_ERR_RANGE, 0, b""), c.name
    # 4. all of them once more under AddressSanitizer + UBSan, every array (the text too) in a heap block of its exact size
    rc, err_text, res = eml.run_asan([c for c, _ in cases] + bad, str(tmp_path), order_seed=3)
    assert rc == 0, err_text[-3000:]
    assert res[:len(cases)] == [(abi.PLO_OK, w) for w in wants]
    assert res[len(cases):] == [(abi.PLO_ERR_RANGE, b"")] * len(bad)


def test_refusal_names_the_lowest_item(tmp_path):
    lens = [40, 41, 42, 43, 44, 45]
    recs = [trd.make_record(k, l) for k, l in enumerate(lens)]
    rd, win = trd.write_window(tmp_path, recs)
    ix = tnd.real_hand_index()
    M = lambda s: cg.encode(s)
    L = abi.ITEM_LIFTED
    # item 2: one base past chrom_len; item 3 (flipped): one read base too many; item 4: both; items 0, 1, 5: fine (5 ends at chrom_len)
    items = [(0, 0, L, 0, 50, 0, 100, M("40M")), (1, 0, L, 0, 50, 0, 3000, M("41M")), (2, 0, L, 0, 50, 0, 3959, M("42M")), (3, 1, L, 1, 20, 1, 10, M("43M1I")),
             (4, 0, L, 0, 50, 0, 3990, M("45M")), (5, 0, L, 0, 50, 0, 3955, M("45M"))]
    em = tnd.Emulated(win, ix, trd.hand_lift(items), trd.CN, trd.RN)
    for order_seed, item_seed in ((0, 0), (4, 9), (1, 2)):
        st, _, text, _, err = emu_md(em, order_seed, item_seed)
        assert st == abi.PLO_ERR_RANGE and err == 2 and text == b""
    win.close()
    rd.close()


# ---- 5. the small_bam recipe ----------------------------------------------------------------------------------------------------------

def test_small_bam_items(small_bam, oracle):
    w, path, meta = small_bam
    ix = w.index_data()
    rd, win = trd.open_window(path)
    lift = oracle.liftover_batch(ix, win.batch_data(), abi.STAGES_ALL, 2)
    em = tnd.Emulated(win, ix, lift, meta["contig_names"], bamsynth.ref_names(w))
    texts, off = expected_md(lift, em.host, ix.chrom_seq)
    for order_seed, item_seed in ((0, 0), (7, 3)):  # the ticket loop in lane order; shuffled lanes, shuffled items
        st, got_off, got_text, got_len, err = emu_md(em, order_seed, item_seed)
        assert st == abi.PLO_OK and err == 0xFFFFFFFF
        assert np.array_equal(got_off, off) and np.array_equal(got_len, np.diff(off))
        for i in range(lift.n_items):
            assert got_text[int(off[i]):int(off[i + 1])] == texts[i], (order_seed, item_seed, i)
        assert got_text == b"".join(texts)
    # the sample is not vacuous
    lifted = np.flatnonzero(lift.item_status == abi.ITEM_LIFTED)
    assert len(lifted) > 100
    assert (em.f["item_seq_off"][lifted] != abi.NO_FLIP).any(), "no flipped item"
    assert any(b"^" in texts[i] for i in lifted), "no text with a deletion"
    assert any(re.search(rb"[A-Z]0[A-Z]", texts[i]) for i in lifted), "no text with 0 between two letters"
    assert any(re.search(rb"[0-9]{3}", texts[i]) for i in lifted), "no text with a number of three digits"
    # the invariant: letters + inserted bases = NM
    want_nm, _ = tnd.expected_nm(lift, em.host, ix.chrom_seq)
    for i in lifted:
        c = lift.cigar[int(lift.item_cigar_off[i]):int(lift.item_cigar_off[i]) + int(lift.item_cigar_len[i])]
        assert mx.n_letters(texts[i]) + int((c >> 4)[(c & 15) == 1].sum()) == int(want_nm[i])
    # 6. the records
    check_records(em, want_nm, texts, off)
    check_records(em, want_nm, texts, off, vec=False, nthreads=3, order_seed=9)
    win.close()
    rd.close()


# ---- 6. records -----------------------------------------------------------------------------------------------------------------------

def test_records_cut_the_source_md_and_order_the_tags(tmp_path):
    """MD:Z sits behind ZM:C / NM:i and in front of SA:Z and CG:B,I; the first source MD is cut whatever its type, a second one stays; a read
    whose items are not all LIFTED; an unmapped copy keeps its MD"""
    from oracle import pyrecords as pr

    n = 70_001
    cig = trd.long_cigar(n)
    rng = np.random.default_rng(5)
    sp = rng.integers(0, 256, (n + 1) // 2, dtype=np.uint8)
    sp[-1] &= 0xF0
    src = pr.Record(0, 10, 60, 0, 0, -1, -1, 0, b"long", [int(x) for x in cig], sp.tobytes(), n, bytes(n),
                    [(b"rq", b"f" + struct.pack("<f", 1.0)), (b"NM", b"C\x07"), (b"MD", b"Zstale7A3\0")])
    rd, win = trd.write_window(tmp_path, [src.to_bytes(), trd.make_record(1, 33, aux=b"ZMC\x05MDi\x01\x02\x03\x04XXZkeep\0MDZ10A5\0"),
                                          trd.make_record(2, 20, aux=b"MDZ20\0XYZgo\0"), trd.make_record(3, 21, flag=0x10)])
    ix = trd.hand_index()
    rng = np.random.default_rng(6)
    ix.chrom_seq = [ACGT[rng.integers(0, 4, 36_000)].copy() for _ in range(2)]
    ix.chrom_len = np.array([36_000, 36_000], np.int64)
    L = abi.ITEM_LIFTED
    lift = trd.hand_lift([(0, 0, L, 0, 50, 0, 77, cig), (0, 1, L, 1, 20, 1, 99, cig), (1, 0, L, 0, 50, 0, 5, cg.encode("33M")), (1, 1, abi.ITEM_NO_LIFTOVER, 0, 0, 0, 0, []),
                          (2, 0, abi.ITEM_NO_LIFTOVER, 0, 0, 0, 0, []), (3, 1, L, 1, 20, 1, 35_979, cg.encode("21M"))])
    em = tnd.Emulated(win, ix, lift, trd.CN, trd.RN)
    texts, off = expected_md(lift, em.host, ix.chrom_seq)
    want_nm, _ = tnd.expected_nm(lift, em.host, ix.chrom_seq)
    st, got_off, got_text, _, _ = emu_md(em, 3, 5)
    assert st == abi.PLO_OK and np.array_equal(got_off, off) and got_text == b"".join(texts) and texts[3] == texts[4] == b"" and len(texts[0]) > 35_000
    res = check_records(em, want_nm, texts, off)
    check_records(em, want_nm, texts, off, vec=False)
    tags = lambda r: [t for _, _, t, _ in nx.aux_fields(r)]
    both, md, host = res["both"], res["md"], em.host
    assert len(both) == 5 and is_unmapped(both[3])
    # the record with more than 65535 ops: the order of the tags, the stale text gone
    assert tags(both[0])[-5:] == [b"ZM", b"NM", b"MD", b"SA", b"CG"] and tags(md[0])[-4:] == [b"ZM", b"MD", b"SA", b"CG"]
    assert b"stale" in host[0] and b"stale" not in both[0] and b"stale" not in md[0] and b"NMC\x07" not in both[0]
    # MD:i followed by a second MD:Z: only the first is cut
    assert b"MDi\x01\x02\x03\x04" in host[2] and b"MDi\x01\x02\x03\x04" not in md[2] and b"MDZ10A5\0" in md[2] and b"XXZkeep\0" in md[2]
    assert mx.strip_md(md[2])[1] == [b"10A5", texts[2]]
    # the unmapped copy of a read that carries MD: the host builder's bytes
    assert both[3] == md[3] == host[3] and b"MDZ20\0XYZgo\0" in host[3]
    for r, i in ((both[0], 0), (both[1], 1), (both[4], 5)):
        assert mx.strip_md(r)[1] == [texts[i]] and nx.strip_nm(r)[1] == [int(want_nm[i])]
    win.close()
    rd.close()


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------

def device_md(run_or_steps):
    mo = run_or_steps.eng.md_dev(run_or_steps.ddesc)
    n = int(mo.n_items)
    off = run_or_steps.eng.download(mo.item_md_off, np.uint64, n + 1)
    text = run_or_steps.eng.download(mo.md_text, np.uint8, int(mo.md_bytes)).tobytes() if int(mo.md_bytes) else b""
    return off, text, mo


def check_device_md(run, texts, off):
    got_off, got_text, mo = device_md(run)
    assert np.array_equal(got_off, off)
    for i in range(len(texts)):
        assert got_text[int(off[i]):int(off[i + 1])] == texts[i], (i, got_text[int(off[i]):int(off[i + 1])][:80], texts[i][:80])
    assert got_text == b"".join(texts)
    assert int(mo.md_bytes) == int(off[-1]) and int(mo.n_items) == len(texts) and int(mo.err_item) == 0xFFFFFFFF and mo.md_ms > 0
    return mo


def check_device_records(run, host, hoff_counts, lift, item_nm, texts):
    """plo_records_build_dev = the host builder's records with the fields the context's results call for"""
    rec = run.records()
    want, woff = with_tags(host, lift, item_nm, texts)
    assert rec.n_records == len(want) and (rec.n_lifted, rec.n_unmapped_copies) == hoff_counts
    assert np.array_equal(rec.record_off, woff)
    data = rec.data()
    for i, (a, e) in enumerate(zip(trd._split(data, rec.record_off), want)):
        assert a == e, (i, a[-80:], e[-80:])
    assert data == b"".join(want)


def relift(run):
    run.out = run.eng.liftover_batch_dev(run.ddesc)
    run.eng.compact_output_dev(run.out)
    run.finish()
    run.sa()


@pytest.mark.gpu
def test_device_md_and_records_of_the_small_bam(small_bam):
    """7. item_md_off, the text and md_bytes of plo_md_dev; the records behind it carry MD:Z, with plo_nm_dev in either order NM:i and MD:Z;
    the same context's next batch without the calls equals the host builder exactly"""
    w, path, meta = small_bam
    ixd = w.index_data()
    index = api.Index(ixd, 0)
    cn, rn = meta["contig_names"], bamsynth.ref_names(w)
    rd, win = trd.open_window(path)
    run = trd.DeviceRun(win, index, cn, rn, False)
    run.finish()
    run.sa()
    lift = run.lift_result()
    hdata, hoff, hnl, hnu = trd.host_records(win, ixd, lift, cn, rn, False)
    host = trd._split(hdata, hoff)
    texts, off = expected_md(lift, host, ixd.chrom_seq)
    want_nm, _ = tnd.expected_nm(lift, host, ixd.chrom_seq)
    assert any(b"^" in t for t in texts) and sum(1 for r in host if is_unmapped(r)) > 0
    check_device_md(run, texts, off)
    check_device_records(run, host, (hnl, hnu), lift, None, texts)  # MD alone
    assert np.array_equal(tnd.device_nm(run)[0], want_nm)
    check_device_records(run, host, (hnl, hnu), lift, want_nm, texts)  # MD, then NM: neither call drops the other's result
    relift(run)
    assert np.array_equal(tnd.device_nm(run)[0], want_nm)
    check_device_records(run, host, (hnl, hnu), lift, want_nm, None)  # NM alone: the lift dropped the MD result
    check_device_md(run, texts, off)
    check_device_records(run, host, (hnl, hnu), lift, want_nm, texts)  # NM, then MD
    # the next batch on the same context, without the calls: the host builder's bytes
    relift(run)
    check_device_records(run, host, (hnl, hnu), run.lift_result(), None, None)
    run.eng.close()
    win.close()
    rd.close()
    index.close()


def hand_window(tmp_path, cases):
    """the cases as reads of one BAM, the way test_nm_dev.hand_window lays them out: -> (index, path)"""
    SEG_POS = 37
    starts, parts, at = [], [ACGT[np.zeros(64, np.int64)]], 64
    for c in cases:
        starts.append(at)
        parts.append(c.ref)
        at += len(c.ref)
    chrom = np.concatenate(parts + [ACGT[np.zeros(64, np.int64)]])
    ixd = tnd.one_to_one_index(chrom, len(chrom) - SEG_POS, SEG_POS)
    recs, order = [], sorted(range(len(cases)), key=lambda k: starts[k] + cases[k].pos)
    for k in order:
        p = starts[k] + cases[k].pos - SEG_POS
        assert p >= 0
        recs.append(tnd.case_record(k, cases[k], p))
    path = str(tmp_path / "hand.bam")
    wr = bam.BamWriter(path, "@HD\tVN:1.6\n", trd.CN, [len(chrom) - SEG_POS], level=1)
    wr.write(b"".join(recs))
    wr.close()
    return ixd, path


@pytest.mark.gpu
def test_device_hand_made_items(tmp_path):
    """8. the hand-made items in one batch through the C ABI (see test_nm_dev.test_device_hand_made_items): whatever the lift stages make of
    a read's CIGAR, the text is md_expect's over the host builder's record.  The item of more than 65535 ops and the numbers of one to six
    digits run on the device."""
    cases = [c for c, _ in all_cases() if not c.flip]
    ixd, path = hand_window(tmp_path, cases)
    index = api.Index(ixd, 0)
    rd, win = trd.open_window(path)
    assert win.n_records == len(cases)
    run = trd.DeviceRun(win, index, trd.CN, ["chr1"], False)
    run.finish()
    run.sa()
    lift = run.lift_result()
    lifted = lift.item_status == abi.ITEM_LIFTED
    assert lifted.sum() == len(cases) - 1 and int(lift.item_cigar_len.max()) > 65535  # (the read of S and I alone has nothing to lift)
    hdata, hoff, hnl, hnu = trd.host_records(win, ixd, lift, trd.CN, ["chr1"], False)
    host = trd._split(hdata, hoff)
    texts, off = expected_md(lift, host, ixd.chrom_seq)
    for run_len in (9, 10, 99, 100, 999, 1000, 9999, 10_000, 100_000):
        assert any(re.fullmatch(rb"0[A-Z]%d[A-Z]0" % run_len, t) for t in texts), run_len
    assert any(re.search(rb"\^[A-Z]{1025}[0-9]", t) for t in texts) and any(re.search(rb"([A-Z]0){16}[A-Z]", t) for t in texts)
    check_device_md(run, texts, off)
    want_nm, _ = tnd.expected_nm(lift, host, ixd.chrom_seq)
    for i in np.flatnonzero(lifted):
        c = lift.item_cigar(int(i))
        assert mx.n_letters(texts[i]) + int((c >> 4)[(c & 15) == 1].sum()) == int(want_nm[i])
    check_device_records(run, host, (hnl, hnu), lift, None, texts)
    run.eng.close()
    win.close()
    rd.close()
    index.close()


@pytest.mark.gpu
def test_device_md_refusals(small_bam, tmp_path):
    """9. out of order and sparse: PLO_ERR_INVALID_ARG; a CIGAR past the chromosome's end: PLO_ERR_RANGE with err_item, by a check -- the
    context lifts the next batch correctly"""
    import torch

    from portello_amd import devbatch
    w, path, meta = small_bam
    rd, win = trd.open_window(path)
    index = api.Index(w.index_data(), 0)
    st = tnd.Steps(index)
    b, f, r = win.batch_raw()
    up = devbatch.upload_raw_window(b, f, r, st.dev)
    torch.cuda.synchronize()
    with pytest.raises(api.PortelloError, match="no lift result") as e:
        st.eng.md_dev(up.batch.desc())
    assert e.value.status == abi.PLO_ERR_INVALID_ARG
    st.lift(win, finish=False)
    with pytest.raises(api.PortelloError, match="no finishing result") as e:
        st.eng.md_dev(st.ddesc)
    assert e.value.status == abi.PLO_ERR_INVALID_ARG
    sp = bam.sparse_pack(win.batch_data())
    db = devbatch.DeviceBatch.from_batch_data(sp, st.dev)
    torch.cuda.synchronize()
    sdesc = db.desc()
    st.eng.liftover_batch_dev(sdesc)
    with pytest.raises(api.PortelloError, match="sparse") as e:
        st.eng.md_dev(sdesc)
    assert e.value.status == abi.PLO_ERR_INVALID_ARG
    st.eng.close()
    win.close()
    rd.close()
    index.close()
    # the window of test_nm_dev.test_device_nm_refusals: a contig that maps 1:1 onto the chromosome but is 50 bases longer than the
    # chromosome has room for, so the reads on its end lift to CIGARs that run past chrom_len
    SEG_POS, C = 100, 3000
    rng = np.random.default_rng(31)
    chrom = ACGT[rng.integers(0, 4, C)].copy()
    ixd = tnd.one_to_one_index(chrom, C - SEG_POS + 50, SEG_POS)
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
    st = tnd.Steps(index)
    lift = st.lift(win_a, stages)
    assert (lift.item_status == abi.ITEM_LIFTED).all() and lift.n_items == 5
    ends = lift.item_ref_pos + np.array([sum(int(c) >> 4 for c in lift.item_cigar(i)) for i in range(5)])
    assert list(ends > C) == [False, False, False, True, True] and int(ends[2]) == C
    with pytest.raises(api.PortelloError, match="consumes more reference") as e:
        st.eng.md_dev(st.ddesc)
    assert e.value.status == abi.PLO_ERR_RANGE and e.value.err_item == 3
    # the next batch on the same context
    lift = st.lift(win_b, stages)
    hdata, hoff, _, _ = trd.host_records(win_b, ixd, lift, trd.CN, ["chr1"], False)
    texts, off = expected_md(lift, trd._split(hdata, hoff), ixd.chrom_seq)
    check_device_md(st, texts, off)
    st.eng.close()
    for x in (win_a, rd_a, win_b, rd_b):
        x.close()
    index.close()


@pytest.mark.gpu
def test_bam_to_bam_with_md(tmp_path):
    """10. run_bam_to_bam(device_records=True, device_batch=True, emit_md=True), alone and with emit_nm, on a 2 000-read synthetic BAM"""
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
        pipeline.run_bam_to_bam(inp, str(tmp_path / "x.bam"), index, ixd, cn, rn, lens, emit_md=True)
    kw = dict(window_reads=700, n_workers=2, io_threads=8, device_records=True, device_batch=True)
    outs = {}
    for name, extra in (("md", dict(emit_md=True, unassembled_path=unp)), ("both", dict(emit_nm=True, emit_md=True)), ("off", dict(emit_md=False))):
        outp = str(tmp_path / f"{name}.bam")
        st = pipeline.run_bam_to_bam(inp, outp, index, ixd, cn, rn, lens, **kw, **extra)
        assert st.reads == w.n_reads
        outs[name] = (outp, st)
    for name in ("md", "both"):
        assert outs[name][1].md_device_ms > 0 and outs[name][1].lift_detail_s.get("md", 0) > 0
    assert outs["both"][1].nm_device_ms > 0 and outs["md"][1].nm_device_ms == 0
    assert outs["off"][1].md_device_ms == 0 and "md" not in outs["off"][1].lift_detail_s

    import bamcheck

    records_of = lambda path: bamcheck.read_bam(path)[2]
    off_recs = records_of(outs["off"][0])
    assert len(off_recs) == outs["off"][1].records_out
    chroms = ixd.chrom_seq
    for name in ("md", "both"):
        recs = records_of(outs[name][0])
        assert len(recs) == len(off_recs) == outs[name][1].records_out
        stripped, n_lifted, n_events = [], 0, 0
        for r in recs:
            bare, vals = mx.strip_md(r)
            bare, nms = nx.strip_nm(bare)
            stripped.append(bare)
            if is_unmapped(r):
                assert vals == [] and nms == []
                continue
            n_lifted += 1
            assert vals == [mx.md_of_record(bare, chroms)]
            n_events += vals[0].isdigit() is False
            tags = [t for _, _, t, _ in nx.aux_fields(r)]
            if name == "both":
                assert nms == [nx.nm_of_record(bare, chroms)] and tags[tags.index(b"MD") - 2:tags.index(b"MD")] == [b"ZM", b"NM"]
            else:
                assert nms == [] and tags[tags.index(b"MD") - 1] == b"ZM"
        assert n_lifted == outs[name][1].lifted > 1000 and n_events > 0
        assert sorted(stripped) == sorted(off_recs)
        if name == "md":  # with the field removed the file passes the existing record comparison
            bare_path = str(tmp_path / "bare.bam")
            wr = bam.BamWriter(bare_path, bam.output_header(rn, lens), rn, lens, level=1)
            wr.write(b"".join(stripped))
            wr.close()
            v = expect.verify_lifted_bam(inp, [bare_path], ixd, cn, rn, window=1000, every=1, threads=8, unassembled_bam=unp)
            assert v["ok"] and v["reads_verified"] == w.n_reads and v["records_verified"] == outs[name][1].records_out == v["records_in_output"], v
    index.close()
