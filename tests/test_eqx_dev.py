"""= / X CIGARs of the lifted records written on the device (plo_eqx_dev, portello_amd/csrc/eqx_core.hpp) and put into the records by
plo_records_build_dev in place of the lift's M CIGARs.

The yardstick is plo_records_build on the same window (the host builder writes M) plus tests/eqx_expect.py, a restatement of the rule over
an output record's own bytes: neither touches the code under test.  All comparisons are of integers and bytes.  The CPU tests run
eqx_core.hpp and records_core.hpp under the wave emulator (tests/emu/emu_eqx.cpp), with shuffled lane and item orders, and the hand-made
cases once more in a program built with AddressSanitizer + UBSan where every array sits in a heap block of its exact size; the GPU tests
run the C ABI on the device and the pipeline mode."""
import os
import struct

import numpy as np
import pytest

import emu_eqx_lib as eel
import emu_md_lib as eml
import emu_nm_lib as enl
import eqx_expect as ex
import md_expect as mx
import nm_expect as nx
import test_md_dev as tmd
import test_nm_dev as tnd
import test_records_dev as trd
from portello_amd import abi, api, bam, bamsynth, synth
from portello_amd import cigar as cg

# the small_bam recipe of tests/test_md_dev.py.  test_small_bam_items asserts that the seed holds a flipped item with an X, an item with
# a D next to an X and a run across a 16-byte line of the reference.
SMALL_SEED = tmd.SMALL_SEED
ACGT = tnd.ACGT
is_unmapped = tmd.is_unmapped


@pytest.fixture(scope="module")
def small_bam(tmp_path_factory):
    d = tmp_path_factory.mktemp("eqxdev")
    w = synth.generate(synth.config("tiny", n_reads=300, seed=SMALL_SEED, split_read_frac=0.3, sorted_reads=True))
    path = str(d / "reads.bam")
    meta = bamsynth.write_read_bam(w, path, level=6, n_unmapped=4)
    return w, path, meta


def expected_eqx(lift, recs, chroms):
    """eqx_expect over the host builder's records -> (the CIGARs [n_items], empty for items that are not LIFTED; item_eqx_off [n_items + 1])"""
    cigs = [np.zeros(0, np.uint32)] * lift.n_items
    lr = tnd.lifted_records(recs)
    idx = np.flatnonzero(lift.item_status == abi.ITEM_LIFTED)
    assert len(lr) == len(idx)
    for i, r in zip(idx, lr):
        tid, pos, _, ops, codes = nx.record_alignment(r)
        assert tid == int(lift.item_chrom_index[i]) and pos == int(lift.item_ref_pos[i])
        cigs[i] = ex.eqx_ops(ops, codes, chroms[tid], pos)
    off = np.zeros(lift.n_items + 1, np.uint64)
    off[1:] = np.cumsum([len(c) for c in cigs])
    return cigs, off


def flat(cigs):
    return np.concatenate(cigs).astype(np.uint32) if len(cigs) else np.zeros(0, np.uint32)


def with_eqx(recs, lift, item_nm, texts, cigs):
    """the host builder's records as plo_records_build_dev writes them while the context holds an NM result, an MD result, an eqx result
    (cigs), any of them or none (None): test_md_dev.with_tags, then the CIGAR of every lifted record replaced -> (records, record_off)"""
    out, _ = tmd.with_tags(recs, lift, item_nm, texts)
    if cigs is not None:
        it = iter(np.flatnonzero(lift.item_status == abi.ITEM_LIFTED))
        out = [r if is_unmapped(r) else ex.splice_cigar(r, cigs[int(next(it))]) for r in out]
    off = np.zeros(len(out) + 1, np.uint64)
    off[1:] = np.cumsum([len(r) for r in out])
    return out, off


def emu_eqx(em, order_seed=0, item_seed=0):
    return eel.eqx_batch(em.ix, em.vb, em.lift, em.f["item_seq_off"], em.f["rev_seq"], order_seed, item_seed)


def emu_records(em, item_nm, md_off, md_text, eqx_off, eqx_ops, **kw):
    return eel.records_with_eqx(em.ix, em.vb, em.rw.raw, em.rw.rec_off, em.lift, em.f, em.sa_off, em.sa_text, em.cn, item_nm, md_off, md_text, eqx_off, eqx_ops, em.target, **kw)


def check_records(em, item_nm, texts, md_off, cigs, eqx_off, **kw):
    """6. records_core.hpp under the emulator with an eqx result alone, with NM + MD + eqx, with none: byte for byte"""
    text, ops = b"".join(texts), flat(cigs)
    res = {}
    for name, nm, md, eq in (("eqx", None, None, cigs), ("all", item_nm, texts, cigs), ("none", None, None, None)):
        want, woff = with_eqx(em.host, em.lift, nm, md, eq)
        st, data, roff, nl, nu = emu_records(em, nm, md_off if md is not None else None, text if md is not None else None, eqx_off if eq is not None else None,
                                             ops if eq is not None else None, **kw)
        assert st == 0 and (nl, nu) == (em.hnl, em.hnu) and np.array_equal(roff, woff), name
        for i, (a, e) in enumerate(zip(trd._split(data, roff), want)):
            assert a == e, (name, i, a[:80], e[:80])
        assert data == b"".join(want), name
        res[name] = want
    assert b"".join(res["none"]) == em.hdata
    return res


# ---- 1. the rule by hand --------------------------------------------------------------------------------------------------------------

by_hand = tmd.by_hand


def test_rule_by_hand():
    worked = [(by_hand("8M", "ACGAACGT", b"ACGTACGT"), "3=1X4="),                # the example of the header
              (by_hand("2S4M1I3M", "TTACCTAACG", b"ACGTACG"), "2S2=1X1=1I3="),  # only the 4M and the 3M are rewritten
              (by_hand("1M", "N", b"N"), "1X"), (by_hand("1M", "R", b"R"), "1="),  # N against N mismatches, R against R matches
              (by_hand("3M", "=A=", b"#AN"), "3="),                              # a read '=' matches anything
              (by_hand("4M", "CCCC", b"C#\x00\xff"), "1=3X"), (by_hand("2M", "AN", b"a#"), "2X"),  # a reference byte outside the table
              (by_hand("5M5=", "ACGTACGTAC", b"ACGTACGTAC"), "5=5="),           # two adjacent compared ops: two runs
              (by_hand("3X2=", "ACGTA", b"ACGTT"), "3=1=1X"),                     # the source's = and X are compared like M
              (by_hand("2M0M2M", "ACGT", b"ACGT"), "2=2="), (by_hand("0M", "", b"A"), ""), (by_hand("2M0I2M", "ACGT", b"ACTT"), "2=0I1X1=")]
    for c, text in worked:
        want = ex.parse(text)
        assert ex.text(want) == text
        assert np.array_equal(ex.eqx_ops(c.ops, c.codes, c.ref, c.pos), want) and np.array_equal(ex.eqx_slow(c.ops, c.codes, c.ref, c.pos), want), c.name
        assert ex.n_edits(want) == nx.nm_counts(c.ops, c.codes, c.ref, c.pos)[0], c.name
        assert ex.x_positions(want) == ex.md_mismatch_positions(mx.md_text(c.ops, c.codes, c.ref, c.pos)), c.name
        for seed in (0, 5):
            st, n, got = eel.eqx_one(c, seed)
            assert (st, n) == (abi.PLO_OK, len(want)) and np.array_equal(got, want), (c.name, seed, ex.text(got))
    assert np.array_equal(ex.collapse_to_m(ex.parse("2S2=1X1=1I3=")), ex.parse("2S4M1I3M"))


# ---- 2. hand-made items ---------------------------------------------------------------------------------------------------------------

def eqx_cases():
    """-> [(case, its = / X CIGAR as text, or None)], every one from explicit bases (test_md_dev.exact: the reference's own letters but at
    the read positions given)"""
    rng = np.random.default_rng(16)
    ref = ACGT[rng.integers(0, 4, 6000)].copy()
    M = lambda s: np.array(cg.encode(s), np.uint32)
    out = []

    def add(name, cigar, pos, mism, want, flip=False, front=0):
        ops = M(cigar) if isinstance(cigar, str) else cigar
        t, l = ops & 15, (ops >> 4).astype(np.int64)
        parts, at = [ACGT[:0]], pos  # the reference letters under the read, an A for every inserted or clipped base
        for tt, ll in zip(t, l):
            if tt in (0, 7, 8):
                parts.append(ref[at:at + ll])
            elif tt in (1, 4):
                parts.append(ACGT[np.zeros(ll, np.int64)])
            if tt in (0, 2, 3, 7, 8):
                at += ll
        out.append((enl.Case(name, ops, tmd.exact(np.concatenate(parts), mism), ref, pos, flip=flip, front=front), want))

    # an op of 1 base, an all-X op, a mismatch on the first and on the last base of an op
    add("1M match", "1M", 9, (), "1=")
    add("1M mismatch", "1M", 9, (0,), "1X")
    add("all X", "20M", 5, range(20), "20X")
    add("all X, three pieces", "40M", 5, range(40), "40X")
    add("first and last of an op", "20M5I20M", 7, (0, 19, 25, 44), "1X18=1X5I1X18=1X")
    # a mismatch on either side of a 16-byte line of the reference, and on both: every residue of pos, so every alignment of the chromosome
    for p in range(16):
        add(f"before the line @{p}", "48M", p, (15,), "15=1X32=")
        add(f"behind the line @{p}", "48M", p, (16,), "16=1X31=")
        add(f"across the line @{p}", "48M", p, (15, 16), "15=2X31=")
    # odd and even read offsets (the nibble phase), the bases at every residue of their 8-byte words
    for s in (1, 2):
        for front in (0, 3):
            add(f"{s}S, front {front}", f"{s}S100M", 6, (s + 40, s + 41, s + 77), f"{s}S40=2X35=1X22=", front=front)
    # a run that crosses piece boundaries
    add("= across pieces", "40M", 3, (), "40=")
    add("X across pieces", "40M", 3, range(10, 30), "10=20X10=")
    # a run that crosses a 64-piece trip boundary: one match of more than 1024 bases; the mismatch at piece 63 / 64 for one residue of pos
    for p in range(16):
        add(f"trip, no mismatch @{p}", "2000M", p, (), "2000=")
        add(f"trip, before @{p}", "2000M", p, (1015,), "1015=1X984=")
        add(f"trip, behind @{p}", "2000M", p, (1016,), "1016=1X983=")
        add(f"trip, across @{p}", "2000M", p, (1015, 1016), "1015=2X983=")
    add("X across a trip", "2000M", 8, range(1000, 1040), "1000=40X960=")
    add("three trips", "3000M", 2, (0, 1500, 2999), "1X1499=1X1498=1X")
    # items of 63, 64, 65, 128 and 129 ops: 3M 1I 3M 1I ... (an I in front of the step boundary), and behind 2S (an M in front of it)
    for n in (63, 64, 65, 128, 129):
        for lead in ("", "2S"):
            ops = np.concatenate([M(lead), np.tile(M("3M1I"), 70)])[:n]
            l_read = int((ops >> 4).sum())
            add(f"{n} ops {lead}", ops, 4, range(1, l_read, 7), None)
    # a step whose 64 ops are all non-compared, compared ops in the steps around it
    add("a step of I and D", np.concatenate([np.tile(M("3M1I"), 32), np.tile(M("1I1D"), 32), M("5M")]), 10, (1, 130), None)
    # leading and trailing S; I, D, N, H and P in place
    add("S around", "5S20M7S", 12, (8,), "5S3=1X16=7S")
    add("I D N H P", "3H2S10M2I10M3D10M50N10M1P10M4S2H", 13, (), "3H2S10=2I10=3D10=50N10=1P10=4S2H")
    add("X next to D and I", "10M3D10M2I10M", 14, (9, 10, 19, 22), "9=1X3D1X8=1X2I1X9=")
    # two adjacent compared ops, a compared op of length 0, non-compared ops of length 0
    add("5M5=", "5M5=", 15, (), "5=5=")
    add("4X4M, all mismatches", "4X4M", 15, range(8), "4X4X")
    add("0M between", "5M0M5M", 16, (4, 5), "4=1X1X4=")
    add("0M alone", "3S0M3S", 16, (), "3S3S")
    add("0I 0D", "5M0I0D5M", 17, (), "5=0I0D5=")
    # a flipped item: the bases come from the finishing's buffer
    add("flipped", "2S75M", 100, (2, 40, 41, 76), "2S1X37=2X34=1X", flip=True)
    return out


def all_cases():
    """test_nm_dev.hand_cases() and the cases above -> [(case, text or None)]"""
    return [(c, None) for c in tnd.hand_cases()] + eqx_cases()


def test_hand_made_items(tmp_path):
    cases = all_cases()
    wants = []
    for c, text in cases:
        want = ex.eqx_ops(c.ops, c.codes, c.ref, c.pos)
        if c.l_seq < 5000:
            assert np.array_equal(want, ex.eqx_slow(c.ops, c.codes, c.ref, c.pos)), c.name
        if text is not None:
            assert ex.text(want) == text, (c.name, ex.text(want)[:120])  # the case produces what it was made for
        # the three properties: M back, NM, MD's mismatch positions
        if not np.isin(c.ops & 15, (7, 8)).any() and (c.ops >> 4).all() and not ((c.ops[1:] & 15 == 0) & (c.ops[:-1] & 15 == 0)).any():
            assert np.array_equal(ex.collapse_to_m(want), c.ops), c.name
        assert ex.n_edits(want) == nx.nm_counts(c.ops, c.codes, c.ref, c.pos)[0], c.name
        assert ex.x_positions(want) == ex.md_mismatch_positions(mx.md_text(c.ops, c.codes, c.ref, c.pos)), c.name
        wants.append(want)
        for seed in ((0, 5) if len(c.ops) < 1000 and c.l_seq < 300 else (0,)):  # (the sanitizer program below runs every case with shuffled lanes)
            st, n, got = eel.eqx_one(c, seed)
            assert st == abi.PLO_OK, (c.name, seed, st)  # (-2: a store outside the item's slot, -3: an op of it unwritten, -4: count and emit differ)
            assert n == len(want) and np.array_equal(got, want), (c.name, seed, ex.text(got[:40]), ex.text(want[:40]))
    by_name = {c.name: w for (c, _), w in zip(cases, wants)}
    assert ex.text(by_name["S + I"]) == "5S10I3S" and len(by_name["70001 ops"]) == 70_001
    for n in (63, 64, 65, 128, 129):
        assert len(by_name[f"{n} ops "]) > n and np.isin(by_name[f"{n} ops 2S"] & 15, (ex.X,)).sum() > 5
    # refusals: PLO_ERR_RANGE, nothing written
    bad = tnd.refusal_cases()
    for c in bad:
        with pytest.raises(IndexError):
            ex.eqx_ops(c.ops, c.codes, c.ref, c.pos)
        for seed in (0, 5):
            st, n, got = eel.eqx_one(c, seed)
            assert (st, n, len(got)) == (abi.PLO_ERR_RANGE, 0, 0), c.name
    # 7. all of them once more under AddressSanitizer + UBSan, every array (the output ops too) in a heap block of its exact size
    rc, err_text, res = eel.run_asan([c for c, _ in cases] + bad, str(tmp_path), order_seed=3)
    assert rc == 0, err_text[-3000:]
    for (c, _), w, (st, got) in zip(cases, wants, res):
        assert st == abi.PLO_OK and np.array_equal(got, w), c.name
    assert [(st, len(got)) for st, got in res[len(cases):]] == [(abi.PLO_ERR_RANGE, 0)] * len(bad)


def test_three_walks_agree():
    """the invariant eqx_core.hpp states, on what the three emulated walks hand out (no model in between): the bases under X plus the I and D
    lengths are NM, the X positions are the MD letters that do not stand behind '^', and the = / X CIGAR keeps the reference and read length"""
    def lengths(ops):
        t, l = ops & 15, (ops >> 4).astype(np.int64)
        return int(l[np.isin(t, (0, 2, 3, 7, 8))].sum()), int(l[np.isin(t, (0, 1, 4, 7, 8))].sum())

    for c, _ in all_cases():
        for seed in (0, 5):
            st_nm, nm, _ = enl.nm_one(c, seed)
            st_md, _, md = eml.md_one(c, seed)
            st_eqx, _, eqx = eel.eqx_one(c, seed)
            assert (st_nm, st_md, st_eqx) == (abi.PLO_OK,) * 3, (c.name, seed)
            assert ex.n_edits(eqx) == nm, (c.name, seed)
            assert ex.x_positions(eqx) == ex.md_mismatch_positions(md), (c.name, seed)
            assert lengths(eqx) == lengths(c.ops), (c.name, seed)
    for c in tnd.refusal_cases():
        for seed in (0, 5):
            assert (enl.nm_one(c, seed)[0], eml.md_one(c, seed)[0], eel.eqx_one(c, seed)[0]) == (abi.PLO_ERR_RANGE,) * 3, (c.name, seed)


# ---- 3. the 65 535 boundary through the record builder ---------------------------------------------------------------------------------

def alternating_read(k, chrom, pos, n_ops, flag=0):
    """a read of one M over n_ops bases that match and mismatch the chromosome from pos in turn: its = / X CIGAR has n_ops ops of 1 base"""
    codes = tmd.exact(chrom[pos:pos + n_ops], range(1, n_ops, 2))
    c = enl.Case(f"{n_ops} alternating", np.array(cg.encode(f"{n_ops}M"), np.uint32), codes, chrom, pos)
    return c, bamsynth.encode_record(0, pos, 37, flag, b"alt%d" % k, c.ops, c.packed().tobytes(), n_ops, bytes(n_ops), b"XXZkeep\0")


def test_the_65535_boundary(tmp_path):
    """two reads of one long M whose = / X CIGARs have exactly 65 535 and 65 536 ops: the first is serialised in place, the second with the
    <l_seq>S<ref_len>N placeholder and CG:B,I, though the M CIGAR of either is one op; a third read's item is not LIFTED"""
    ix = trd.hand_index()
    rng = np.random.default_rng(8)
    ix.chrom_seq = [ACGT[rng.integers(0, 4, 70_000)].copy() for _ in range(2)]
    ix.chrom_len = np.array([70_000, 70_000], np.int64)
    (c0, r0), (c1, r1) = alternating_read(0, ix.chrom_seq[0], 7, 65_535), alternating_read(1, ix.chrom_seq[0], 11, 65_536)
    rd, win = trd.write_window(tmp_path, [r0, r1, trd.make_record(2, 30)])
    L = abi.ITEM_LIFTED
    lift = trd.hand_lift([(0, 0, L, 0, 50, 0, 7, c0.ops), (1, 0, L, 0, 50, 0, 11, c1.ops), (2, 0, abi.ITEM_NO_LIFTOVER, 0, 0, 0, 0, [])])
    em = tnd.Emulated(win, ix, lift, trd.CN, trd.RN)
    cigs, off = expected_eqx(lift, em.host, ix.chrom_seq)
    assert [len(c) for c in cigs] == [65_535, 65_536, 0] and set((cigs[1] >> 4).tolist()) == {1}
    st, got_off, got_ops, got_len, err = emu_eqx(em, 2, 4)
    assert st == abi.PLO_OK and np.array_equal(got_off, off) and np.array_equal(got_ops, flat(cigs)) and list(got_len) == [65_535, 65_536, 0]
    want_nm, _ = tnd.expected_nm(lift, em.host, ix.chrom_seq)
    texts, md_off = tmd.expected_md(lift, em.host, ix.chrom_seq)
    res = check_records(em, want_nm, texts, md_off, cigs, off)
    check_records(em, want_nm, texts, md_off, cigs, off, vec=False, nthreads=3, order_seed=6)
    a, b, u = res["eqx"]
    n_cigar = lambda r: struct.unpack_from("<H", r, 16)[0]
    assert n_cigar(a) == 65_535 and b"CGBI" not in a and n_cigar(em.host[0]) == 1
    assert n_cigar(b) == 2 and b.endswith(b"CGBI" + struct.pack("<I", 65_536) + cigs[1].astype("<u4").tobytes()) and n_cigar(em.host[1]) == 1
    assert np.frombuffer(b, "<u4", 2, 36 + b[12]).tolist() == [(65_536 << 4) | 4, (65_536 << 4) | 3]
    assert is_unmapped(u) and u == em.host[2]
    for r, c in ((a, cigs[0]), (b, cigs[1])):
        assert np.array_equal(nx.record_alignment(r)[3], c)
    win.close()
    rd.close()


# ---- 4. refusals ----------------------------------------------------------------------------------------------------------------------

def test_refusal_names_the_lowest_item(tmp_path):
    lens = [40, 41, 42, 43, 44, 45]
    recs = [trd.make_record(k, l) for k, l in enumerate(lens)]
    rd, win = trd.write_window(tmp_path, recs)
    ix = tnd.real_hand_index()
    M = lambda s: cg.encode(s)
    L = abi.ITEM_LIFTED
    # item 2 (flipped): one read base too many; item 4: one base past chrom_len; items 0, 1, 3, 5: fine (5 ends at chrom_len)
    items = [(0, 0, L, 0, 50, 0, 100, M("40M")), (1, 0, L, 0, 50, 0, 3000, M("41M")), (2, 1, L, 1, 20, 1, 10, M("42M1I")), (3, 0, L, 0, 50, 0, 20, M("43M")),
             (4, 0, L, 0, 50, 0, 3957, M("44M")), (5, 0, L, 0, 50, 0, 3955, M("45M"))]
    em = tnd.Emulated(win, ix, trd.hand_lift(items), trd.CN, trd.RN)
    for order_seed, item_seed in ((0, 0), (4, 9), (1, 2)):
        st, _, ops, _, err = emu_eqx(em, order_seed, item_seed)
        assert st == abi.PLO_ERR_RANGE and err == 2 and len(ops) == 0
    # the chromosome's end alone, at a higher item
    items[2] = (2, 1, L, 1, 20, 1, 10, M("42M"))
    em = tnd.Emulated(win, ix, trd.hand_lift(items), trd.CN, trd.RN)
    for order_seed, item_seed in ((0, 0), (3, 7)):
        st, _, ops, _, err = emu_eqx(em, order_seed, item_seed)
        assert st == abi.PLO_ERR_RANGE and err == 4 and len(ops) == 0
    win.close()
    rd.close()


# ---- 5. and 6. the small_bam recipe ---------------------------------------------------------------------------------------------------

def check_properties(lift, cigs, want_nm, texts):
    """the three properties that need no new yardstick, for every lifted item"""
    for i in np.flatnonzero(lift.item_status == abi.ITEM_LIFTED):
        c = lift.cigar[int(lift.item_cigar_off[i]):int(lift.item_cigar_off[i]) + int(lift.item_cigar_len[i])]
        assert np.array_equal(ex.collapse_to_m(cigs[i]), c), i       # = / X collapsed to M and merged: the item's M CIGAR
        assert ex.n_edits(cigs[i]) == int(want_nm[i]), i               # X bases + I + D lengths: nm_expect's NM
        assert ex.x_positions(cigs[i]) == ex.md_mismatch_positions(texts[i]), i  # the X positions: md_expect's mismatch positions


def test_small_bam_items(small_bam, oracle):
    w, path, meta = small_bam
    ix = w.index_data()
    rd, win = trd.open_window(path)
    lift = oracle.liftover_batch(ix, win.batch_data(), abi.STAGES_ALL, 2)
    em = tnd.Emulated(win, ix, lift, meta["contig_names"], bamsynth.ref_names(w))
    cigs, off = expected_eqx(lift, em.host, ix.chrom_seq)
    for order_seed, item_seed in ((0, 0), (7, 3)):  # the ticket loop in lane order; shuffled lanes, shuffled items
        st, got_off, got_ops, got_len, err = emu_eqx(em, order_seed, item_seed)
        assert st == abi.PLO_OK and err == 0xFFFFFFFF
        assert np.array_equal(got_off, off) and np.array_equal(got_len, np.diff(off))
        for i in range(lift.n_items):
            assert np.array_equal(got_ops[int(off[i]):int(off[i + 1])], cigs[i]), (order_seed, item_seed, i)
        assert np.array_equal(got_ops, flat(cigs))
    # the sample is not vacuous
    lifted = np.flatnonzero(lift.item_status == abi.ITEM_LIFTED)
    assert len(lifted) > 100
    kinds = lambda i: (cigs[i] & 15).tolist()
    assert any(em.f["item_seq_off"][i] != abi.NO_FLIP and ex.X in kinds(i) for i in lifted), "no flipped item with an X"
    assert any({(2, ex.X), (ex.X, 2)} & set(zip(kinds(i), kinds(i)[1:])) for i in lifted), "no item with a D next to an X"
    assert any((cigs[i] >> 4)[np.isin(cigs[i] & 15, (ex.EQ, ex.X))].max(initial=0) > 16 for i in lifted), "no run across a 16-byte line"
    want_nm, _ = tnd.expected_nm(lift, em.host, ix.chrom_seq)
    texts, md_off = tmd.expected_md(lift, em.host, ix.chrom_seq)
    check_properties(lift, cigs, want_nm, texts)
    # 6. the records
    check_records(em, want_nm, texts, md_off, cigs, off)
    check_records(em, want_nm, texts, md_off, cigs, off, vec=False, nthreads=3, order_seed=9)
    win.close()
    rd.close()


def test_binding_and_pipeline_switch(tmp_path):
    import ctypes as C

    from portello_amd import pipeline

    assert abi.PLO_API_VERSION >= 16 and [f[0] for f in abi.PloEqxOut._fields_] == ["n_items", "item_eqx_off", "eqx_ops", "n_ops", "err_item", "eqx_ms"]
    assert C.sizeof(abi.PloEqxOut) == 40 and abi.PloEqxOut.n_ops.offset == 24 and abi.PloEqxOut.eqx_ms.offset == 36
    assert callable(api.Engine.eqx_dev) and pipeline.PipelineStats().eqx_device_ms == 0.0
    with pytest.raises(ValueError, match="device_records"):
        pipeline.run_bam_to_bam(str(tmp_path / "none.bam"), str(tmp_path / "x.bam"), None, None, [], [], [], emit_eqx=True)


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------

def device_eqx(run_or_steps):
    eo = run_or_steps.eng.eqx_dev(run_or_steps.ddesc)
    n = int(eo.n_items)
    off = run_or_steps.eng.download(eo.item_eqx_off, np.uint64, n + 1)
    ops = run_or_steps.eng.download(eo.eqx_ops, np.uint32, int(eo.n_ops)) if int(eo.n_ops) else np.zeros(0, np.uint32)
    return off, ops, eo


def check_device_eqx(run, cigs, off):
    got_off, got_ops, eo = device_eqx(run)
    assert np.array_equal(got_off, off)
    for i in range(len(cigs)):
        g = got_ops[int(off[i]):int(off[i + 1])]
        assert np.array_equal(g, cigs[i]), (i, ex.text(g[:40]), ex.text(cigs[i][:40]))
    assert np.array_equal(got_ops, flat(cigs))
    assert int(eo.n_ops) == int(off[-1]) and int(eo.n_items) == len(cigs) and int(eo.err_item) == 0xFFFFFFFF and eo.eqx_ms > 0
    return eo


def check_device_records(run, host, counts, lift, item_nm, texts, cigs):
    """plo_records_build_dev = the host builder's records with the fields and the CIGARs the context's results call for"""
    rec = run.records()
    want, woff = with_eqx(host, lift, item_nm, texts, cigs)
    assert rec.n_records == len(want) and (rec.n_lifted, rec.n_unmapped_copies) == counts
    assert np.array_equal(rec.record_off, woff)
    data = rec.data()
    for i, (a, e) in enumerate(zip(trd._split(data, rec.record_off), want)):
        assert a == e, (i, a[:80], e[:80])
    assert data == b"".join(want)


@pytest.mark.gpu
def test_device_eqx_and_records_of_the_small_bam(small_bam):
    """8. item_eqx_off, the ops and n_ops of plo_eqx_dev; the records behind it carry the = / X CIGARs; plo_nm_dev / plo_md_dev in either
    order keep each other's and this call's result; after a re-lift a build without the call equals the host builder exactly"""
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
    cigs, off = expected_eqx(lift, host, ixd.chrom_seq)
    texts, md_off = tmd.expected_md(lift, host, ixd.chrom_seq)
    want_nm, _ = tnd.expected_nm(lift, host, ixd.chrom_seq)
    assert any(ex.X in (c & 15) for c in cigs) and sum(1 for r in host if is_unmapped(r)) > 0
    check_device_eqx(run, cigs, off)
    check_device_records(run, host, (hnl, hnu), lift, None, None, cigs)  # eqx alone
    assert np.array_equal(tnd.device_nm(run)[0], want_nm)
    tmd.check_device_md(run, texts, md_off)
    check_device_records(run, host, (hnl, hnu), lift, want_nm, texts, cigs)  # eqx, NM, MD: none of the calls drops another's result
    tmd.relift(run)
    tmd.check_device_md(run, texts, md_off)
    check_device_records(run, host, (hnl, hnu), lift, None, texts, None)  # MD alone: the lift dropped the eqx result
    check_device_eqx(run, cigs, off)
    assert np.array_equal(tnd.device_nm(run)[0], want_nm)  # (NM and MD read the lift's M CIGAR: the same values behind an eqx result)
    check_device_records(run, host, (hnl, hnu), lift, want_nm, texts, cigs)  # MD, eqx, NM
    tmd.relift(run)
    assert np.array_equal(tnd.device_nm(run)[0], want_nm)
    check_device_eqx(run, cigs, off)
    check_device_records(run, host, (hnl, hnu), lift, want_nm, None, cigs)  # NM, eqx
    # the next batch on the same context, without the calls: the host builder's bytes
    tmd.relift(run)
    check_device_records(run, host, (hnl, hnu), run.lift_result(), None, None, None)
    run.eng.close()
    win.close()
    rd.close()
    index.close()


@pytest.mark.gpu
def test_device_hand_made_items(tmp_path):
    """9. the hand-made items and the two 65 535-boundary reads in one batch through the C ABI (see test_md_dev.test_device_hand_made_items):
    whatever the lift stages make of a read's CIGAR, the ops are eqx_expect's over the host builder's record"""
    cases = [c for c, _ in all_cases() if not c.flip and (c.ops >> 4).all()]  # (ops of length 0 stay with the emulated cases)
    rng = np.random.default_rng(8)
    chrom = ACGT[rng.integers(0, 4, 70_000)].copy()
    cases += [alternating_read(0, chrom, 7, 65_535)[0], alternating_read(1, chrom, 11, 65_536)[0]]
    ixd, path = tmd.hand_window(tmp_path, cases)
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
    cigs, off = expected_eqx(lift, host, ixd.chrom_seq)
    n_ops = sorted(len(c) for c in cigs)
    assert 65_535 in n_ops and 65_536 in n_ops and n_ops[-1] > 65_536 and any(len(c) == 0 for c in cigs)
    assert sum(1 for i in np.flatnonzero(lifted) if int(lift.item_cigar_len[i]) <= 65_535 < len(cigs[i])) >= 1  # the rule goes by the NEW count
    want_nm, _ = tnd.expected_nm(lift, host, ixd.chrom_seq)
    texts, _ = tmd.expected_md(lift, host, ixd.chrom_seq)
    check_properties(lift, cigs, want_nm, texts)
    check_device_eqx(run, cigs, off)
    check_device_records(run, host, (hnl, hnu), lift, None, None, cigs)
    run.eng.close()
    win.close()
    rd.close()
    index.close()


@pytest.mark.gpu
def test_device_eqx_refusals(small_bam, tmp_path):
    """10. out of order and sparse: PLO_ERR_INVALID_ARG; CIGARs past the chromosome's end: PLO_ERR_RANGE with the lowest item in err_item, by
    a check -- the context lifts the next batch correctly"""
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
        st.eng.eqx_dev(up.batch.desc())
    assert e.value.status == abi.PLO_ERR_INVALID_ARG
    st.lift(win, finish=False)
    with pytest.raises(api.PortelloError, match="no finishing result") as e:
        st.eng.eqx_dev(st.ddesc)
    assert e.value.status == abi.PLO_ERR_INVALID_ARG
    sp = bam.sparse_pack(win.batch_data())
    db = devbatch.DeviceBatch.from_batch_data(sp, st.dev)
    torch.cuda.synchronize()
    sdesc = db.desc()
    st.eng.liftover_batch_dev(sdesc)
    with pytest.raises(api.PortelloError, match="sparse") as e:
        st.eng.eqx_dev(sdesc)
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
        st.eng.eqx_dev(st.ddesc)
    assert e.value.status == abi.PLO_ERR_RANGE and e.value.err_item == 3  # two items leave the chromosome: the lower one
    # the next batch on the same context
    lift = st.lift(win_b, stages)
    hdata, hoff, _, _ = trd.host_records(win_b, ixd, lift, trd.CN, ["chr1"], False)
    cigs, off = expected_eqx(lift, trd._split(hdata, hoff), ixd.chrom_seq)
    check_device_eqx(st, cigs, off)
    st.eng.close()
    for x in (win_a, rd_a, win_b, rd_b):
        x.close()
    index.close()


def record_key(r):
    """name, flag and position: what an eqx run's record and the off run's share"""
    tid, pos = struct.unpack_from("<ii", r, 4)
    return r[36:36 + r[12]], struct.unpack_from("<H", r, 18)[0], tid, pos


@pytest.mark.gpu
def test_bam_to_bam_with_eqx(tmp_path):
    """11. run_bam_to_bam(device_records=True, device_batch=True, emit_eqx=True) on the 2 000-read synthetic BAM of test_bam_to_bam_with_md:
    alone, with emit_nm + emit_md + sorted_runs + index_runs, and off"""
    import bamcheck
    import index_expect as ixx

    from portello_amd import pipeline

    w = synth.generate(synth.config("chr20", n_reads=2_000), device="cuda")
    inp = str(tmp_path / "reads.bam")
    meta = bamsynth.write_read_bam(w, inp, level=1, n_threads=8)
    ixd = w.index_data()
    index = api.Index(w.index_data_device())
    cn, rn = meta["contig_names"], bamsynth.ref_names(w)
    lens = [int(s.numel()) for s in w.chrom_seq]
    with pytest.raises(ValueError, match="device_records"):
        pipeline.run_bam_to_bam(inp, str(tmp_path / "x.bam"), index, ixd, cn, rn, lens, emit_eqx=True)
    kw = dict(window_reads=700, n_workers=2, io_threads=8, device_records=True, device_batch=True)
    outs = {}
    for name, extra in (("eqx", dict(emit_eqx=True)), ("all", dict(emit_eqx=True, emit_nm=True, emit_md=True, sorted_runs=True, index_runs=True)), ("off", dict(emit_eqx=False))):
        (tmp_path / name).mkdir()
        outp = str(tmp_path / name / "lifted.bam")
        st = pipeline.run_bam_to_bam(inp, outp, index, ixd, cn, rn, lens, **kw, **extra)
        assert st.reads == w.n_reads
        outs[name] = (outp, st)
    for name in ("eqx", "all"):
        assert outs[name][1].eqx_device_ms > 0 and outs[name][1].lift_detail_s.get("eqx", 0) > 0
    assert outs["off"][1].eqx_device_ms == 0 and "eqx" not in outs["off"][1].lift_detail_s
    assert outs["all"][1].nm_device_ms > 0 and outs["all"][1].md_device_ms > 0 and outs["eqx"][1].nm_device_ms == 0 and outs["eqx"][1].md_device_ms == 0

    records_of = lambda path: bamcheck.read_bam(path)[2]
    chroms = ixd.chrom_seq
    off_recs = records_of(outs["off"][0])
    assert len(off_recs) == outs["off"][1].records_out
    by_key = {}  # -> [(the off run's record, the same with its CIGAR replaced by eqx_expect over its own bytes)]
    for r in off_recs:
        by_key.setdefault(record_key(r), []).append((r, r if is_unmapped(r) else ex.splice_cigar(r, ex.eqx_of_record(r, chroms))))
    run_paths = outs["all"][1].out_paths
    assert len(run_paths) >= 2 and outs["all"][1].index_paths == [p + ".bai" for p in run_paths]
    for name, paths in (("eqx", [outs["eqx"][0]]), ("all", run_paths)):
        recs = [r for p in paths for r in records_of(p)]
        assert len(recs) == len(off_recs) == outs[name][1].records_out
        n_lifted, n_x, used = 0, 0, {}
        for r in recs:
            k = record_key(r)
            cand = by_key[k]
            if is_unmapped(r):  # unmapped copies are untouched
                assert r in [o for o, _ in cand]
                continue
            n_lifted += 1
            bare = r
            if name == "all":
                bare, vals = mx.strip_md(bare)
                bare, nms = nx.strip_nm(bare)
            want = [e for o, e in cand if not is_unmapped(o)]
            assert bare in want, k
            used[k] = used.get(k, 0) + 1
            ops = nx.record_alignment(r)[3]
            n_x += int(ex.X in (ops & 15))
            assert 0 not in (ops & 15)
            if name == "all":  # NM and MD of the = / X record are those of the M record
                o = [o for o, e in cand if e == bare][0]
                assert nms == [nx.nm_of_record(o, chroms)] == [ex.n_edits(ops)] and vals == [mx.md_of_record(o, chroms)]
        assert n_lifted == outs[name][1].lifted > 1000 and n_x > 0
        assert all(used.get(k, 0) == sum(1 for o, _ in v if not is_unmapped(o)) for k, v in by_key.items())
    # the .bai of the combined run answers region queries like a brute-force scan
    largest = max(run_paths, key=os.path.getsize)
    blob, bai_blob = open(largest, "rb").read(), open(largest + ".bai", "rb").read()
    assert bai_blob == ixx.expected_bai(blob)
    recs, bai = ixx.bam_layout(blob)[0], ixx.parse_bai(bai_blob)
    starts = sorted(struct.unpack_from("<i", r, 8)[0] for r in records_of(largest) if not is_unmapped(r))
    regs = [(0, 0, lens[0]), (0, 7, 7)] + [(0, max(0, p - d), min(lens[0], p + d)) for p in starts[::max(1, len(starts) // 6)] for d in (1, 3000)]
    hits = 0
    for r, a, b in regs:
        got, want = ixx.query(blob, bai, r, a, b), ixx.brute(recs, r, a, b)
        assert got == want, (r, a, b, len(got), len(want))
        hits += bool(want)
    assert hits > 5
    index.close()
