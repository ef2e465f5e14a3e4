"""The reference FASTA loaded on the device (plo_fasta_*, portello_amd/csrc/fasta_core.hpp; plo_fasta_load_file).

The yardstick is tests/fasta_expect.py, the rule of include/portello_liftover.h restated a line at a time, itself pinned by the hand-worked
vectors of tests/golden/fasta_vectors.json (the first of them the reference's own test).  All comparisons are of integers and bytes.  The CPU
tests run fasta_core.hpp -- the kernels' bodies and the host's carry between the pieces -- under the wave emulator (tests/emu/emu_fasta.cpp)
with several wave counts and lane orders, and once more in a program built with AddressSanitizer + UBSan where every array sits in a heap
block of its exact size; the GPU tests run the C ABI on the device."""
import json
import os

import numpy as np
import pytest

import emu_fasta_lib as efl
import fasta_expect as fx
from portello_amd import abi, api, bam, bamsynth, fasta, synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = json.load(open(os.path.join(HERE, "golden", "fasta_vectors.json"), encoding="utf-8"))["cases"]
ACGT = np.frombuffer(b"ACGTNacgtn", np.uint8)


def gold_text(c):
    return c["text"].encode("latin-1")


def gold_want(c):
    w = c.get("want")
    return (w["names"], w["lens"]) if w else (None, None)


# ---- the texts ----------------------------------------------------------------------------------------------------------------------------
def make_text(n_bytes, width, seed, crlf=False, n_records=3):
    """a well-formed FASTA of exactly n_bytes bytes (cut anywhere: the rule has an answer for every cut)"""
    rng = np.random.default_rng(seed)
    eol = b"\r\n" if crlf else b"\n"
    parts, size, k = [], 0, 0
    per = max(1, n_bytes // max(1, n_records))
    while size < n_bytes:
        head = b">r%d some words" % k + eol
        body = ACGT[rng.integers(0, len(ACGT), per)].tobytes()
        rec = head + b"".join(body[i:i + width] + eol for i in range(0, len(body), width))
        parts.append(rec)
        size += len(rec)
        k += 1
    return b"".join(parts)[:n_bytes]


def seam_text(T, left, right, seed=3):
    """a FASTA whose byte T - 1 is the last of `left` and whose byte T is the first of `right`"""
    rng = np.random.default_rng(seed)
    head = b">first\n"
    fill = T - len(head) - len(left)
    body = ACGT[rng.integers(0, 4, fill)].tobytes()
    text = head + body + left + right + b"\nACGTTGCA\n>tail\nGG\n"
    assert text[T - 1:T] == left[-1:] and text[T:T + 1] == right[:1]
    return text


FEATURE = (b"\n \r\n>one first record\nACGTacgtNN\nAC\n\n>two\tdesc > x 1 *\r\nGGCCggcc\r\nTT\r\n>\nA\n>empty\n>three\nnnnnACGTRYKM \t\nAC\n"
           b">a_rather_long_identifier_that_a_cut_will_split|with|bars\nTTTTTTTTTTGGGGGGGGGGCCCCCCCCCCAAAAAAAAAA\nacgtacgtacgtacgtac\n>last\nG")


def tile_cases():
    T = efl.tile()
    cases = {}
    for n in (0, 1, T - 1, T, T + 1, 3 * T + 7):
        cases[f"bytes_{n}"] = make_text(n, 60, 100 + n % 97)
    for wdt in (1, 15, 16, 17, 60, 63, 64, 65):
        cases[f"width_{wdt}"] = make_text(T + 300, wdt, 7 + wdt, crlf=(wdt % 2 == 0))
    rng = np.random.default_rng(5)
    cases["twenty_tiles"] = make_text(19 * T + 77, 61, 9, n_records=7)  # (fa_states gives a lane eight neighbouring tiles)
    cases["sequence_line_longer_than_two_tiles"] = b">long\n" + ACGT[rng.integers(0, len(ACGT), 2 * T + 50)].tobytes() + b"\n>next\nAC\n"
    cases["header_line_longer_than_a_tile"] = b">id " + b"x>1*" * (T // 4 + 9) + b"\nACGT\n>b\nGG\n"
    cases["newline_ends_a_tile_gt_opens_the_next"] = seam_text(T, b"\n", b">seam description")
    cases["gt_ends_a_tile"] = seam_text(T, b"\n>", b"seam\tdescription")
    cases["cr_ends_a_tile_newline_opens_the_next"] = seam_text(T, b"AC\r", b"\nGT")
    cases["sequence_byte_ends_a_tile_line_goes_on"] = seam_text(T, b"A", b"C")
    return cases


# ---- the comparisons ------------------------------------------------------------------------------------------------------------------
def check_emulated(got, exp, want_names, text, what=""):
    assert got.canary_ok, what
    assert got.err_kind == exp.err_kind and got.status == (abi.PLO_ERR_DATA if exp.err_kind else abi.PLO_OK), (what, got.err_kind, got.err_offset, exp.err_kind, exp.err_offset)
    if exp.err_kind:
        assert (got.err_offset, got.err_chrom, got.err_len) == (exp.err_offset, exp.err_chrom, exp.err_len), what
        assert got.chrom_dst == [] and got.chrom_len == [], what  # a refused load hands out no sequence
        if exp.err_kind in (fx.ERR_BAD_BYTE, fx.ERR_NO_HEADER):
            return
    assert got.text_bytes == len(text) and got.n_bases == exp.n_bases, what
    assert (got.ids, got.lens, got.wants) == (exp.ids, exp.lens, fx.want_index(exp, want_names)), what
    if exp.err_kind:
        return
    assert got.chrom_len == exp.chrom_len, what
    assert got.chrom_seq() == exp.chrom_seq, what
    # every slot starts at a multiple of 256, has at least 16 bytes, and whatever is no base of a chromosome is zero
    at, mask = 0, np.ones(len(got.alloc), bool)
    for d, n in zip(got.chrom_dst, got.chrom_len):
        assert d % fx.ALIGN == 0 and d == at, what
        at = d + fx.slot_bytes(n)
        mask[d:d + n] = False
    assert len(got.alloc) >= at and not np.frombuffer(got.alloc, np.uint8)[mask].any(), what


def emulate_many(cases):
    """cases of efl.load_many, each checked against the expectation -> [Got]"""
    res = efl.load_many(cases)
    for c, got in zip(cases, res):
        check_emulated(got, fx.load(c["text"], c.get("want_names"), c.get("want_lens")), c.get("want_names"), c["text"], {k: v for k, v in c.items() if k != "text"})
    return res


def emulate(text, want=(None, None), **kw):
    return emulate_many([dict(text=text, want_names=want[0], want_lens=want[1], **kw)])[0]


# ---- 0. the expectation itself against the hand-worked vectors ------------------------------------------------------------------------
def test_expectation_gives_the_golden_vectors():
    assert GOLD[0]["name"] == "reference_foo" and GOLD[0]["src"].startswith("lib/rust-vc-utils/src/genome_ref.rs")
    for c in GOLD:
        e = fx.load(gold_text(c), *gold_want(c))
        if "err" in c:
            g = c["err"]
            assert (e.err_kind, e.err_offset, e.err_chrom, e.err_len) == (g["kind"], g.get("offset", 0), g.get("chrom", 0), g.get("len", 0)), c["name"]
            assert e.chrom_seq == [] and e.chrom_len == []
        else:
            assert e.err_kind == 0 and [i.decode("latin-1") for i in e.ids] == c["ids"] and [s.decode() for s in e.seqs] == c["seqs"], c["name"]
            assert [s.decode() for s in e.chrom_seq] == c.get("chrom_seq", c["seqs"]), c["name"]


# ---- 1. CPU: the emulator against the expectation -------------------------------------------------------------------------------------
def test_emulated_hand_cases():
    cases = [dict(text=gold_text(c), want_names=gold_want(c)[0], want_lens=gold_want(c)[1], vec=vec, order_seed=int(vec)) for c in GOLD for vec in (True, False)]
    for (c, vec), got in zip([(c, v) for c in GOLD for v in (True, False)], emulate_many(cases)):
        if "err" not in c:  # and against the vector itself
            assert [s.decode() for s in got.chrom_seq()] == c.get("chrom_seq", c["seqs"]), c["name"]


def test_emulated_sizes_around_the_tile():
    cases = [dict(text=text, **kw) for text in tile_cases().values()
             for kw in (dict(n_waves=1), dict(n_waves=3, order_seed=11), dict(n_waves=2, order_seed=4, vec=False))]
    assert all(fx.load(t).err_kind == 0 for t in tile_cases().values())
    emulate_many(cases)
    T = efl.tile()
    seam = fx.load(tile_cases()["gt_ends_a_tile"])
    assert seam.ids[1] == b"seam" and seam.offs[1] == T - 1  # (the cases are what their names say)
    assert fx.load(tile_cases()["newline_ends_a_tile_gt_opens_the_next"]).offs[1] == T


def test_emulated_pieces_cut_anywhere():
    text = FEATURE
    assert 150 <= len(text) <= 260
    exp = fx.load(text)
    assert exp.err_kind == 0 and exp.ids[2] == b"" and exp.lens[3] == 0 and b"R" in exp.seqs[4] and len(exp.ids) == 7
    ref = emulate(text, n_waves=1)
    cases = [dict(text=text, cuts=[cut, len(text) - cut], n_waves=1 + cut % 2, order_seed=cut % 3, vec=bool(cut % 5)) for cut in range(len(text) + 1)]  # two pieces cut at every offset
    cases.append(dict(text=text, cuts=[1] * len(text), n_waves=1))  # pieces of one byte
    cases.append(dict(text=text, cuts=[x for _ in range(len(text) // 2) for x in (0, 2, 0)] + [len(text) % 2, 0], n_waves=1, order_seed=2))  # empty pieces between
    for c, got in zip(cases, emulate_many(cases)):
        assert (got.alloc, got.ids, got.lens, got.chrom_dst, got.status) == (ref.alloc, ref.ids, ref.lens, ref.chrom_dst, 0), c["cuts"]
    # a record that spans three pieces, with a wanted list, several wave counts and lane orders
    T = efl.tile()
    big = make_text(2 * T + 500, 60, 77, n_records=2)
    e2 = fx.load(big)
    want = ([i.decode() for i in e2.ids[::-1]], e2.lens[::-1])
    one = emulate(big, want)
    for cuts, kw in (([T // 2, T, len(big) - T - T // 2], dict(n_waves=2, order_seed=9)), ([T - 1, 2, len(big) - T - 1], dict(n_waves=4, order_seed=2, vec=False)),
                     ([7, T + 1, 0, len(big) - T - 8], dict(n_waves=1, order_seed=5))):
        got = emulate(big, want, cuts=cuts, **kw)
        assert got.alloc == one.alloc


def test_emulated_wanted_list():
    text = b">u0\nACGT\n>w_b\n" + b"ACGTACGTAC\n" * 30 + b">u1 x\nGGGG\nCC\n>w_a\nacgtnACGTNNNNNNN\n>w_c\nTTTTT\n>u2\nAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAA\n"
    want = (["w_a", "w_b", "w_c"], [16, 300, 5])  # file order b, a, c; unwanted records in front, between and behind
    got = emulate(text, want, n_waves=2, order_seed=3)
    assert got.chrom_dst == [0, 256, 768] and len(got.alloc) == 1024 and got.wants == [-1, 1, -1, 0, 2, -1]
    assert emulate(text, want, cuts=[40, 200, len(text) - 240], vec=False).alloc == got.alloc


def test_emulated_refusals():
    # two offenders: the lowest decides, wherever the pieces are cut and whichever wave sees which
    T = efl.tile()
    base = bytearray(make_text(2 * T + 100, 60, 21))
    body = [i for i in range(len(base)) if base[i] in b"ACGTN" and base[i - 1] in b"ACGTN"]
    lo, hi = body[len(body) // 3], body[-5]
    assert lo < T < hi
    for bad in (b"1", b"*", b">", b"\x80", b"\0", b"-"):
        t = bytearray(base)
        t[lo:lo + 1] = bad
        t[hi:hi + 1] = b"7"
        for kw in (dict(), dict(cuts=[lo, 1, len(t) - lo - 1], n_waves=3, order_seed=8), dict(cuts=[hi, len(t) - hi])):
            got = emulate(bytes(t), **kw)
            assert (got.err_kind, got.err_offset) == (fx.ERR_BAD_BYTE, lo)
    t = b"\n\r\n" + bytes(base[base.index(b"\n") + 1:])  # the first header line gone: the first base is the offender, not the later ones
    got = emulate(t, cuts=[2, 5, len(t) - 7])
    assert (got.err_kind, got.err_offset) == (fx.ERR_NO_HEADER, 3)
    # the wanted list
    text = b">a\n" + b"ACGTACGTAC\n" * 60 + b">b\nGGGGCCCC\n>c\nTT\n"
    for want, lens, kind, chrom, length in ((["a", "zz", "b", "yy"], [600, 1, 8, 1], fx.ERR_MISSING, 1, 0), (["a", "b"], [600, 9], fx.ERR_LENGTH, 1, 8),
                                            (["b", "a", "c"], [8, 4, 3], fx.ERR_LENGTH, 1, 600)):
        got = emulate(text, (want, lens), n_waves=2, order_seed=6)
        assert (got.err_kind, got.err_chrom, got.err_len) == (kind, chrom, length)
    # a record longer than wanted stores nothing outside its slot: the neighbours' slots and the canaries are intact, its length is counted to the end
    got = efl.load(text, ["b", "a", "c"], [8, 4, 2], cuts=[100, len(text) - 100])
    assert (got.status, got.err_kind, got.err_chrom, got.err_len, got.canary_ok) == (abi.PLO_ERR_DATA, fx.ERR_LENGTH, 1, 600, True)
    assert len(got.alloc) == 768 and got.alloc[:8] == b"GGGGCCCC" and got.alloc[256:260] == b"ACGT" and got.alloc[512:514] == b"TT"
    assert not any(got.alloc[8:256]) and not any(got.alloc[260:512]) and not any(got.alloc[514:])
    dup = b">a\nAC\n>b\nGG\n>a\nTTTT\n>b\nC\n"
    got = emulate(dup, (["b", "a"], [2, 2]), cuts=[13, len(dup) - 13])
    assert (got.err_kind, got.err_offset, got.err_chrom, got.err_len) == (fx.ERR_DUPLICATE, 12, 1, 2)


def test_asan_program(tmp_path):
    """the same harness as a program of its own with AddressSanitizer + UBSan, every array in a heap block of its exact size"""
    cases = [dict(text=gold_text(c), want_names=gold_want(c)[0], want_lens=gold_want(c)[1], vec=bool(i & 1)) for i, c in enumerate(GOLD)]
    for i, (name, text) in enumerate(tile_cases().items()):
        cases.append(dict(text=text, n_waves=1 + i % 3, order_seed=i, vec=bool(i & 1)))
        if len(text) > 10:
            cases.append(dict(text=text, cuts=[len(text) // 3, 1, len(text) - len(text) // 3 - 1], n_waves=2, order_seed=i + 1))
    cases += [dict(text=FEATURE, cuts=[c, len(FEATURE) - c], n_waves=1) for c in range(0, len(FEATURE) + 1, 9)]
    cases.append(dict(text=FEATURE, cuts=[1] * len(FEATURE), n_waves=1))
    long_rec = b">a\n" + b"ACGTACGTAC\n" * 60 + b">b\nGGGGCCCC\n>c\nTT\n"
    cases.append(dict(text=long_rec, want_names=["b", "a", "c"], want_lens=[8, 4, 2], cuts=[100, len(long_rec) - 100]))
    cases.append(dict(text=long_rec, want_names=["b", "a", "c"], want_lens=[8, 600, 2], vec=False))
    rc, err, res = efl.run_asan(cases, str(tmp_path))
    assert rc == 0, err[-3000:]
    for c, got in zip(cases, res):
        check_emulated(got, fx.load(c["text"], c.get("want_names"), c.get("want_lens")), c.get("want_names"), c["text"], c.get("cuts"))


# ---- 2. CPU: the host side ------------------------------------------------------------------------------------------------------------
def test_struct_sizes():
    import ctypes as C

    assert C.sizeof(abi.PloFastaWant) == 8 + 8 + 8
    # u32 (+4) | 2 pointers | 3 u64 | float + i32 | u64 | u32 (+4) | i64
    assert C.sizeof(abi.PloFastaOut) == 8 + 16 + 24 + 8 + 8 + 8 + 8
    assert abi.PloFastaOut.fasta_ms.offset == 48 and abi.PloFastaOut.err_kind.offset == 52 and abi.PloFastaOut.err_len.offset == 72


def test_file_refusals_need_no_device(tmp_path):
    gz = tmp_path / "ref.fa.gz"
    gz.write_bytes(b"\x1f\x8b\x08\x00" + bytes(20))
    with pytest.raises(api.PortelloError) as e:
        fasta.load_reference(str(gz))
    assert e.value.status == abi.PLO_ERR_DATA and "gzip" in str(e.value) and "compress" in str(e.value)
    with pytest.raises(api.PortelloError) as e:
        fasta.load_reference(str(tmp_path / "is_not_there.fa"))
    assert e.value.status == abi.PLO_ERR_IO and "is_not_there.fa" in str(e.value)
    with pytest.raises(api.PortelloError) as e:  # a directory opens and does not read
        fasta.load_reference(str(tmp_path))
    assert e.value.status == abi.PLO_ERR_IO


class _Chroms:
    def __init__(self, seqs):
        self.chrom_seq = seqs


@pytest.mark.parametrize("width,lower,crlf", [(60, 0.0, False), (17, 0.3, True), (1, 1.0, False)])
def test_write_reference_fasta_round_trips(tmp_path, width, lower, crlf):
    w = synth.generate(synth.config("tiny", n_reads=20, seed=5, chrom_lens=(3_001, 120, 61)))
    path = str(tmp_path / "ref.fa")
    text = bamsynth.write_reference_fasta(w, path, width=width, lower_frac=lower, crlf=crlf)
    assert open(path, "rb").read() == text and (b"\r\n" in text) == crlf
    e = fx.load(text)
    assert e.err_kind == 0 and [i.decode() for i in e.ids] == bamsynth.ref_names(w)
    assert e.seqs == [s.numpy().tobytes() for s in w.chrom_seq]
    if lower > 0:
        assert any(97 <= b <= 122 for b in text.split(b"\n", 1)[1][:2000])
    longest = max(len(l.rstrip(b"\r")) for l in text.split(b"\n") if not l.startswith(b">"))
    assert longest == width


# ---- 3. GPU: the C ABI ----------------------------------------------------------------------------------------------------------------
def check_device(ref, exp, want_names, text):
    assert ref.chrom_len == exp.chrom_len
    assert (ref.record_ids, ref.record_lens, ref.record_want) == (exp.ids, exp.lens, fx.want_index(exp, want_names))
    assert ref.stats["n_bases"] == exp.n_bases and ref.stats["text_bytes"] == len(text) and ref.stats["n_records_seen"] == len(exp.ids)
    at = None
    for c, (p, n) in enumerate(zip(ref.chrom_ptrs, ref.chrom_len)):
        assert p % fx.ALIGN == 0 and (at is None or p == at)  # one allocation, slot behind slot
        at = p + fx.slot_bytes(n)
        slot = ref.download_bytes(p, fx.slot_bytes(n)).tobytes()
        assert slot[:n] == exp.chrom_seq[c], (c, slot[:60], exp.chrom_seq[c][:60])
        assert not any(slot[n:])


def device_load(text, want=(None, None), cuts=None, hint=None):
    pieces = [text] if cuts is None else [text[sum(cuts[:i]):sum(cuts[:i + 1])] for i in range(len(cuts))]
    assert b"".join(pieces) == text
    exp = fx.load(text, *want)
    if exp.err_kind:
        with pytest.raises(fasta.FastaError) as e:
            fasta.load_reference_bytes(pieces, *want, text_bytes_hint=len(text) if hint is None else hint)
        assert e.value.status == abi.PLO_ERR_DATA
        assert (e.value.kind, e.value.offset, e.value.chrom, e.value.length) == (exp.err_kind, exp.err_offset, exp.err_chrom, exp.err_len), (text[:60], e.value)
        return None
    ref = fasta.load_reference_bytes(pieces, *want, text_bytes_hint=len(text) if hint is None else hint)
    check_device(ref, exp, want[0], text)
    return ref


@pytest.mark.gpu
def test_device_hand_cases_and_refusals():
    for c in GOLD:
        ref = device_load(gold_text(c), gold_want(c))
        if ref is not None:
            assert [ref.download(i).tobytes().decode() for i in range(len(ref.chrom_len))] == c.get("chrom_seq", c["seqs"]), c["name"]
            if "want" in c:
                assert ref.names == c["want"]["names"]
            ref.close()
    text = b">a\n" + b"ACGTACGTAC\n" * 60 + b">b\nGGGGCCCC\n>c\nTT\n"
    device_load(text, (["b", "a", "c"], [8, 4, 2]), cuts=[100, len(text) - 100])  # LENGTH, longer than its slot
    T = efl.tile()
    base = bytearray(make_text(2 * T + 100, 60, 21))
    body = [i for i in range(len(base)) if base[i] in b"ACGTN" and base[i - 1] in b"ACGTN"]
    lo, hi = body[len(body) // 3], body[-5]
    base[lo:lo + 1], base[hi:hi + 1] = b"*", b"7"
    for cuts in (None, [lo, 1, len(base) - lo - 1], [hi, len(base) - hi]):
        device_load(bytes(base), cuts=cuts)


@pytest.mark.gpu
def test_device_sizes_around_the_tile(monkeypatch):
    for name, text in tile_cases().items():
        ref = device_load(text, hint=0 if "width" in name else None)  # (hint 0: the output allocation has to grow)
        ref.close()
    monkeypatch.setenv("PLO_FASTA_BYTESTORES", "1")  # k_fa_emit<false>: every base a store of its own
    for name in ("bytes_%d" % (3 * efl.tile() + 7), "width_17", "cr_ends_a_tile_newline_opens_the_next"):
        device_load(tile_cases()[name]).close()


@pytest.mark.gpu
def test_device_pieces_and_wanted_list():
    text = FEATURE
    for cut in list(range(0, len(text) + 1, 7)) + [len(text)]:
        device_load(text, cuts=[cut, len(text) - cut]).close()
    device_load(text, cuts=[1] * len(text)).close()
    device_load(text, cuts=[x for _ in range(len(text) // 2) for x in (0, 2, 0)] + [len(text) % 2, 0]).close()
    T = efl.tile()
    big = make_text(2 * T + 500, 60, 77, n_records=2)
    e2 = fx.load(big)
    want = ([i.decode() for i in e2.ids[::-1]], e2.lens[::-1])
    for cuts in (None, [T // 2, T, len(big) - T - T // 2], [T - 1, 2, len(big) - T - 1], [7, T + 1, 0, len(big) - T - 8]):
        device_load(big, want, cuts=cuts).close()
    text = b">u0\nACGT\n>w_b\n" + b"ACGTACGTAC\n" * 30 + b">u1 x\nGGGG\nCC\n>w_a\nacgtnACGTNNNNNNN\n>w_c\nTTTTT\n>u2\nAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAAA\n"
    ref = device_load(text, (["w_a", "w_b", "w_c"], [16, 300, 5]), cuts=[40, 200, len(text) - 240])
    assert [p - ref.chrom_ptrs[0] for p in ref.chrom_ptrs] == [0, 256, 768] and ref.names == ["w_a", "w_b", "w_c"]
    ref.close()


@pytest.mark.gpu
@pytest.mark.parametrize("crlf", [False, True], ids=["lf", "crlf"])
def test_load_file_of_8_mb_in_pieces(tmp_path, crlf):
    """plo_fasta_load_file over a file of three records and about 8 MB read in pieces of 1 MiB: every byte and every length"""
    rng = np.random.default_rng(31)
    seqs = [np.frombuffer(b"ACGTN", np.uint8)[rng.integers(0, 5, n)] for n in (5_000_003, 2_500_000, 377_777)]
    path = str(tmp_path / "ref.fa")
    text = bamsynth.write_reference_fasta(_Chroms(seqs), path, width=60, lower_frac=0.3, crlf=crlf)
    assert len(text) > 7_900_000 and sum(97 <= b <= 122 for b in text[:100_000]) > 20_000
    names, lens = ["chr3", "chr1", "chr2"], [len(seqs[2]), len(seqs[0]), len(seqs[1])]
    ref = fasta.load_reference(path, names, lens, piece_bytes=1 << 20)
    assert ref.chrom_len == lens and ref.names == names and ref.record_ids == [b"chr1", b"chr2", b"chr3"] and ref.record_lens == [len(s) for s in seqs]
    assert ref.stats["text_bytes"] == len(text) and ref.stats["n_bases"] == sum(lens) and ref.stats["fasta_ms"] > 0
    for c, k in enumerate((2, 0, 1)):
        assert np.array_equal(ref.download(c), seqs[k]), c
    ref.close()
    every = fasta.load_reference(path, piece_bytes=(3 << 20) + 4097)  # without a list: file order, the allocation sized by the file; pieces of more than 512 tiles
    assert every.chrom_len == [len(s) for s in seqs] and every.names == ["chr1", "chr2", "chr3"]
    for c in range(3):
        assert np.array_equal(every.download(c), seqs[c]), c
    every.close()


@pytest.mark.gpu
def test_wrong_length_is_refused_and_the_next_load_works(tmp_path):
    w = synth.generate(synth.config("tiny", n_reads=20, seed=5, chrom_lens=(3_001, 120, 61)))
    path = str(tmp_path / "ref.fa")
    bamsynth.write_reference_fasta(w, path, lower_frac=0.2)
    names = bamsynth.ref_names(w)
    with pytest.raises(fasta.FastaError) as e:
        fasta.load_reference(path, names, [3_001, 121, 61])
    assert e.value.status == abi.PLO_ERR_DATA and (e.value.kind, e.value.chrom, e.value.length) == (abi.FA_ERR_LENGTH, 1, 120)
    assert 'Chromosome "chr2" specified with inconsistent length: 121 in the assembly-to-ref alignment file, and 120 in the reference fasta' in str(e.value)
    with pytest.raises(fasta.FastaError) as e:
        fasta.load_reference(path, names + ["chrUn"], [3_001, 120, 61, 5])
    assert (e.value.kind, e.value.chrom) == (abi.FA_ERR_MISSING, 3)
    assert 'Chromosome "chrUn" specified in the assembly-to-ref alignment file, but not in the reference fasta' in str(e.value)
    ref = fasta.load_reference(path, names, [3_001, 120, 61])
    for c, s in enumerate(w.chrom_seq):
        assert ref.download(c).tobytes() == s.numpy().tobytes()
    ref.close()


@pytest.mark.gpu
def test_end_to_end_index_from_a_loaded_reference(tmp_path):
    """both phases from files and the reference from its FASTA: the lifted window's records, with NM:i and MD:Z, equal record for record
    what the same calls give over an index built from the host arrays"""
    import test_md_dev as tmd
    import test_nm_dev as tnd
    import test_records_dev as trd

    w = synth.generate(synth.config("tiny", n_reads=300, seed=411, split_read_frac=0.3, sorted_reads=True))  # the small_bam recipe
    asm, reads, fa = str(tmp_path / "asm.bam"), str(tmp_path / "reads.bam"), str(tmp_path / "ref.fa")
    bamsynth.write_contig_bam(w, asm, seed=3)
    meta = bamsynth.write_read_bam(w, reads, level=6, n_unmapped=4)
    bamsynth.write_reference_fasta(w, fa, width=60, lower_frac=0.3)
    rd, win = trd.open_window(reads)
    ph = bam.Phase1(asm, rd.ref_names, rd.ref_lens, n_threads=2)
    ref = fasta.load_reference(fa, ph.ref_names, ph.ref_lens)
    out = {}
    for name, ixd in (("host", ph.index_data([s.numpy() for s in w.chrom_seq])), ("device", ph.index_data_device(ref))):
        assert ixd.seq_mem == (abi.MEM_DEVICE if name == "device" else abi.MEM_HOST)
        assert (name == "device") == any(k is ref for k in ixd._keep)  # the description keeps the loader alive
        index = api.Index(ixd, 0)
        assert (name == "device") == any(k is ref for k in index.data._keep)  # and still does behind to_desc
        run = trd.DeviceRun(win, index, meta["contig_names"], ph.ref_names, False)
        run.finish()
        run.sa()
        item_nm, _ = tnd.device_nm(run)
        md_off, md_text, _ = tmd.device_md(run)
        rec = run.records()
        out[name] = (rec.data(), np.array(rec.record_off), rec.n_lifted, item_nm, md_off, md_text)
        run.eng.close()
        index.close()
    h, d = out["host"], out["device"]
    assert h[2] == d[2] > 100 and np.array_equal(h[1], d[1]) and np.array_equal(h[3], d[3]) and np.array_equal(h[4], d[4]) and h[5] == d[5]
    assert trd._split(d[0], d[1]) == trd._split(h[0], h[1]) and b"MDZ" in d[0]
    assert (h[3] > 0).any()  # the sample is not vacuous: reads differ from the reference
    win.close()
    rd.close()
    ph.close()
    ref.close()
