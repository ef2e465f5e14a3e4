"""Allele pileup and candidate sites on the device: plo_pileup_* (portello_amd/csrc/pileup_core.hpp), portello_amd.pileup and
run_bam_to_bam(pileup_out=...).

The yardstick is tests/pileup_expect.py -- the rule of include/portello_liftover.h restated in plain Python, a dict of counts per
(ref, pos, channel) -- and, for the yardstick itself, the hand-worked vectors of tests/golden/pileup_vectors.json.  All comparisons are of
integers and text.  The CPU tests run pileup_core.hpp under the wave emulator (tests/emu/emu_pileup.cpp) with PLO_PILEUP_TILE = 12, shuffled
lane orders and several wave counts -- every accepted add is repeated there by the one-thread form of the rule, and the two must agree --,
and once more in a program built with AddressSanitizer + UBSan where every array, every chromosome and the records sit in heap blocks of
their exact size.  The GPU tests run the C ABI on the device and the pipeline mode.

Mutations this file is meant to catch (each was tried on the wave part of pileup_core.hpp):
  * anchoring an I or S at rf - 1 even in front of the record's first base (no max with pos) fails
    test_hand_vectors["clips, a mismatch, an insertion, a deletion and an N"]: the leading clip leaves the record's span;
  * dropping the read position's carry across the 64-op seam (rd_done not taken over from the step) fails test_op_counts[65], [128] and
    [129]: the bases behind the seam are compared with the wrong ones."""
import ctypes as C
import json
import os
import random
import re
import struct
import threading

import numpy as np
import pytest

import depth_expect as dx
import emu_pileup_lib as epl
import index_expect as ix
import pileup_expect as px
from portello_amd import abi, api, pileup

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "pileup_vectors.json")))
T = epl.TILE
NO_RECORD = 0xFFFFFFFF
OP_COUNTS = [0, 1, 63, 64, 65, 128, 129]
CODES = "MIDNSHP=X"
TABLE = "=ACMGRSVTWYHKDBN"
OK, BAD = abi.PLO_OK, abi.PLO_ERR_INVALID_ARG


def cigar(text):
    out, n = [], ""
    for ch in text:
        if ch.isdigit():
            n += ch
        else:
            out.append(ix.op(int(n), CODES.index(ch)))
            n = ""
    return out


def pack(codes):
    c = list(codes) + [0] * (len(codes) & 1)
    return bytes((c[k] << 4) | c[k + 1] for k in range(0, len(c), 2))


def rec(ref, pos, flag=0, ops=(), seq=(), name=b"r", aux=b"", n_cigar=None, block_size=None, l_seq_says=None, cut=0):
    """a record with its bases (seq: letters of the table or 4-bit codes) and qualities in front of its aux fields; ops: words or CIGAR
    text; n_cigar / block_size / l_seq_says: the fields, when they shall lie; cut: bytes dropped from the end (block_size follows)"""
    ops = cigar(ops) if isinstance(ops, str) else list(ops)
    codes = [TABLE.index(ch) for ch in seq] if isinstance(seq, str) else list(seq)
    body = struct.pack("<iiBBHHHIiii", ref, pos, len(name), 0, 0, len(ops) if n_cigar is None else n_cigar, flag, len(codes) if l_seq_says is None else l_seq_says, -1, -1, 0) + name
    body += struct.pack("<%dI" % len(ops), *ops) + pack(codes) + bytes(17 + k % 20 for k in range(len(codes))) + aux
    if cut:
        body = body[:-cut]
    return struct.pack("<I", len(body) if block_size is None else block_size) + body


def cg_field(ops, count=None):
    return b"CGBI" + struct.pack("<I", len(ops) if count is None else count) + struct.pack("<%dI" % len(ops), *ops)


def placeholder(ref, pos, real, seq, flag=0, front=b"XAZabc\0NMi\x05\0\0\0", cg=True, count=None):
    """the real ops behind the placeholder <l_seq>S<ref_len>N"""
    ref_len = sum(o >> 4 for o in real if (o & 15) in dx.REF)
    return rec(ref, pos, flag, [ix.op(len(seq), 4), ix.op(ref_len, 3)], seq, b"long", front + (cg_field(real, count) if cg else b""))


def read_len(ops):
    return sum(o >> 4 for o in ops if (o & 15) in px.READ_OPS)


def ref_len_of(ops):
    return sum(o >> 4 for o in ops if (o & 15) in dx.REF)


def read_for(chrom, pos, ops, flips=(), rng=None):
    """the codes of a read that matches chrom under ops from pos (a reference byte that no code matches gets '='), random bases in I and S;
    flips: read positions that get a one-hot code the reference byte does not have"""
    rng = rng or random.Random(len(ops) * 131 + pos)
    out, rf = [], pos
    for o in ops:
        n, c = o >> 4, o & 15
        if c in (0, 7, 8):
            for k in range(n):
                c2 = TABLE.find(chr(chrom[rf + k]))
                out.append(c2 if 1 <= c2 <= 14 else 0)
            rf += n
        elif c in (1, 4):
            out += [rng.choice([1, 2, 4, 8, 15, 5]) for _ in range(n)]
        elif c in (2, 3):
            rf += n
    refpos = ref_positions(pos, ops)
    for k in flips:
        have = TABLE.find(chr(chrom[refpos[k]])) if refpos[k] is not None else -1
        out[k] = next(x for x in (1, 2, 4, 8) if x != have)
    return out


def ref_positions(pos, ops):
    """read position -> its reference position (None in I and S)"""
    out, rf = [], pos
    for o in ops:
        n, c = o >> 4, o & 15
        if c in (0, 7, 8):
            out += list(range(rf, rf + n))
            rf += n
        elif c in (1, 4):
            out += [None] * n
        elif c in (2, 3):
            rf += n
    return out


def golden_records(v):
    out = []
    for k, r in enumerate(v["records"]):
        if isinstance(r, dict):
            out.append(rec(r["ref"], r["pos"], r["flag"], r["cigar"], r["seq"], b"g%d" % k, l_seq_says=r.get("l_seq"), cut=r.get("cut", 0)))
        else:
            out.append(rec(r[0], r[1], r[2], r[3], r[4], b"g%d" % k))
    return out


def golden_chroms(v):
    return [c.encode("latin-1") for c in v["chroms"]]


def golden_regions(v):
    return [tuple(r) for r in v["regions"]] if v.get("regions") else None


def golden_counts(v):
    return {(r, p, px.NAMES.index(ch)): n for r, p, ch, n in v["counts"]}


def rand_chrom(rng, n, odd=0.03):
    return bytes(rng.choice(b"acgtnRY*\0Z") if rng.random() < odd else rng.choice(b"ACGTACGTACGTN") for _ in range(n))


def random_record(rng, chroms, k, max_ops=10):
    """a record that is valid by construction: its ops end inside its chromosome, its bases are as many as its ops consume"""
    while True:
        r = rng.randrange(len(chroms))
        ops = [ix.op(rng.choice([0, 1, 1, 2, rng.randrange(1, 9), rng.randrange(1, 40)]), rng.choice((0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 7, 8, 8, 11))) for _ in range(rng.randrange(max_ops + 1))]
        span = ref_len_of(ops)
        by_chance = len(ops) == 2 and ops[0] == ix.op(read_len(ops), 4) and ops[1] & 15 == 3  # the placeholder form: its aux fields would be walked
        if span <= len(chroms[r]) and not by_chance:
            break
    pos = rng.randrange(len(chroms[r]) - span + 1)
    n = read_len(ops)
    codes = read_for(chroms[r], pos, ops, rng=rng)
    for j in range(n):
        if rng.random() < 0.12:
            codes[j] = rng.choice([1, 2, 4, 8, rng.randrange(16)])
    flag = rng.choice([0, 0, 0, 0, 16, 0x800, 0x100, 0x400, 4, 1 | 16])
    form = rng.randrange(8)
    if form == 0:
        return placeholder(r, pos, ops, codes, flag)
    if form == 1:
        return rec(rng.choice([-1, r]), rng.choice([-1, pos]), flag | 4, ops, codes, b"u%d" % k)
    return rec(r, pos, flag, ops, codes, b"q" * (1 + k % 8), bytes(rng.randrange(256) for _ in range(rng.randrange(9))))


class Emu:
    def __init__(self, chroms, **kw):
        self.o = epl.EmuPileup(chroms, **kw)

    def __enter__(self):
        return self.o

    def __exit__(self, *a):
        self.o.close()


def same(a, b):
    return len(a) == len(b) and a.tobytes() == b.tobytes()


def emu_check(recs, chroms, regions=None, exclude=px.EXCLUDE_DEFAULT, what="", geometries=((0, 1), (1, 3), (2, 8)), depth=None, site_kw=None):
    """the emulated object against the restatement: slots, the add's outputs, the array element for element, the sites"""
    data, off = ix.concat(recs)
    ref_len = [len(c) for c in chroms]
    assert px.first_offender(data, off, ref_len, exclude) is None, what
    cnt, n_counted, n_events = px.counts(recs, chroms, regions, exclude)
    want = px.array(cnt, ref_len, regions)
    for seed, n_waves in geometries:
        with Emu(chroms, regions=regions, exclude=exclude) as o:
            assert o.slots() == px.slots(ref_len, regions), what
            assert o.add(data, off, seed, n_waves) == (OK, n_counted, NO_RECORD, 0, n_events), (what, seed)  # -4: the waves and the one-thread rule disagree
            got = o.array()
            assert np.array_equal(got, want) and int(got.sum()) == n_events, (what, seed)
            for kw in (site_kw or [dict(), dict(mask=0xFF), dict(mask=0x80), dict(min_count=2)]):
                st, sites = o.sites(depth=depth, order_seed=seed, **kw)
                assert st == OK and same(sites, px.sites(cnt, chroms, regions, depth, **kw)), (what, seed, kw)
    return cnt


# ---- CPU: the yardstick -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("v", GOLDEN["vectors"], ids=lambda v: v["name"])
def test_expectation_by_hand(v):
    """the restatement gives the hand-worked counts, and nothing else"""
    recs, chroms = golden_records(v), golden_chroms(v)
    assert px.first_offender(*ix.concat(recs), [len(c) for c in chroms]) is None
    assert px.counts(recs, chroms, golden_regions(v)) == (golden_counts(v), v["n_counted"], v["n_events"])


@pytest.mark.parametrize("v", GOLDEN["refused"], ids=lambda v: v["name"])
def test_expectation_of_refusals_by_hand(v):
    assert px.first_offender(*ix.concat(golden_records(v)), [len(c) for c in golden_chroms(v)]) == (v["err_record"], v["err_kind"])


def test_api_version_and_structs():
    assert abi.PLO_API_VERSION >= 20 and abi.PILEUP_CHANNELS == 8 == px.CHANNELS and abi.PILEUP_MASK_DEFAULT == 0x6F == px.MASK_DEFAULT
    assert C.sizeof(abi.PloPileupSite) == 48 == abi.PILEUP_SITE_DTYPE.itemsize and abi.PILEUP_SITE_DTYPE == px.SITE
    assert [(n, abi.PILEUP_SITE_DTYPE.fields[n][1]) for n in abi.PILEUP_SITE_DTYPE.names] == [(f[0], getattr(abi.PloPileupSite, f[0]).offset) for f in abi.PloPileupSite._fields_]
    assert C.sizeof(abi.PloPileupRegion) == 12 and C.sizeof(abi.PloPileupOpts) == 16 and abi.PloPileupOpts.regions.offset == 8
    assert C.sizeof(abi.PloPileupInfo) == 56 and abi.PloPileupInfo.bytes_allocated.offset == 40
    assert C.sizeof(abi.PloPileupAddOut) == 32 and abi.PloPileupAddOut.n_events.offset == 16 and abi.PloPileupAddOut.add_ms.offset == 24
    assert C.sizeof(abi.PloPileupSitesOpts) == 16 and C.sizeof(abi.PloPileupSitesOut) == 24 and abi.PloPileupSitesOut.sites_ms.offset == 16
    text = open(os.path.join(HERE, "..", "include", "portello_liftover.h")).read()
    assert re.search(r"#define PLO_API_VERSION (\d+)", text).group(1) == str(abi.PLO_API_VERSION) and "#define PLO_PILEUP_CHANNELS 8" in text
    for name, cls in (("plo_pileup_region", abi.PloPileupRegion), ("plo_pileup_opts", abi.PloPileupOpts), ("plo_pileup_info", abi.PloPileupInfo),
                      ("plo_pileup_add_out", abi.PloPileupAddOut), ("plo_pileup_sites_opts", abi.PloPileupSitesOpts), ("plo_pileup_site", abi.PloPileupSite),
                      ("plo_pileup_sites_out", abi.PloPileupSitesOut)):
        body = text[text.index("typedef struct %s {" % name):]
        body = body[:body.index("} %s;" % name)]
        declared = [n for line in body.splitlines()[1:] for n in re.findall(r"(\w+)(?:\[\w+\])?\s*(?:,|;)", line.split("/*")[0])]
        assert declared == [f[0] for f in cls._fields_], name


def test_writer(tmp_path):
    """the text of <prefix>.sites.tsv"""
    sites = np.array([(0, 4, 7, ord("A"), (0, 0, 0), (0, 3, 0, 0, 0, 0, 1, 0)), (2, 0, -1, 0, (0, 0, 0), (0, 0, 0, 0, 9, 8, 7, 6)), (2, 11, 0, ord("t"), (0, 0, 0), (1, 0, 0, 0, 0, 0, 0, 0))],
                     abi.PILEUP_SITE_DTYPE)
    p = str(tmp_path / "x.sites.tsv")
    pileup.write_sites(p, ["chr1", "empty", "chrM"], sites)
    assert open(p).read() == ("#chrom\tpos\tend\tref\tdepth\tA\tC\tG\tT\tN\tDEL\tINS\tCLIP\n" "chr1\t4\t5\tA\t7\t0\t3\t0\t0\t0\t0\t1\t0\n" "chrM\t0\t1\tN\t-1\t0\t0\t0\t0\t9\t8\t7\t6\n"
                              "chrM\t11\t12\tt\t0\t1\t0\t0\t0\t0\t0\t0\t0\n") == px.sites_text(["chr1", "empty", "chrM"], sites)
    pileup.write_sites(p, ["chr1"], sites[:0])
    assert open(p).read() == "#chrom\tpos\tend\tref\tdepth\tA\tC\tG\tT\tN\tDEL\tINS\tCLIP\n"


def test_pileup_out_needs_device_records(tmp_path):
    from portello_amd import pipeline

    with pytest.raises(ValueError, match="device_records"):
        pipeline.run_bam_to_bam("in.bam", str(tmp_path / "x.bam"), None, None, [], [], [], pileup_out=str(tmp_path / "p"))
    with pytest.raises(ValueError, match="pileup_min_count"):
        pipeline.run_bam_to_bam("in.bam", str(tmp_path / "x.bam"), None, None, [], [], [], device_records=True, pileup_out=str(tmp_path / "p"), pileup_min_count=0)


def test_context_and_build_know_the_new_file():
    from portello_amd import build

    assert "pileup_core.hpp" in build.HEADERS
    src = open(os.path.join(HERE, "..", "portello_amd", "csrc", "engine.hip")).read()
    assert "uint32_t plo_api_version(void) { return PLO_API_VERSION; }" in src and "k_pileup_check" in src and "k_pileup_add" in src and "k_pileup_sites<true>" in src


# ---- CPU: pileup_core.hpp under the wave emulator ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("v", GOLDEN["vectors"], ids=lambda v: v["name"])
def test_hand_vectors(v):
    """1. the hand vectors: the array holds the hand-worked counts and nothing else"""
    recs, chroms = golden_records(v), golden_chroms(v)
    cnt = emu_check(recs, chroms, golden_regions(v), what=v["name"])
    assert cnt == golden_counts(v)
    with Emu(chroms, regions=golden_regions(v)) as o:
        assert o.add(*ix.concat(recs)) == (OK, v["n_counted"], NO_RECORD, 0, v["n_events"])
        assert np.array_equal(o.array(), px.array(golden_counts(v), [len(c) for c in chroms], golden_regions(v)))


@pytest.mark.parametrize("v", GOLDEN["refused"], ids=lambda v: v["name"])
def test_hand_refusals(v):
    with Emu(golden_chroms(v)) as o:
        assert o.add(*ix.concat(golden_records(v))) == (BAD, 0, v["err_record"], v["err_kind"], 0) and not o.array().any()


def seam_ops(n_ops, kind):
    """n_ops ops around the 64-op seam.  kind 0: short matches of all three codes; kind 1: D, I and S sit on the ops 62 .. 65 and 127 .. 129;
    kind 2: N, P, H and ops of length 0 there"""
    ops = [ix.op(1 + k % 3, (7, 8, 0)[k % 3]) for k in range(n_ops)]
    special = {1: (2, 1, 4, 1, 2), 2: (3, 6, 5, 3, 6)}.get(kind)
    if special:
        for j, k in enumerate((62, 63, 64, 65, 127, 128, 129)):
            if k < n_ops:
                ops[k] = ix.op(0 if kind == 2 and j == 3 else 2, special[j % 5])
    return ops


CHROM_SEAM = rand_chrom(random.Random(3), 420)


@pytest.mark.parametrize("n_ops", OP_COUNTS)
def test_op_counts(n_ops):
    """2. op counts around the wave's width: the read and reference positions carry across the 64-op seam"""
    recs = []
    for kind in range(3):
        ops = seam_ops(n_ops, kind)
        n = read_len(ops)
        codes = read_for(CHROM_SEAM, 3 + kind, ops, flips=[k for k in (0, n // 2, n - 1) if n and ref_positions(3 + kind, ops)[k] is not None])
        recs.append(rec(0, 3 + kind, 0, ops, codes, b"s%d" % kind))
    cnt = emu_check(recs, [CHROM_SEAM], what=n_ops, geometries=((0, 1), (1, 2)))
    if n_ops >= 65:
        assert sum(n for (_, _, ch), n in cnt.items() if ch == px.DEL) >= 1 and sum(n for (_, _, ch), n in cnt.items() if ch == px.INS) >= (2 if n_ops > 65 else 1)  # (op 63 is an I, op 65 another)


def test_long_cigar_through_cg():
    """3. a 65 536-op record through the placeholder and CG:B,I; a placeholder without CG is taken as it stands"""
    rng = random.Random(5)
    real = [ix.op(1, rng.choice([7, 7, 8, 2, 1])) for _ in range(65536)]
    chrom = rand_chrom(rng, ref_len_of(real) + 150, odd=0)
    codes = read_for(chrom, 100, real, rng=rng)
    for k in range(0, len(codes), 97):
        codes[k] = 15
    recs = [rec(0, 3, 0, "5M", "TTTTT", b"short"), placeholder(0, 100, real, codes), placeholder(0, 20, cigar("4=2D4="), "ACGTACG", cg=False),
            rec(0, 0, 0, [ix.op(9, 4), ix.op(5, 3)], "ACGTACG", b"not the form", cg_field(cigar("7M")), l_seq_says=7)]
    # (the third: 7S10N as it stands -- one clip; the fourth: 9S is not l_seq, the in-record ops stand and disagree with l_seq)
    data, off = ix.concat(recs)
    assert px.first_offender(data, off, [len(chrom)]) == (3, px.ERR_LSEQ)
    cnt = emu_check(recs[:3], [chrom], what="long", geometries=((1, 2),), site_kw=[dict()])
    assert cnt[(0, 20, px.CLIP)] == 1 and sum(n for (_, _, ch), n in cnt.items() if ch == px.N) >= 300


def test_match_alignment():
    """4. an M op starting at every reference address mod 16 with lengths 1, 15, 16, 17, 33, at even and odd read positions; mismatches at
    the first and last base of the op and of every piece, and at the chromosome's first and last base"""
    rng = random.Random(9)
    chrom = rand_chrom(rng, 16 + 33 + 15, odd=0)
    recs = []
    for start in range(16):
        for n in (1, 15, 16, 17, 33):
            for odd in (0, 1):
                ops = ([ix.op(1, 4)] if odd else []) + [ix.op(n, 0)]
                flips = sorted({odd, odd + n - 1} | {odd + k for k in range(n) if (start + k) % 16 in (0, 15)})
                recs.append(rec(0, start, 0, ops, read_for(chrom, start, ops, flips), b"a" * (1 + (start + n) % 8)))
    last = len(chrom) - 33
    recs.append(rec(0, last, 0, "33M", read_for(chrom, last, cigar("33M"), [0, 32]), b"end"))
    recs.append(rec(0, 0, 0, "2M", read_for(chrom, 0, cigar("2M"), [0]), b"begin"))
    cnt = emu_check(recs, [chrom], what="alignment", geometries=((0, 2), (3, 5)), site_kw=[dict()])
    assert sum(n for (_, p, ch), n in cnt.items() if p == len(chrom) - 1 and ch < 4) == 1 and sum(n for (_, p, ch), n in cnt.items() if p == 0 and ch < 4) >= 3


def test_a_second_trip_of_pieces():
    """5. one op of 64 * 16 + 1 bases: its pieces need a second trip; sparse mismatches, and a read that mismatches everywhere"""
    rng = random.Random(11)
    n = 64 * 16 + 1
    chrom = rand_chrom(rng, n + 40, odd=0.01)
    ops = [ix.op(n, 0)]
    sparse = read_for(chrom, 7, ops, flips=[0, 15, 16, 1000, 1023, 1024, n - 1])
    recs = [rec(0, 7, 0, ops, sparse, b"sparse"), rec(0, 20, 16, [ix.op(n, 8)], [15] * n, b"every base"), rec(0, 1, 0, [ix.op(3, 4), ix.op(n, 7), ix.op(2, 1)], [15] * 3 + sparse + [1, 1], b"odd")]
    cnt = emu_check(recs, [chrom], what="second trip", geometries=((1, 2),), site_kw=[dict(mask=0xFF)])
    assert sum(n_ for (_, _, ch), n_ in cnt.items() if ch == px.N) >= n


@pytest.mark.parametrize("name_len", range(1, 9))
def test_read_names_move_the_bases(name_len):
    """6. read names of 1 to 8 bytes move the bases through every address mod 8: both paths of the piece rule, nothing outside the bases"""
    rng = random.Random(20 + name_len)
    chrom = rand_chrom(rng, 200, odd=0.02)
    recs = []
    for k, (pos, lead, n) in enumerate(((0, 0, 70), (5, 1, 64), (16, 2, 33), (31, 3, 96), (48, 0, 16), (100, 5, 100))):
        ops = ([ix.op(lead, 4)] if lead else []) + [ix.op(n, 0)]
        recs.append(rec(0, pos, 0, ops, read_for(chrom, pos, ops, flips=[lead, lead + n // 2, lead + n - 1]), b"n" * name_len, bytes(k)))
    emu_check(recs, [chrom], what=name_len, geometries=((name_len, 2),), site_kw=[dict()])


def test_every_code_against_every_byte():
    """7. every read code 0-15 against A C G T N, a lower-case byte, Z and 0 -- base by base and through the 16-base path"""
    col = b"ACGTNaZ\0"
    chrom = col + bytes(8) + col * 6 + b"MRWSYKVHDB=" + col
    recs = [rec(0, 0, 0, "8M", [c] * 8, b"c%d" % c) for c in range(16)]
    recs += [rec(0, 16, 0, [ix.op(48 + 11 + 8, 0)], [c] * 67, b"w%d" % c, bytes(c % 3)) for c in range(16)]
    cnt = emu_check(recs, [chrom], what="codes", geometries=((0, 1), (5, 4)), site_kw=[dict(), dict(mask=0x10)])
    assert cnt[(0, 0, px.C)] == 1 and cnt[(0, 0, px.N)] == 11 and (0, 0, px.A) not in cnt and cnt[(0, 4, px.N)] == 11 and cnt[(0, 6, px.N)] == 11 and cnt[(0, 6, px.A)] == 1


def test_indels_clips_and_empty_records():
    """8. I in front of the first M, between ops and at the end; D at the chromosome's last bases; N, H, P, leading and trailing S, ops of
    length 0; a record of only S and I; a record at pos == ref_len"""
    chrom = b"ACGTTGCAAC" * 3
    n = len(chrom)
    recs = [rec(0, 4, 0, "2I3M", read_for(chrom, 4, cigar("2I3M")), b"front"), rec(0, 4, 0, "3M2I3M", read_for(chrom, 4, cigar("3M2I3M")), b"between"),
            rec(0, 4, 0, "3M2I", read_for(chrom, 4, cigar("3M2I")), b"end"), rec(0, 0, 0, "1I1M", "CA", b"at 0"),
            rec(0, n - 5, 0, "2M3D", read_for(chrom, n - 5, cigar("2M3D")), b"D last"), rec(0, n - 1, 0, "1D", "", b"D only"), rec(0, n - 2, 0, "1M1D", "A", b"D at the last base"),
            rec(0, 2, 0, "2H3S2M4N1P2M0M0D0I0S3S1H", read_for(chrom, 2, cigar("2H3S2M4N1P2M0M0D0I0S3S1H")), b"all"), rec(0, 6, 0, "4S2I", "ACGTAC", b"S and I"),
            rec(0, n, 0, "3S", "AAA", b"at ref_len"), rec(0, n, 0, "", "", b"nothing"), rec(0, 3, 0, "2D2M", read_for(chrom, 3, cigar("2D2M")), b"D first"),
            rec(0, 5, 0, "1S1I2M", read_for(chrom, 5, cigar("1S1I2M")), b"S I")]
    cnt = emu_check(recs, [chrom], what="indels", site_kw=[dict(), dict(mask=0xE0)])
    assert cnt[(0, 4, px.INS)] == 1 and cnt[(0, 6, px.INS)] == 2 and cnt[(0, 0, px.INS)] == 1 and cnt[(0, n - 3, px.DEL)] == 1 and cnt[(0, n - 1, px.DEL)] == 2
    assert cnt[(0, 2, px.CLIP)] == 1 and cnt[(0, 9, px.CLIP)] == 1 and cnt[(0, 5, px.CLIP)] == 1 and cnt[(0, 5, px.INS)] == 1 and cnt[(0, 3, px.DEL)] == 1
    assert not any(p == 6 and ch == px.CLIP for (_, p, ch) in cnt)


def test_flags():
    """9. each bit of 0x704 alone is not counted, supplementary is; a custom mask"""
    chrom = b"ACGTACGTAC"
    flags = [0, 4, 0x100, 0x200, 0x400, 0x800, 16, 1, 0x704]
    recs = [rec(0, k, f, "1M", [15], b"f%d" % k) for k, f in enumerate(flags)]
    cnt = emu_check(recs, [chrom], what="default")
    assert sorted(p for (_, p, _ch) in cnt) == [0, 5, 6, 7]
    cnt = emu_check(recs, [chrom], exclude=0x810, what="custom")
    assert sorted(p for (_, p, _ch) in cnt) == [0, 1, 2, 3, 4, 7, 8]
    assert sorted(p for (_, p, _ch) in emu_check(recs, [chrom], exclude=0, what="none")) == list(range(9))


def test_regions():
    """10. events at beg - 1, beg, end - 1, end; an insertion whose anchor falls just outside; a chromosome without a region; an empty one"""
    chroms = [b"ACGTACGTACGTACGTACGTACGTACGT", b"ACGTACGT", b"TTTTTTTT", b""]
    regions = [(0, 10, 20), (2, 3, 3)]
    recs = [rec(0, p, 0, "1M", [15], b"m%d" % p) for p in (9, 10, 19, 20)]
    recs += [rec(0, 8, 0, "2M1I2M", read_for(chroms[0], 8, cigar("2M1I2M")), b"anchor 9"), rec(0, 9, 0, "2M1I2M", read_for(chroms[0], 9, cigar("2M1I2M")), b"anchor 10"),
             rec(0, 18, 0, "2M2D1M1S", read_for(chroms[0], 18, cigar("2M2D1M1S")), b"D at 20, S at 22"), rec(0, 17, 0, "2M2D", read_for(chroms[0], 17, cigar("2M2D")), b"D at 19"),
             rec(1, 0, 0, "8M", [15] * 8, b"no region"), rec(2, 0, 0, "8M", [1] * 8, b"empty region")]
    cnt = emu_check(recs, chroms, regions, what="regions")
    assert cnt == {(0, 10, px.N): 1, (0, 19, px.N): 1, (0, 10, px.INS): 1, (0, 19, px.DEL): 1}
    assert px.slots([len(c) for c in chroms], regions) == ([10, 0, 3, 0], [20, 0, 3, 0], [0, 10, 10, 10, 10])
    whole = emu_check(recs, chroms, None, what="whole")
    assert whole[(0, 9, px.INS)] == 1 and whole[(0, 20, px.DEL)] == 1 and whole[(0, 22, px.CLIP)] == 1 and whole[(1, 7, px.N)] == 1 and whole[(2, 0, px.A)] == 1
    emu_check(recs, chroms, [(0, 0, 28), (1, 8, 8), (3, 0, 0), (2, 7, 8)], what="one region each")


@pytest.mark.parametrize("ref_len,regions", [([5, -1], None), ([5, 5], [(2, 0, 1)]), ([5, 5], [(-1, 0, 1)]), ([5, 5], [(0, -1, 1)]), ([5, 5], [(0, 3, 2)]), ([5, 5], [(1, 0, 6)]),
                                              ([5, 5], [(0, 0, 1), (1, 0, 1), (0, 2, 3)])])
def test_create_refusals(ref_len, regions):
    with pytest.raises(px.Refused):
        px.slots(ref_len, regions)
    with pytest.raises(epl.CreateRefused) as e:
        epl.EmuPileup([b"A" * max(0, n) for n in ref_len], regions=regions, ref_len=ref_len)
    assert e.value.args[0] == BAD


def test_sites():
    """11. with the emulator's tile of 12: sites at base 0, at the tile seams and at a chromosome's last base; chromosomes of length 0 and 1;
    m = min_count - 1 and min_count; m * den == num * depth exactly and one short of it; depth 0; no depth; a mask of CLIP only"""
    rng = random.Random(4)
    chroms = [rand_chrom(rng, 2 * T + 5, odd=0), b"", b"G", rand_chrom(rng, 3 * T, odd=0), rand_chrom(rng, T + 1, odd=0)]
    recs = []
    for r, p, k in ((0, 0, 3), (0, T - 1, 1), (0, T, 2), (0, 2 * T + 4, 4), (2, 0, 2), (3, T - 1, 1), (3, 3 * T - 1, 5), (4, 0, 1), (4, T, 3), (3, 7, 6)):
        recs += [rec(r, p, 0, "1M", [15], b"x")] * k  # k mismatches at (r, p), channel N: the code 15 matches no byte
    recs += [rec(0, 5, 0, "2S2M", read_for(chroms[0], 5, cigar("2S2M")), b"clip")] * 2 + [rec(3, 20, 0, "1M1D1M", read_for(chroms[3], 20, cigar("1M1D1M")), b"del")] * 4
    depth = [np.full(len(c), 10, np.int32) for c in chroms]
    depth[3][7] = 30    # 6 * 5 == 1 * 30: exactly the fraction
    depth[3][3 * T - 1] = 26  # 5 * 5 == 25 < 26: one short
    depth[0][0] = 0     # a depth of 0 passes
    depth[3][21] = 21   # DEL: 4 * 5 = 20 < 21
    kws = [dict(mask=0xFF), dict(mask=0xFF, min_count=3), dict(mask=0xFF, min_count=4), dict(mask=0x80), dict(mask=0x10, min_count=2), dict(), dict(mask=0xFF, min_count=7)]
    cnt = emu_check(recs, chroms, what="sites", site_kw=kws)
    emu_check(recs, chroms, what="sites with depth", depth=depth, site_kw=[dict(mask=0xFF, num=1, den=5), dict(mask=0xFF, num=0, den=0), dict(mask=0x1F, num=3, den=10, min_count=2),
                                                                            dict(mask=0xFF, num=2 ** 32 - 1, den=2 ** 32 - 1)], geometries=((0, 1), (3, 2)))
    frac = px.sites(cnt, chroms, None, depth, 0xFF, 1, 1, 5)
    got = {(int(s["ref_id"]), int(s["pos"])) for s in frac}
    assert (3, 7) in got and (3, 3 * T - 1) not in got and (0, 0) in got and (3, 21) not in got and (0, 2 * T + 4) in got and (2, 0) in got
    assert int(frac[0]["depth"]) == 0 and frac[0]["ref_base"] == chroms[0][0]
    none = px.sites(cnt, chroms, mask=0xFF, min_count=7)
    assert len(none) == 0 and len(px.sites(cnt, chroms, mask=0x80)) == 1
    with Emu([]) as o:  # no chromosome at all
        assert o.add(*ix.concat([rec(-1, -1, 4)])) == (OK, 0, NO_RECORD, 0, 0) and o.sites()[0] == OK and len(o.sites()[1]) == 0 and o.array().shape == (0, 8)
    with Emu(chroms) as o:  # what plo_pileup_sites_dev refuses
        assert o.sites(min_count=0)[0] == BAD and o.sites(min_count=-3)[0] == BAD and o.sites(num=1, den=0)[0] == BAD and o.sites(num=0, den=0)[0] == OK
        assert o.sites(depth=depth, depth_state=0)[0] == BAD and o.sites(depth=depth, depth_state=2)[0] == BAD and o.sites(depth=depth, depth_state=1)[0] == OK


def test_contention():
    """12. 200 identical records mismatching at one base give a count of 200"""
    chrom = b"ACGTACGTACGTACGTACGTACGT"
    ops = cigar("1S5M1I2M1D3M")
    one = rec(0, 4, 0, ops, read_for(chrom, 4, ops, flips=[3]), b"same")
    cnt = emu_check([one] * 200, [chrom], what="contention", geometries=((0, 1), (1, 7)), site_kw=[dict(min_count=200), dict(min_count=201)])
    assert cnt[(0, 6, px.A)] == 200 and cnt[(0, 4, px.CLIP)] == 200 == cnt[(0, 8, px.INS)] == cnt[(0, 11, px.DEL)]


def test_order_and_splits():
    """13. the same records permuted, and split over several add calls with other wave counts, give an identical array; the summed
    n_events equals the array's sum"""
    rng = random.Random(17)
    chroms = [rand_chrom(rng, 300), rand_chrom(rng, 65), rand_chrom(rng, 150)]
    recs = [random_record(rng, chroms, k) for k in range(120)]
    cnt, n_counted, n_events = px.counts(recs, chroms)
    want = px.array(cnt, [len(c) for c in chroms])
    for k in range(3):
        order = list(recs)
        random.Random(k).shuffle(order)
        cuts = sorted(random.Random(40 + k).sample(range(len(order)), k * 2))
        pieces = [order[a:b] for a, b in zip([0] + cuts, cuts + [len(order)])]
        with Emu(chroms) as o:
            total = events = 0
            for j, piece in enumerate(pieces):
                st, nc, er, ek, ne = o.add(*ix.concat(piece), order_seed=j + k, n_waves=1 + (3 * j + k) % 5)
                assert (st, er, ek) == (OK, NO_RECORD, 0)
                total += nc
                events += ne
            assert total == n_counted and events == n_events == int(o.array().sum()) and np.array_equal(o.array(), want)
            assert o.reset() == OK and not o.array().any()


def test_numpy_restatement_agrees():
    """the record-at-a-time numpy form of the rule that tools/bench_records.py checks a whole window with gives counts()'s counts"""
    rng = random.Random(23)
    chroms = [rand_chrom(rng, 300), rand_chrom(rng, 90)]
    recs = [r for r in (random_record(rng, chroms, k) for k in range(150)) if r[36:40] != b"long"]
    for regions in (None, [(0, 50, 250)]):
        cnt, n_counted, n_events = px.counts(recs, chroms, regions)
        data, off = ix.concat(recs)
        keys, n, nc, ne, per = px.counts_numpy(np.frombuffer(data, np.uint8), off.astype(np.int64), chroms, regions)
        assert (nc, ne) == (n_counted, n_events) and {(int(k) >> 40, (int(k) >> 3) & ((1 << 37) - 1), int(k) & 7): int(x) for k, x in zip(keys, n)} == cnt
        assert per == [sum(x for (_, _, ch), x in cnt.items() if ch == c) for c in range(8)] and min(per) >= 1


REFUSAL_CHROMS = [rand_chrom(random.Random(70), 500), rand_chrom(random.Random(71), 300), rand_chrom(random.Random(72), 64)]


def refusals():
    """name -> (data, off, lowest offender, kind): inside a buffer of otherwise good records, behind the first wave's worth of them, and in
    front of a SECOND offender of another kind"""
    rng = random.Random(77)
    chroms = REFUSAL_CHROMS
    good = [random_record(rng, chroms, k) for k in range(130)]
    at, second = 70, 100

    def two(bad, later=None):
        recs = list(good)
        recs[at] = bad
        recs[second] = rec(0, 0, 0, "5M", "ACGTA", b"cut", n_cigar=9) if later is None else later
        return ix.concat(recs)

    lseq_bad = rec(1, 5, 0, "3M1I", "ACGTA", b"five bases")
    out = {}
    data, off = two(rec(0, 0, 0, "1M", "A"), lseq_bad)
    o = off.copy()
    o[at + 1] = o[at] - 1
    out["record_off decreases"] = (data, o, at, dx.ERR_OFFSET)
    out["shorter than 36 bytes"] = two(rec(0, 5)[:35]) + (at, dx.ERR_SHORT)
    out["block_size disagrees"] = two(rec(0, 5, 0, "4M", "ACGT", block_size=41)) + (at, dx.ERR_BLOCK)
    out["refID == n_ref"] = two(rec(len(chroms), 5)) + (at, dx.ERR_REFID)
    out["pos == -2"] = two(rec(0, -2)) + (at, dx.ERR_POS)
    out["the CIGAR one op past the record"] = two(rec(0, 5, 0, [ix.op(1, 0)] * 70, (), b"cut", n_cigar=71), lseq_bad) + (at, dx.ERR_CIGAR)
    out["a malformed field in front of CG"] = two(placeholder(0, 5, cigar("4M"), "ACGT", front=b"XAZno end", cg=False)) + (at, dx.ERR_AUX)
    out["CG leaves the record"] = two(placeholder(0, 5, cigar("4M2I4M"), "ACGTACGTAC", count=4)) + (at, dx.ERR_AUX)
    out["one base beyond ref_len"] = two(rec(1, 298, 0, "3M", "ACG", b"beyond"), lseq_bad) + (at, dx.ERR_END)
    out["the qualities leave the record"] = two(rec(0, 5, 0, "6M", "ACGTAC", b"short of one", cut=1), lseq_bad) + (at, px.ERR_SEQ)
    out["the bases leave the record, uncounted"] = two(rec(-1, -1, 4, "", (), b"l_seq lies", l_seq_says=40), lseq_bad) + (at, px.ERR_SEQ)
    out["l_seq of 2^32 - 1"] = two(rec(0, 5, 0, "2M", "AC", b"huge", l_seq_says=0xFFFFFFFF)) + (at, px.ERR_SEQ)
    out["one base more than the CIGAR reads"] = two(lseq_bad) + (at, px.ERR_LSEQ)
    out["one base fewer, through CG"] = two(placeholder(2, 10, cigar("2=1D2X1S"), "ACGT")) + (at, px.ERR_LSEQ)
    return out, chroms, good


def test_refusal_cases_cover_every_kind():
    cases, chroms, _ = refusals()
    assert {k for _, _, _, k in cases.values()} == set(range(1, 11))
    for name, (data, off, r, kind) in cases.items():
        assert px.first_offender(data, off, [len(c) for c in chroms]) == (r, kind), name


@pytest.mark.parametrize("name", sorted(refusals()[0]))
def test_refusal(name):
    """14. every kind as the lowest of two offenders; the array after a refused add equals the array before it, zero or not"""
    cases, chroms, good = refusals()
    data, off, r, kind = cases[name]
    for seed, n_waves in ((0, 1), (1, 4), (2, 7)):
        with Emu(chroms) as o:
            assert o.add(data, off, seed, n_waves) == (BAD, 0, r, kind, 0), name
            assert not o.array().any(), name
            assert o.add(*ix.concat(good), seed, n_waves)[0] == OK
            before = o.array()
            assert before.any()
            assert o.add(data, off, seed, n_waves) == (BAD, 0, r, kind, 0), name
            assert np.array_equal(o.array(), before), name


@pytest.mark.parametrize("seed", range(4))
def test_fuzz(seed):
    """15. seeded: 2 or 3 chromosomes of at most 300 bases, small random records valid by construction, against the restatement; with and
    without regions; a seed that leaves a channel without an event fails"""
    rng = random.Random(2000 + seed)
    chroms = [rand_chrom(rng, rng.randrange(40, 301)) for _ in range(2 + seed % 2)]
    recs = [random_record(rng, chroms, k, max_ops=rng.choice([6, 14])) for k in range(150)]
    exclude = rng.choice([px.EXCLUDE_DEFAULT, 0, 0x10])
    regions = None if seed < 2 else [(r, len(c) // 4, len(c) - len(c) // 5) for r, c in enumerate(chroms) if r != 1]
    dep, _ = dx.depths(recs, [len(c) for c in chroms], exclude)
    cnt = emu_check(recs, chroms, regions, exclude, what=seed, geometries=((seed, 1 + seed),), depth=[d.astype(np.int32) for d in dep],
                    site_kw=[dict(mask=0xFF), dict(num=1, den=5, min_count=2), dict(mask=0x0F, num=1, den=2)])
    per_channel = [sum(n for (_, _, ch), n in cnt.items() if ch == c) for c in range(8)]
    assert min(per_channel) >= 1, per_channel


def test_asan_program(tmp_path):
    """16. the same harness as a stand-alone program with ASan + UBSan, every array in a heap block of its exact size: hand vectors, op counts,
    the alignment catalogue, a CG record, fuzz cases with regions and depth, refusals"""
    cases, wants = [], []

    def case(recs, chroms, regions=None, pieces=1, depth=None, **kw):
        step = (len(recs) + pieces - 1) // pieces or 1
        adds = [ix.concat(recs[a:a + step]) + (len(cases) % 3, 1 + len(cases) % 4) for a in range(0, max(1, len(recs)), step)]
        cases.append(dict(chroms=chroms, regions=regions, adds=adds, depth=depth, **kw))
        wants.append((recs, chroms, regions, depth, kw, None))

    for v in GOLDEN["vectors"]:
        case(golden_records(v), golden_chroms(v), golden_regions(v), mask=0xFF)
    for n_ops in OP_COUNTS:
        case([rec(0, 3 + k, 0, seam_ops(n_ops, k), read_for(CHROM_SEAM, 3 + k, seam_ops(n_ops, k))) for k in range(3)], [CHROM_SEAM])
    rng = random.Random(31)
    chrom = rand_chrom(rng, 1100, odd=0.01)
    recs = []
    for start in range(16):
        for n in (1, 15, 16, 17, 33, 64 * 16 + 1):
            ops = [ix.op(start % 3, 4), ix.op(n, 0)]
            recs.append(rec(0, start, 0, ops, read_for(chrom, start, ops, flips=[start % 3, start % 3 + n - 1]), b"n" * (1 + start % 8)))
    case(recs, [chrom], pieces=2)
    real = [ix.op(1 + k % 2, (7, 8, 2, 1)[k % 4]) for k in range(300)]
    case([placeholder(0, 9, real, read_for(chrom, 9, real, flips=[0, 5])), placeholder(0, 2, cigar("3M"), "ACG", cg=False)], [chrom], mask=0xFF)
    chroms = [rand_chrom(rng, 290), rand_chrom(rng, 64), rand_chrom(rng, 131)]
    recs = [random_record(rng, chroms, k) for k in range(120)]
    dep = [d.astype(np.int32) for d in dx.depths(recs, [len(c) for c in chroms])[0]]
    case(recs, chroms, None, 3, dep, mask=0xFF, num=1, den=5)
    case(recs, chroms, [(0, 100, 290), (2, 0, 1)], 2, dep, min_count=2)
    ref_cases, ref_chroms, good = refusals()
    for name, (data, off, r, kind) in sorted(ref_cases.items()):
        cases.append(dict(chroms=ref_chroms, adds=[ix.concat(good) + (0, 3), (data, off, 1, 3)]))
        wants.append((good, ref_chroms, None, None, {}, (r, kind)))
    rc, err, res = epl.run_asan(cases, str(tmp_path))
    assert rc == 0, err[-3000:]
    assert "ERROR" not in err and "runtime error" not in err, err[-3000:]
    for got, (recs, chroms, regions, depth, kw, refused) in zip(res, wants):
        cnt, n_counted, n_events = px.counts(recs, chroms, regions)
        assert got["create"] == OK
        if refused:
            assert got["adds"][0][0] == OK and got["adds"][1] == (BAD,) + refused + (0, 0)
        else:
            assert all(a[0] == OK for a in got["adds"]) and sum(a[3] for a in got["adds"]) == n_counted and sum(a[4] for a in got["adds"]) == n_events
        assert np.array_equal(got["array"], px.array(cnt, [len(c) for c in chroms], regions))
        assert got["sites_status"] == OK and same(got["sites"], px.sites(cnt, chroms, regions, depth, **kw))


# ---- GPU ------------------------------------------------------------------------------------------------------------------------------------

def shipped_tile():
    return int(re.search(r"#define PLO_PILEUP_TILE (\d+)", open(os.path.join(HERE, "..", "portello_amd", "csrc", "pileup_core.hpp")).read()).group(1))


def index_for(chroms):
    """an index whose chrom_seq are these chromosomes (one contig with one segment on the first: the pileup reads nothing else of it)"""
    from portello_amd import cigar as cg

    return abi.IndexData(contig_len=np.array([1000]), contig_seg_off=np.array([0, 1], np.uint32), seg_chrom_index=np.array([0], np.uint32), seg_pos=np.array([0]),
                         seg_is_fwd_strand=np.array([1], np.uint8), seg_mapq=np.array([50], np.uint8), seg_seq_order_start=np.array([0]), seg_seq_order_end=np.array([1000]),
                         seg_cigar_off=np.array([0, 1], np.uint32), seg_cigar=np.array(list(cg.encode("1000M")), np.uint32),
                         chrom_seq=[np.frombuffer(c, np.uint8).copy() if len(c) else np.zeros(0, np.uint8) for c in chroms], rev_contig_seq=[None])


class Dev:
    """hand-made records through pileup.DevicePileup on one engine whose index holds `chroms`"""

    def __init__(self, chroms):
        import torch

        self.torch = torch
        self.dev = torch.device("cuda", 0)
        self.chroms = chroms
        self.index = api.Index(index_for(chroms), 0)
        self.eng = api.Engine(self.index)

    def upload(self, data, off):
        t = self.torch
        raw = t.from_numpy(np.frombuffer(data, np.uint8).copy()).to(self.dev) if len(data) else t.zeros(16, dtype=t.uint8, device=self.dev)
        offs = t.from_numpy(np.ascontiguousarray(off, np.uint64).view(np.int64)).to(self.dev)
        t.cuda.synchronize()
        return raw, offs

    def add(self, obj, recs, eng=None):
        data, off = ix.concat(recs)
        raw, offs = self.upload(data, off)
        return obj.add_dev(eng or self.eng, raw.data_ptr(), len(data), len(recs), offs.data_ptr())

    def depth_object(self, dep):
        """a FINISHED depth object that holds these depths: one record of 1M per unit of depth would do, here runs of equal depth as M ops"""
        from portello_amd import depth

        obj = depth.DeviceDepth(self.eng, [len(c) for c in self.chroms])
        recs = []
        for r, d in enumerate(dep):
            for level in range(1, int(d.max()) + 1 if len(d) else 0):
                on = np.flatnonzero(np.diff(np.concatenate([[0], (d >= level).astype(np.int8), [0]])))
                recs += [rec(r, int(a), 0, [ix.op(int(b - a), 0)], (), b"d") for a, b in zip(on[0::2], on[1::2])]
        if recs:
            data, off = ix.concat(recs)
            raw, offs = self.upload(data, off)
            obj.add(self.eng, raw.data_ptr(), len(data), len(recs), offs.data_ptr())
        obj.finish(self.eng)
        return obj

    def check(self, recs, regions=None, exclude=px.EXCLUDE_DEFAULT, pieces=1, depth=None, site_kw=None, what=""):
        chroms, ref_len = self.chroms, [len(c) for c in self.chroms]
        assert px.first_offender(*ix.concat(recs), ref_len, exclude) is None, what
        cnt, n_counted, n_events = px.counts(recs, chroms, regions, exclude)
        obj = pileup.DevicePileup(self.eng, ref_len, regions, exclude)
        info = obj.info()
        beg, end, off = px.slots(ref_len, regions)
        assert int(info.n_bases) == off[-1] and int(info.bytes_allocated) >= 32 * off[-1] and int(info.n_ref) == len(ref_len), what
        assert np.ctypeslib.as_array(info.slot_off, (len(ref_len) + 1,)).tolist() == off, what
        if ref_len:
            assert np.ctypeslib.as_array(info.slot_beg, (len(ref_len),)).tolist() == beg and np.ctypeslib.as_array(info.slot_end, (len(ref_len),)).tolist() == end, what
        assert C.cast(info.array, C.c_void_p).value % 32 == 0
        step = (len(recs) + pieces - 1) // pieces or 1
        total = events = 0
        for a in range(0, max(1, len(recs)), step):
            ao = self.add(obj, recs[a:a + step])
            assert (int(ao.err_record), int(ao.err_kind)) == (NO_RECORD, 0), what
            total += int(ao.n_counted)
            events += int(ao.n_events)
        got = obj.array()
        assert total == n_counted and events == n_events == int(got.sum()), what
        assert np.array_equal(got, px.array(cnt, ref_len, regions)), what
        dobj = self.depth_object(depth) if depth is not None else None
        for kw in (site_kw or [dict(), dict(mask=0xFF), dict(mask=0x80), dict(min_count=2)]):
            sites = obj.sites(dobj, kw.get("mask", px.MASK_DEFAULT), kw.get("min_count", 1), (kw.get("num", 0), kw.get("den", 1)))
            assert same(sites, px.sites(cnt, chroms, regions, depth, **kw)), (what, kw)
        if dobj is not None:
            dobj.close()
        obj.close()
        return cnt

    def close(self):
        self.eng.close()
        self.index.close()


@pytest.mark.gpu
def test_device_vectors():
    """17. the hand vectors through plo_pileup_add_dev and plo_pileup_sites_dev, an index per vector"""
    for v in GOLDEN["vectors"]:
        d = Dev(golden_chroms(v))
        assert d.check(golden_records(v), golden_regions(v), what=v["name"]) == golden_counts(v), v["name"]
        d.close()


@pytest.mark.gpu
def test_device_shapes():
    """18. the shape catalogue on the device, one index for all: op counts at the step seam, the CG record, M ops at every address mod 16,
    the second trip of pieces, names of 1 to 8 bytes, every code against every byte, indels and clips, flags, a fuzz case with depth"""
    rng = random.Random(44)
    col = b"ACGTNaZ\0"
    real = [ix.op(1, rng.choice([7, 7, 8, 2, 1])) for _ in range(65536)]
    chroms = [CHROM_SEAM, rand_chrom(rng, 64 * 16 + 60, odd=0.01), col + bytes(8) + col * 6 + b"MRWSYKVHDB=" + col, b"ACGTTGCAAC" * 3, rand_chrom(rng, ref_len_of(real) + 150, odd=0), b"", b"G"]
    d = Dev(chroms)
    for n_ops in OP_COUNTS:
        recs = []
        for kind in range(3):
            ops = seam_ops(n_ops, kind)
            n = read_len(ops)
            recs.append(rec(0, 3 + kind, 0, ops, read_for(chroms[0], 3 + kind, ops, flips=[k for k in (0, n // 2, n - 1) if n and ref_positions(3 + kind, ops)[k] is not None]), b"s%d" % kind))
        d.check(recs, what=n_ops, site_kw=[dict(mask=0xFF)])
    recs = []
    for start in range(16):
        for n in (1, 15, 16, 17, 33, 64 * 16 + 1):
            for odd in (0, 1):
                ops = ([ix.op(1, 4)] if odd else []) + [ix.op(n, 0)]
                flips = sorted({odd, odd + n - 1} | {odd + k for k in range(n) if (start + k) % 16 in (0, 15) and k < 40})
                recs.append(rec(1, start, 0, ops, read_for(chroms[1], start, ops, flips), b"a" * (1 + (start + n + odd) % 8)))
    recs.append(rec(1, len(chroms[1]) - 33, 0, "33M", read_for(chroms[1], len(chroms[1]) - 33, cigar("33M"), [0, 32]), b"end"))
    recs.append(rec(1, 20, 16, [ix.op(64 * 16 + 1, 8)], [15] * (64 * 16 + 1), b"every base"))
    d.check(recs, pieces=2, what="alignment", site_kw=[dict(), dict(mask=0x10, min_count=2)])
    recs = [rec(2, 0, 0, "8M", [c] * 8, b"c%d" % c) for c in range(16)] + [rec(2, 16, 0, [ix.op(67, 0)], [c] * 67, b"w%d" % c, bytes(c % 3)) for c in range(16)]
    d.check(recs, what="codes", site_kw=[dict(), dict(mask=0x10)])
    c3, n = chroms[3], len(chroms[3])
    recs = [rec(3, 4, 0, "2I3M", read_for(c3, 4, cigar("2I3M")), b"front"), rec(3, 4, 0, "3M2I3M", read_for(c3, 4, cigar("3M2I3M")), b"between"), rec(3, 4, 0, "3M2I", read_for(c3, 4, cigar("3M2I")), b"end"),
            rec(3, n - 5, 0, "2M3D", read_for(c3, n - 5, cigar("2M3D")), b"D last"), rec(3, n - 1, 0, "1D", "", b"D only"),
            rec(3, 2, 0, "2H3S2M4N1P2M0M0D0I0S3S1H", read_for(c3, 2, cigar("2H3S2M4N1P2M0M0D0I0S3S1H")), b"all"), rec(3, 6, 0, "4S2I", "ACGTAC", b"S and I"), rec(3, n, 0, "3S", "AAA", b"at ref_len"),
            rec(6, 0, 0, "1M", "T", b"one base"), rec(6, 0, 0, "1S1M1I", "ATC", b"one base 2")]
    recs += [rec(3, k, f, "1M", [15], b"f%d" % k) for k, f in enumerate([0, 4, 0x100, 0x200, 0x400, 0x800, 16, 1, 0x704])]
    d.check(recs, what="indels and flags", site_kw=[dict(mask=0xFF), dict(mask=0xE0)])
    d.check(recs, exclude=0x810, what="a custom mask", site_kw=[dict(mask=0xFF)])
    codes = read_for(chroms[4], 100, real, rng=rng)
    for k in range(0, len(codes), 97):
        codes[k] = 15
    d.check([rec(4, 3, 0, "5M", "TTTTT", b"short"), placeholder(4, 100, real, codes), placeholder(4, 20, cigar("4=2D4="), "ACGTACG", cg=False)], what="long", site_kw=[dict(mask=0xFF)])
    d.close()
    small = [chroms[0][:300], chroms[1][:200], chroms[3]]
    recs = [random_record(rng, small, k) for k in range(200)]
    d = Dev(small)
    dep = [x.astype(np.int32) for x in dx.depths(recs, [len(c) for c in small])[0]]
    cnt = d.check(recs, pieces=3, depth=dep, what="fuzz", site_kw=[dict(mask=0xFF), dict(num=1, den=5, min_count=2), dict(mask=0x0F, num=1, den=2)])
    assert min(sum(n_ for (_, _, ch), n_ in cnt.items() if ch == c) for c in range(8)) >= 1
    d.close()


@pytest.mark.gpu
def test_device_real_tile_and_sites():
    """19. one object over a chromosome of 1024 * 64 + 1 bases with sites at 0, 1023, 1024 and the last base: the shipped tile has a seam and
    the scan of the tiles' counts a second level; the thresholds of the site rule against a depth object; what the sites call refuses"""
    from portello_amd import depth

    tile = shipped_tile()
    n = tile * 64 + 1
    assert tile == 1024 and (n + tile - 1) // tile == 65
    rng = random.Random(6)
    chroms = [rand_chrom(rng, n, odd=0), rand_chrom(rng, 40, odd=0)]
    d = Dev(chroms)
    recs = []
    for p, k in ((0, 3), (tile - 1, 2), (tile, 2), (n - 1, 4), (5000, 6), (6000, 5)):
        recs += [rec(0, p, 0, "1M", [15], b"x")] * k
    recs += [rec(1, 39, 0, "1M", [15], b"y"), rec(0, 70, 0, "2S2M", read_for(chroms[0], 70, cigar("2S2M")), b"clip")]
    dep = [np.full(n, 10, np.int32), np.full(40, 2, np.int32)]
    dep[0][5000], dep[0][6000], dep[0][0] = 30, 26, 0
    cnt = d.check(recs, depth=dep, what="tile", site_kw=[dict(mask=0xFF), dict(mask=0xFF, num=1, den=5), dict(mask=0xFF, min_count=4), dict(mask=0x80), dict(mask=0xFF, min_count=7)])
    got = {(int(s["ref_id"]), int(s["pos"])) for s in px.sites(cnt, chroms, None, dep, 0xFF, 1, 1, 5)}
    assert {(0, 0), (0, tile - 1), (0, tile), (0, n - 1), (0, 5000), (1, 39)} <= got and (0, 6000) not in got
    obj = pileup.DevicePileup(d.eng, [n, 40])
    open_depth = depth.DeviceDepth(d.eng, [n, 40])
    other = depth.DeviceDepth(d.eng, [n, 41])
    other.finish(d.eng)
    for call, text in ((lambda: obj.sites(min_count=0), "min_count"), (lambda: obj.sites(min_frac=(1, 0)), "frac_den"), (lambda: obj.sites(open_depth), "not finished"),
                       (lambda: obj.sites(other), "another list")):
        with pytest.raises(api.PortelloError, match=text) as e:
            call()
        assert e.value.status == BAD
    assert len(obj.sites(min_frac=(0, 0))) == 0
    for o in (obj, open_depth, other):
        o.close()
    with pytest.raises(api.PortelloError, match="chromosomes") as e:  # the index has other chromosomes than the object
        o2 = pileup.DevicePileup(d.eng, [n, 41])
        d.add(o2, recs[:1])
    assert e.value.status == BAD
    o2.close()
    d.close()


@pytest.mark.gpu
def test_device_refusals_and_regions():
    """20. every refusal returns its status, err_record and err_kind, names the record, and adds nothing -- on a fresh context and on a used
    one; what plo_pileup_create refuses; regions"""
    cases, chroms, good = refusals()
    d = Dev(chroms)
    ref_len = [len(c) for c in chroms]
    fresh = pileup.DevicePileup(d.eng, ref_len)
    name0 = sorted(cases)[-1]
    raw, offs = d.upload(*cases[name0][:2])
    with pytest.raises(api.PortelloError) as e:  # the context's first call of any kind
        fresh.add_dev(d.eng, raw.data_ptr(), len(cases[name0][0]), len(cases[name0][1]) - 1, offs.data_ptr())
    assert (e.value.err_record, e.value.err_kind) == cases[name0][2:] and not fresh.array().any()
    obj = pileup.DevicePileup(d.eng, ref_len)
    d.add(obj, good)
    before = obj.array()
    assert before.any() and np.array_equal(before, px.array(px.counts(good, chroms)[0], ref_len))
    for name, (data, off, r, kind) in sorted(cases.items()):
        raw, offs = d.upload(data, off)
        for o, want in ((obj, before), (fresh, np.zeros_like(before))):
            with pytest.raises(api.PortelloError, match=r"record %d " % r) as e:
                o.add_dev(d.eng, raw.data_ptr(), len(data), len(off) - 1, offs.data_ptr())
            assert (e.value.status, e.value.err_record, e.value.err_kind) == (BAD, r, kind), name
            assert np.array_equal(o.array(), want), name
    obj.reset()
    assert not obj.array().any()
    d.add(obj, good)
    d.add(obj, good)
    assert np.array_equal(obj.array(), 2 * before)
    obj.close()
    fresh.close()
    for v in GOLDEN["refused"]:
        dv = Dev(golden_chroms(v))
        o2 = pileup.DevicePileup(dv.eng, [len(c) for c in golden_chroms(v)])
        with pytest.raises(api.PortelloError) as e:
            dv.add(o2, golden_records(v))
        assert (e.value.err_record, e.value.err_kind) == (v["err_record"], v["err_kind"]) and not o2.array().any()
        o2.close()
        dv.close()
    for rl, regions in (([5, -1], None), (ref_len, [(3, 0, 1)]), (ref_len, [(0, -1, 1)]), (ref_len, [(0, 3, 2)]), (ref_len, [(2, 0, 65)]), (ref_len, [(0, 0, 1), (0, 2, 3)])):
        with pytest.raises(api.PortelloError) as e:
            pileup.DevicePileup(d.eng, rl, regions)
        assert e.value.status == BAD
    empty = pileup.DevicePileup(d.eng, [])
    assert int(empty.info().n_bases) == 0 and empty.array().shape == (0, 8)
    empty.close()
    d.check(good, [(0, 100, 400), (2, 64, 64)], what="regions", pieces=2)
    d.check(good, [(1, 299, 300), (0, 0, 500), (2, 0, 1)], what="regions 2")
    d.close()


@pytest.mark.gpu
def test_device_contention():
    """21. 200 identical records: every counter they touch reads 200"""
    chrom = b"ACGTACGTACGTACGTACGTACGT"
    d = Dev([chrom])
    ops = cigar("1S5M1I2M1D3M")
    cnt = d.check([rec(0, 4, 0, ops, read_for(chrom, 4, ops, flips=[3]), b"same")] * 200, what="contention", site_kw=[dict(min_count=200), dict(min_count=201)])
    assert sorted(cnt.values()) == [200] * 4
    d.close()


@pytest.mark.gpu
def test_two_engines_add_at_once():
    """22. two engines on two Python threads add disjoint halves of a record set into one object at the same time"""
    rng = random.Random(8)
    chroms = [rand_chrom(rng, 30_000), rand_chrom(rng, 700), rand_chrom(rng, 64)]
    d = Dev(chroms)
    eng2 = api.Engine(d.index)
    recs = [random_record(rng, chroms, k, max_ops=14) for k in range(600)]
    cnt, n_counted, n_events = px.counts(recs, chroms)
    obj = pileup.DevicePileup(d.eng, [len(c) for c in chroms])
    halves = [recs[:300], recs[300:]]
    ups = [[d.upload(*ix.concat(h[a:a + 50])) + (len(ix.concat(h[a:a + 50])[0]),) for a in range(0, 300, 50)] for h in halves]
    counted, events, errors = [0, 0], [0, 0], []
    gate = threading.Barrier(2)

    def work(k, eng):
        try:
            gate.wait()
            for raw, offs, nb in ups[k]:
                ao = obj.add_dev(eng, raw.data_ptr(), nb, offs.numel() - 1, offs.data_ptr())
                counted[k] += int(ao.n_counted)
                events[k] += int(ao.n_events)
        except BaseException as e:  # noqa: BLE001
            errors.append(repr(e))

    ts = [threading.Thread(target=work, args=(k, e)) for k, e in enumerate((d.eng, eng2))]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors and sum(counted) == n_counted and sum(events) == n_events
    assert np.array_equal(obj.array(eng2), px.array(cnt, [len(c) for c in chroms]))
    obj.close()
    eng2.close()
    d.close()


@pytest.fixture(scope="module")
def small_bam(tmp_path_factory):
    from portello_amd import bamsynth, synth

    d = tmp_path_factory.mktemp("pileupdev")
    w = synth.generate(synth.config("tiny", n_reads=300, seed=412, split_read_frac=0.3, sorted_reads=True))
    path = str(d / "reads.bam")
    meta = bamsynth.write_read_bam(w, path, level=6, n_unmapped=4)
    return w, path, meta


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [dict(), dict(sorted_runs=True, emit_eqx=True)], ids=["plain", "sorted_runs+eqx"])
def test_bam_to_bam_pileup_out(small_bam, tmp_path, extra):
    """23. run_bam_to_bam(pileup_out=...): the TSV is the restatement's over the records read back from the written BAM, and the BAM is byte
    for byte the one of a run without pileup_out"""
    import bamcheck
    from portello_amd import bamsynth, pipeline

    w, path, meta = small_bam
    ixd = w.index_data()
    index = api.Index(ixd, 0)
    cn, rn = meta["contig_names"], bamsynth.ref_names(w)
    chroms = [bytes(np.asarray(s, np.uint8)) for s in ixd.chrom_seq]
    lens = [len(c) for c in chroms]
    kw = dict(window_reads=90, ramp=False, n_workers=2 if extra else 1, io_threads=4, device_records=True, device_batch=True, **extra)
    (tmp_path / "off").mkdir()
    (tmp_path / "on").mkdir()
    st0 = pipeline.run_bam_to_bam(path, str(tmp_path / "off" / "lifted.bam"), index, ixd, cn, rn, lens, **kw)
    regions = [(0, lens[0] // 10, lens[0])] if extra else None
    st = pipeline.run_bam_to_bam(path, str(tmp_path / "on" / "lifted.bam"), index, ixd, cn, rn, lens, pileup_out=str(tmp_path / "on" / "pile"), pileup_min_count=1 if extra else 2,
                                 pileup_min_frac=(1, 5), pileup_regions=regions, **kw)
    assert not st.errors and not st0.errors
    assert st0.pileup_paths == [] and st0.pileup_device_ms == 0 and sorted(os.listdir(str(tmp_path / "off"))) == sorted(map(os.path.basename, st0.out_paths))
    assert st.pileup_paths == [str(tmp_path / "on" / "pile.sites.tsv")] and st.pileup_device_ms > 0 and st.lift_detail_s.get("pileup", 0) > 0 and st.depth_paths == []
    assert [os.path.basename(p) for p in st.out_paths] == [os.path.basename(p) for p in st0.out_paths] and st.records_out == st0.records_out
    recs = []
    for p0, p in zip(st0.out_paths, st.out_paths):
        assert open(p, "rb").read() == open(p0, "rb").read()
        recs += bamcheck.read_bam(p)[2]
    assert len(recs) == st.records_out > 300 and px.first_offender(*ix.concat(recs), lens) is None
    cnt, n_counted, n_events = px.counts(recs, chroms, regions)
    dep, _ = dx.depths(recs, lens)
    want = px.sites(cnt, chroms, regions, dep, px.MASK_DEFAULT, 1 if extra else 2, 1, 5)
    assert n_counted > 250 and open(st.pileup_paths[0]).read() == px.sites_text(rn, want)
    assert n_events > 0  # (whether the synthetic reads differ from the reference at all is the generator's: the text above is compared either way)
    index.close()
