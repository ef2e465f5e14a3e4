"""The device's DEFLATE decoder (portello_amd/csrc/inflate.hpp) on streams built by hand (tests/deflate_craft.py): what RFC 1951 allows and
no encoder at hand emits -- 15-bit codes, length 258 as symbol 284 + 31, single-code distance sets, 7-bit code-length codes, hundreds of
empty blocks -- matches placed on the decoder's own edges (the 4 KiB write-back unit of the 8 KiB ring, INF_NEAR = 7680, stored runs that
bypass the ring), and what it must refuse.  ONE catalogue serves every leg:

  * the reference is zlib: zlib.decompressobj(-15) run here, "accept" only if it reaches the end of the stream and the bytes fit;
  * the table's verdict must be zlib's (that catches mistakes of the builder), and where zlib accepts, its bytes are what the builder meant;
  * the emulator, serial and as a 64-lane wave, agrees with zlib on the verdict and, on accept, on the bytes; a refusal writes nothing
    outside its buffer;
  * a differential test over damaged zlib streams asks the same: our verdict is zlib's, whatever the damage did;
  * the stand-alone AddressSanitizer + UBSan program (tests/emu/emu_inflate.cpp) decodes all of it from heap blocks of the exact sizes;
  * GPU: the accepted streams as BGZF blocks through plo_bgzf_inflate_dev in one call, and one refused stream per status of inflate.hpp in
    a call of its own.  The device lists are slices of the catalogue: nothing reaches the GPU that the wave emulator has not decoded."""
import functools
import time
import zlib
from collections import namedtuple

import numpy as np
import pytest

import deflate_craft as dc
import emu_inflate_lib as eil
from deflate_craft import EOB, Stream, lit, lits, match
from test_inflate import _big_payloads

Entry = namedtuple("Entry", "name stream cap accept expected dev")
ACCEPT, REJECT = True, False
RNG = np.random.default_rng(1951)
FILL = RNG.integers(0, 256, 70000, dtype=np.uint8).tobytes()
NEAR = 7680  # INF_NEAR of inflate.hpp: the largest distance served from the 8 KiB ring, which is written back in halves of 4096


def zlib_verdict(stream: bytes, cap: int):
    """(accept, bytes): accept only if zlib reaches the end of the stream and its output fits into cap -- an error, a stream that ends early
    and an output that is too large are all refusals"""
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(stream, cap + 1)
    except zlib.error:
        return False, b""
    if len(out) > cap or not d.eof:
        return False, b""
    return True, out


# ---- the catalogue -------------------------------------------------------------------------------------------------------------------------
def _chain(symbols):
    """the chain code 1, 2, ..., 14, 15, 15 over 16 symbols, in the order given: a complete code whose last six are beyond the fast table"""
    assert len(symbols) == 16
    return dict(zip(symbols, list(range(1, 16)) + [15]))


CHAIN_LL = _chain([ord("e"), ord("t"), ord("a"), ord("o"), ord("n"), 257, ord("i"), ord("s"), 258, 270, ord("h"), ord("r"), 284, 0, 285, 256])
CHAIN_D = _chain([0, 1, 2, 3, 4, 8, 10, 12, 16, 20, 22, 24, 26, 27, 28, 29])
LONG_LITS = bytes(range(65, 83))  # 18 literals with codes of 11 .. 15 bits
LONG_LL = dc.lengths_of(266, {**{257 + k: 1 + k for k in range(9)}, **dict(zip(LONG_LITS, [11] + [12] * 2 + [13] * 4 + [14] * 4 + [15] * 7)), 256: 15})


def _chain_litlen():
    toks = lits(b"tea on the shore is")  # (bytes without a code are left out below)
    toks = [t for t in toks if t[1] in CHAIN_LL] + [lit(0), match(3, 1), lit(ord("h")), match(4, 2), match(25, 3), match(258, 4), lit(ord("r")),
                                                     match(258, 1, alt258=True), match(227, 2), lit(ord("s")), match(258, 3)]
    return Stream().dynamic(dc.lengths_of(286, CHAIN_LL), [2, 2, 2, 2], toks + [EOB], True)


def _chain_dist():
    s = Stream().stored(FILL[:33000], False)
    toks = [match(258, 32768), match(258, 1), match(258, 24577)]
    for d in CHAIN_D:
        toks += [match(3, dc.DIST_BASE[d]), match(4, dc.DIST_BASE[d] + (1 << dc.DIST_EXTRA[d]) - 1)]
    return s.dynamic(dc.lengths_of(286, {256: 1, 285: 2, 257: 3, 258: 3}), dc.lengths_of(30, CHAIN_D), toks + [EOB], True)


def _long_literals(n=9000):
    data = bytes(RNG.choice(np.frombuffer(LONG_LITS, np.uint8), n))
    return Stream().dynamic(LONG_LL, [0], lits(data) + [EOB], True, cl_sequence=dc.rle_sequence(LONG_LL + [0]))


def _boundary(bounds, length, place, far):
    """a fixed block of literals with one match per boundary B: starting just before it, ending exactly at it, or crossing it in the middle"""
    toks, pos = [], 0
    for B in bounds:
        start = {"start": B - 1, "end": B - length, "cross": B - length // 2}[place]
        assert start > pos
        _fill(toks, pos, start)
        toks.append(match(length, start if far else 1))
        pos = start + length
    return Stream().fixed(toks + lits(b"tail") + [EOB], True)


def _fill(toks, pos, target):
    """tokens for the bytes [pos, target) in front of a match under test: 600 literals to begin with, then long matches at changing
    distances -- one symbol per 258 bytes, and the emulated wave pays per symbol, not per byte -- and literals again for the last 40 bytes,
    so that a literal run leads up to the match"""
    k = 0
    while pos < target:
        if pos < 600:
            n = min(600, target) - pos
            toks += lits(FILL[pos:pos + n])
        elif target - pos > 43:
            n = min(258, target - 40 - pos)
            toks.append(match(n, (211, 257, 563, 299, 300)[k % 5]))
            k += 1
        else:
            n = target - pos
            toks += lits(FILL[pos:target])
        pos += n


def _behind_9000(dist):
    toks = lits(FILL[:9000]) + [match(258, dist), lit(1), lit(2), lit(3), match(3, dist), lit(4), match(65, dist), lit(5), EOB]
    return Stream().fixed(toks, True)


def _stored_mid(n_before):
    """n_before Huffman-coded bytes, a stored run of 300, then matches out of the run, across its end into the ring, and across the whole of it"""
    s = Stream()
    if n_before:
        s.fixed(lits(FILL[:n_before]) + [EOB], False)
    s.stored(FILL[20000:20300], False)
    end = n_before + 300
    toks = lits(b"twenty literals, yes")              # pos = end + 20
    toks.append(match(40, 40))                         # source: 20 bytes of the run, 20 of the ring
    toks.append(match(100, 60 + 50))                   # starts inside the run, overlaps nothing            (pos = end + 60)
    toks.append(match(258, 160 + 100))                 # the run's last 100 bytes and on through the ring   (pos = end + 160)
    pos = end + 418
    toks.append(match(258, pos - max(0, n_before - 5)))  # from in front of the run (where there is a front) across it
    pos += 258
    toks.append(match(30, pos - end + 10))             # the run's last ten bytes, then the ring
    toks += lits(b"end")
    return s.fixed(toks + [EOB], True)


def _overlap_across(bound, dist):
    """Huffman-coded bytes, a stored run of 90 that ends six bytes in front of `bound`, and at once a match of 258 at `dist` <= 90: it
    overlaps itself, all of its source lies in the run, and it crosses the boundary"""
    toks = []
    _fill(toks, 0, bound - 96)
    s = Stream().fixed(toks + [EOB], False).stored(FILL[30000:30090], False)
    assert len(s.expected) == bound - 6
    return s.fixed([match(258, dist), lit(9), match(64, dist + 1), EOB], True)


def _stream_end(a):
    """a fixed block that ends on the last bit of its last byte: 3 + 8 a + 9 * 6 + 7 bits, 8 + a bytes"""
    s = Stream().fixed(lits(b"A" * a + bytes([200] * 6)) + [EOB], True)
    assert s.w.bit_length() == 8 * (8 + a) and len(s.getvalue()) % 4 == a % 4
    return s


def _chain_end():
    """a dynamic block whose 15-bit end-of-block code ends on the last bit of the stream (the one-bit literal pads)"""
    for k in range(8):
        s = Stream().dynamic(dc.lengths_of(286, CHAIN_LL), [1], lits(b"e" * k + b"shore") + [match(4, 1), EOB], True)
        if s.w.bit_length() % 8 == 0:
            return s
    raise AssertionError


CL_REP = dc.lengths_of(19, {1: 2, 2: 2, 3: 3, 16: 3, 18: 2})


def _zeros_then(sym_lengths, n):
    """a cl_sequence for `n` lengths that are zero but for {position: length}: runs of 18 / 17 and plain zeros"""
    return dc.rle_sequence(dc.lengths_of(n, sym_lengths), use16=False, use17=False)


def _catalogue():
    E = []

    def acc(name, s, dev=True, room=0):
        E.append(Entry(name, s.getvalue(), len(s.expected) + room, ACCEPT, bytes(s.expected), dev))

    def rej(name, s, cap=1000, dev=False):
        stream = s if isinstance(s, bytes) else s.getvalue()
        E.append(Entry(name, stream, cap, REJECT, b"", dev))

    # long codes
    acc("chain_litlen", _chain_litlen())
    acc("chain_dist_behind_stored", _chain_dist())
    acc("long_literals_9000", _long_literals())
    # length 258 the other way, in the fast tables and beyond them (chain_litlen)
    acc("alt258_fixed", Stream().fixed(lits(b"abc") + [match(258, 3, alt258=True), match(258, 1), match(258, 261, alt258=True), EOB], True))
    # distance bounds
    acc("dist_eq_pos", Stream().fixed(lits(b"hello") + [match(3, 5), match(8, 8), EOB], True))
    rej("dist_eq_pos_plus_1", Stream().fixed(lits(b"hello") + [match(3, 6), EOB], True), dev=True)  # -7
    rej("dist_beyond_output", Stream().fixed(lits(FILL[:100]) + [match(10, 32768), EOB], True))
    rej("match_at_pos_0", Stream().fixed([match(3, 1), EOB], True))
    # minimal and odd tables
    only_eob = dc.lengths_of(257, {256: 1})
    acc("only_eob_no_dist", Stream().dynamic(only_eob, [0], [EOB], True))
    acc("stored_then_only_eob", Stream().stored(b"hello, world", False).dynamic(only_eob, [0], [EOB], True))
    ab = dc.lengths_of(258, {ord("a"): 2, ord("b"): 2, 256: 2, 257: 2})
    acc("single_dist_sym0", Stream().dynamic(ab, [1], lits(b"ab") + [match(3, 1), lit(ord("a")), match(3, 1), EOB], True))
    acc("single_dist_sym1", Stream().dynamic(ab, [0, 1], lits(b"ab") + [match(3, 2), lit(ord("a")), match(3, 2), EOB], True))
    two = dc.lengths_of(257, {ord("a"): 1, 256: 1})
    acc("cl_code_of_3_symbols", Stream().dynamic(two, [0], lits(b"aaaa") + [EOB], True, cl_lengths=dc.lengths_of(19, {0: 2, 1: 2, 18: 1}),
                                                 cl_sequence=_zeros_then({ord("a"): 1, 256: 1}, 258)))
    ll7 = dc.lengths_of(286, {**{32 + k: 5 + k // 16 for k in range(80)}, **{112 + k: 10 for k in range(29)}, 256: 10, 257: 10, 285: 10})
    text7 = bytes(RNG.integers(32, 141, 500, dtype=np.uint8))
    cl7 = dc.lengths_of(19, {18: 2, 0: 2, 8: 2, 7: 3, 9: 4, 6: 5, 1: 6, 5: 7, 10: 7})
    acc("cl_codes_of_7_bits", Stream().dynamic(ll7, [1, 1], lits(text7[:250]) + [match(3, 1), match(258, 2)] + lits(text7[250:]) + [EOB], True,
                                               cl_lengths=cl7, cl_sequence=dc.rle_sequence(ll7, use16=False, use17=False) + [1, 1]))
    abz = {ord("a"): 1, 256: 3, 257: 3, 258: 2}  # (the last length of the literal/length set is the one that is repeated)
    acc("repeat_from_litlen_into_dist", Stream().dynamic(dc.lengths_of(259, abz), [2, 2, 2, 2], lits(b"aaaa") + [match(4, 2), match(3, 4), match(4, 3), match(3, 1), EOB], True,
                                                         cl_lengths=CL_REP, cl_sequence=_zeros_then(abz, 259) + [(16, 1)]))
    # many small blocks
    s = Stream()
    for _ in range(300):
        s.stored(b"", False)
    acc("300_empty_stored", s.stored(FILL[:500], True))
    s = Stream()
    for _ in range(700):
        s.fixed([EOB], False)
    acc("700_empty_fixed", s.fixed(lits(FILL[:500]) + [match(100, 250), EOB], True))
    acc("stored_65535", Stream().stored(FILL[:65535], True), dev=False)  # (a BGZF block holds 65510 bytes of deflate data at most)
    # the write-back boundaries of the ring
    for bounds in ((4095, 8191, 12288), (4096, 8192), (4097, 8193)):
        for length in (3, 64, 65, 258):
            for place in ("start", "end", "cross") if length > 3 else ("start", "end"):
                for far in (False, True):
                    acc(f"boundary_{bounds[0]}_len{length}_{place}_{'start' if far else 'dist1'}", _boundary(bounds, length, place, far))
    # near and far matches
    for d in (NEAR - 1, NEAR, NEAR + 1, NEAR + 254, NEAR + 255, 8191, 8192, 8193, 8450):
        acc(f"dist_{d}_behind_9000", _behind_9000(d))
    # a stored run in the middle
    for n in (0, 5, 4090, 5000):
        acc(f"stored_run_behind_{n}", _stored_mid(n))
    # an overlapping match (dist < len) whose source is a stored run: the bytes repeat a source that never was in the ring, so every one of
    # them comes from global memory (the far branch's own k % dist); at once behind the run, and across a write-back boundary
    acc("overlap_out_of_stored_3", Stream().stored(b"abc", False).fixed([match(258, 1), match(100, 3), EOB], True))
    acc("overlap_out_of_stored_behind_literals", Stream().fixed(lits(b"hello") + [EOB], False).stored(b"xyz", False).fixed([match(200, 2), lit(7), match(258, 3), EOB], True))
    for bound in (4096, 8192):
        for dist in (1, 2, 7, 90):
            acc(f"overlap_out_of_stored_across_{bound}_dist{dist}", _overlap_across(bound, dist))
    # stream ends
    ends = [(f"end_on_last_bit_len_mod4_{a}", _stream_end(a)) for a in range(4)] + [("end_on_last_bit_15_bit_eob", _chain_end())]
    ends.append(("end_with_padding_bits", Stream().fixed(lits(b"padding") + [EOB], True)))
    for name, s in ends:
        acc(name, s)
        rej(name + "_cut_by_a_byte", s.getvalue()[:-1], cap=len(s.expected), dev=name.endswith("mod4_0"))  # -1
    # zlib's own streams of block-sized payloads
    for k, data in enumerate(_big_payloads()):
        for level in (0, 1, 6, 9):
            c = zlib.compressobj(level, zlib.DEFLATED, -15)
            E.append(Entry(f"zlib_payload{k}_level{level}", c.compress(data) + c.flush(), len(data), ACCEPT, data, True))

    # ---- refused ----
    rej("litlen_286_fixed", Stream().fixed(lits(b"abc") + [dc.raw_ll(286), lit(0), lit(0), EOB], True), dev=True)  # -8
    rej("dist_30_fixed", Stream().fixed(lits(b"abc") + [dc.raw_ll(257), dc.raw_dist(30), lit(0), lit(0), EOB], True))
    rej("match_without_dist_codes", Stream().dynamic(ab, [0], lits(b"ab") + [dc.raw_ll(257), dc.code_bits(0, 1)] + lits(b"abababab") + [EOB], True), dev=True)  # -6
    rej("unused_code_of_single_dist_set", Stream().dynamic(ab, [1], lits(b"ab") + [dc.raw_ll(257), dc.code_bits(1, 1)] + lits(b"abababab") + [EOB], True))
    rej("unused_code_of_single_litlen_set", Stream().dynamic(only_eob, [0], [dc.code_bits(1, 1), dc.code_bits(0, 16), EOB], True))
    rej("litlen_oversubscribed", Stream().dynamic(dc.lengths_of(257, {0: 1, 1: 1, 256: 1}), [1], [EOB], True), dev=True)  # -5
    rej("dist_oversubscribed", Stream().dynamic(ab, [1, 1, 1], [EOB], True))
    rej("litlen_two_2_bit_codes", Stream().dynamic(dc.lengths_of(257, {0: 2, 256: 2}), [1], [EOB], True))
    rej("litlen_lone_2_bit_code", Stream().dynamic(dc.lengths_of(257, {256: 2}), [1], [EOB], True))
    rej("dist_two_2_bit_codes", Stream().dynamic(ab, [2, 2], lits(b"ab") + [EOB], True))
    rej("dist_lone_2_bit_code", Stream().dynamic(ab, [2], lits(b"ab") + [EOB], True))
    rej("no_end_of_block_code", Stream().dynamic(dc.lengths_of(257, {0: 1, 1: 1}), [1], [lit(0), lit(1), lit(0)], True))
    rej("header_16_first", Stream().dynamic(two, [0], [EOB], True, cl_lengths=dc.lengths_of(19, {0: 2, 1: 2, 16: 2, 18: 2}),
                                            cl_sequence=[(16, 0)] + _zeros_then({ord("a"): 1, 256: 1}, 258)[1:]))
    rej("header_repeat_overruns", Stream().dynamic(two, [0], [EOB], True, cl_lengths=dc.lengths_of(19, {0: 2, 1: 2, 18: 1}),
                                                   cl_sequence=_zeros_then({ord("a"): 1, 256: 1}, 257) + [(18, 0)]))
    rej("header_16_overruns", Stream().dynamic(dc.lengths_of(259, abz), [2, 2, 2, 2], lits(b"aa") + [EOB], True,
                                               cl_lengths=CL_REP, cl_sequence=_zeros_then(abz, 259) + [(16, 2)]))
    rej("header_hlit_30", Stream().dynamic(dc.lengths_of(287, {ord("a"): 1, 256: 1}), [0], [EOB], True, hlit=30))
    rej("header_hdist_31", Stream().dynamic(two, [1] + [0] * 31, [EOB], True, hdist=31))
    rej("cl_code_incomplete", Stream().dynamic(two, [0], [EOB], True, cl_lengths=dc.lengths_of(19, {0: 2, 1: 2, 18: 2})))
    rej("cl_code_all_zero", Stream().dynamic(two, [0], [EOB], True, cl_lengths=[0] * 19, cl_sequence=[]).stored(bytes(64), True))
    rej("stored_nlen_mismatch", Stream().stored(b"stored bytes", True, nlen=0x1234), dev=True)  # -4
    rej("stored_nlen_equals_len", Stream().stored(b"stored bytes", True, nlen=12))
    rej("block_type_3", Stream().fixed(lits(b"abc") + [EOB], False).block_type(3, True).stored(bytes(8), True), dev=True)  # -3
    rej("stored_len_past_the_input", Stream().stored(b"short", True, length=6))
    rej("stored_header_cut", Stream().fixed(lits(b"abc") + [EOB], False).stored(b"xy", True).getvalue()[:-3])
    rej("no_final_block", Stream().fixed(lits(b"abc") + [EOB], False).stored(b"more", False))
    rej("no_final_block_long", Stream().fixed(lits(FILL[:3000]) + [EOB], False))
    # an output one byte too small: for a literal, a match and a stored run; in the lane-parallel run and behind long codes
    rej("cap_short_by_a_literal", Stream().fixed(lits(FILL[:200]) + [EOB], True), cap=199, dev=True)  # -2
    rej("cap_short_by_a_match", Stream().fixed(lits(FILL[:200]) + [match(50, 7), EOB], True), cap=249)
    rej("cap_short_by_a_stored_run", Stream().fixed(lits(FILL[:200]) + [EOB], False).stored(FILL[:50], True), cap=249)
    rej("cap_short_by_a_long_literal", _long_literals(300), cap=299)
    rej("cap_short_by_a_long_code_match", _chain_litlen(), cap=len(_chain_litlen().expected) - 1)
    rej("cap_0", Stream().fixed(lits(b"a") + [EOB], True), cap=0)
    # what a BGZF block whose ISIZE is off by one asks of the decoder (ISIZE is its capacity; the kernel refuses a stream that ends early)
    far = _behind_9000(8193)
    rej(ISIZE_SHORT, far, cap=len(far.expected) - 1)
    acc(ISIZE_LONG, far, dev=False, room=1)
    assert len({e.name for e in E}) == len(E)
    return E


ISIZE_SHORT, ISIZE_LONG = "far_match_cap_one_short", "far_match_cap_one_long"
CATALOGUE = _catalogue()
BY_NAME = {e.name: e for e in CATALOGUE}


@functools.lru_cache(maxsize=None)
def emu(name: str, wave: bool):
    e = BY_NAME[name]
    return eil.inflate(e.stream, e.cap, wave=wave)


def test_catalogue_covers_what_it_claims():
    """what the names promise, checked on the streams themselves"""
    assert max(len(e.stream) for e in CATALOGUE) <= 65536 + 5 and max(e.cap for e in CATALOGUE) <= 65535
    assert sum(e.accept for e in CATALOGUE) > 100 and sum(not e.accept for e in CATALOGUE) > 35
    assert [e.name for e in CATALOGUE if e.accept and not e.dev] == ["stored_65535", ISIZE_LONG]
    assert {len(BY_NAME[f"end_on_last_bit_len_mod4_{a}"].stream) % 4 for a in range(4)} == {0, 1, 2, 3}
    assert len(set(BY_NAME["long_literals_9000"].expected)) == 18 and min(l for l in LONG_LL[:256] if l) == 11


@pytest.mark.parametrize("name", [e.name for e in CATALOGUE])
def test_catalogue_against_zlib(name):
    e = BY_NAME[name]
    ok, ref = zlib_verdict(e.stream, e.cap)
    assert ok == e.accept, "the table's verdict is not zlib's: the builder made another stream than it meant"
    if ok:
        assert ref == e.expected and len(ref) == e.cap - (e.name == ISIZE_LONG)
    for wave in (False, True):
        rc, out = emu(name, wave)
        assert (rc == 0) == ok, (name, wave, rc)
        assert -8 <= rc <= 0
        if ok:
            assert out == ref, (name, wave)
    assert emu(name, False)[0] == emu(name, True)[0]


def test_every_status_has_a_refused_stream():
    seen = {emu(e.name, True)[0] for e in CATALOGUE if not e.accept}
    assert seen == set(range(-8, 0))
    assert sorted(emu(e.name, True)[0] for e in DEV_REJECTED) == list(range(-8, 0))


# ---- damaged zlib streams: our verdict is zlib's ------------------------------------------------------------------------------------------
N_DAMAGED, N_DAMAGED_WAVE = 600, 100


@functools.lru_cache(maxsize=None)
def damaged_streams():
    """(stream, cap, wave) * N_DAMAGED: zlib streams of four small payloads at levels 1 / 6 / 9, Z_FIXED and Z_HUFFMAN_ONLY with one bit flipped,
    half of the flips in the first 100 bytes (where the tables are), every fifth stream with a byte overwritten as well"""
    rng = np.random.default_rng(2598)
    q = bytes(rng.integers(33, 74, 1500, dtype=np.uint8))
    payloads = [b"ACGT" * 300 + b"N" * 200 + bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 800)), q + q[::-1][:700] + q[:300],
                (b"@read/%d/ccs\tACGTTGCA\tRG:Z:x\tnp:i:12\n" * 40) + bytes(rng.integers(0, 256, 400, dtype=np.uint8)), bytes(rng.integers(0, 6, 2500, dtype=np.uint8))]
    base = []
    for data in payloads:
        for level, strategy in ((1, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_DEFAULT_STRATEGY), (9, zlib.Z_DEFAULT_STRATEGY), (6, zlib.Z_FIXED), (6, zlib.Z_HUFFMAN_ONLY)):
            c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
            base.append((c.compress(data) + c.flush(), len(data)))
    out = []
    for k in range(N_DAMAGED):
        comp, cap = base[k % len(base)]
        b = bytearray(comp)
        i = int(rng.integers(0, min(100, len(b)))) if k % 2 else int(rng.integers(0, len(b)))
        b[i] ^= 1 << int(rng.integers(0, 8))
        if k % 5 == 0:
            b[int(rng.integers(0, len(b)))] = int(rng.integers(0, 256))
        out.append((bytes(b), cap, k % (N_DAMAGED // N_DAMAGED_WAVE) == 0))
    return out


@functools.lru_cache(maxsize=None)
def damaged_results():
    """the emulator's (rc, bytes) per stream, decoded once for the tests that need them; DAMAGED_SECONDS: what building and decoding them took"""
    t0 = time.perf_counter()
    res = [[eil.inflate(s, cap, wave=w) for w in ((False, True) if wave else (False,))] for s, cap, wave in damaged_streams()]
    DAMAGED_SECONDS.append(time.perf_counter() - t0)
    return res


DAMAGED_SECONDS = []


def test_damaged_streams_get_zlibs_verdict():
    """beside test_inflate.test_corrupt_input_is_an_error_not_a_crash, which lets a damaged stream decode to anything: here a stream that zlib
    still accepts must give zlib's bytes, and one it refuses must be refused.  No case is skipped."""
    results = damaged_results()
    t0 = time.perf_counter()
    n_acc = n_wave = 0
    for (stream, cap, wave), res in zip(damaged_streams(), results):
        ok, ref = zlib_verdict(stream, cap)
        assert len(res) == (2 if wave else 1)
        for mode, (rc, out) in enumerate(res):
            assert (rc == 0) == ok and (not ok or out == ref), (stream.hex(), cap, mode, rc)
        n_acc += ok
        n_wave += wave
    assert n_wave == N_DAMAGED_WAVE and 0.2 * N_DAMAGED < n_acc < 0.95 * N_DAMAGED  # (both verdicts are well represented)
    print(f"damaged streams: {N_DAMAGED} serial, {n_wave} as a wave, zlib accepts {n_acc}: "
          f"{DAMAGED_SECONDS[0]:.1f} s for the emulator (whichever test asked first) + {time.perf_counter() - t0:.1f} s for zlib and the comparison")


# ---- the sanitizer program -----------------------------------------------------------------------------------------------------------------
def test_asan_program_over_the_catalogue_and_the_damaged_streams(tmp_path):
    """every input and output a heap block of its exact size, serial and wave: exit 0 and the library's results"""
    cases = [(e.stream, e.cap, eil.WAVE_SEED) for e in CATALOGUE] + [(s, cap, eil.WAVE_SEED if wave else 0) for s, cap, wave in damaged_streams()]
    want = [[emu(e.name, False), emu(e.name, True)] for e in CATALOGUE] + damaged_results()
    rc, err, got = eil.run_asan(cases, str(tmp_path))
    assert rc == 0, err[-3000:]
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert g == w, (k, CATALOGUE[k].name if k < len(CATALOGUE) else "damaged")


# ---- GPU -----------------------------------------------------------------------------------------------------------------------------------
# slices of the catalogue (every entry of which the two tests above have decoded as a wave, the second one under AddressSanitizer)
DEV_ACCEPTED = [e for e in CATALOGUE if e.accept and e.dev]
DEV_REJECTED = [e for e in CATALOGUE if not e.accept and e.dev]
GOOD = [BY_NAME[n] for n in ("chain_litlen", "stored_run_behind_4090")]


def _wrap(e, **kw):
    return dc.bgzf_wrap(e.stream, e.expected, **kw) if e.accept else dc.bgzf_wrap(e.stream, b"", isize=e.cap, **kw)


EOF_BLOCK = dc.bgzf_wrap(b"\x03\x00", b"")


class Dev:
    def __init__(self):
        import torch
        from portello_amd import api, synth

        self.torch, self.api = torch, api
        self.dev = torch.device("cuda", 0)
        self.index = api.Index(synth.generate(synth.config("tiny", n_reads=20, seed=5)).index_data(), 0)
        self.eng = api.Engine(self.index)

    def inflate(self, data: bytes, cap: int):
        host = np.frombuffer(data, dtype=np.uint8).copy()
        dst = self.torch.full((cap + 64,), 0xEE, dtype=self.torch.uint8, device=self.dev)
        self.torch.cuda.synchronize()
        io = self.eng.bgzf_inflate_dev(host.ctypes.data, len(data), dst.data_ptr(), cap)
        return io, dst.cpu().numpy()

    def close(self):
        self.eng.close()
        self.index.close()


@pytest.fixture(scope="module")
def dev():
    d = Dev()
    yield d
    d.close()


def _walk(buf, cap):
    import emu_cut_lib as ecl

    return ecl.bgzf_walk(buf, cap)


@pytest.mark.gpu
def test_dev_accepted_streams_in_one_call(dev):
    """the first device run of far matches (load_written), matches into and across stored runs, and long codes"""
    buf = b"".join(_wrap(e) for e in DEV_ACCEPTED) + EOF_BLOCK
    plain = b"".join(e.expected for e in DEV_ACCEPTED)
    rc, used, nb, blks = _walk(buf, len(plain))
    assert (rc, used, nb, len(blks)) == (0, len(buf), len(plain), len(DEV_ACCEPTED) + 1)
    io, got = dev.inflate(buf, len(plain))
    assert (int(io.bgzf_consumed), int(io.n_bytes), int(io.n_blocks)) == (used, nb, len(blks))
    for e, (off, coff, clen, uoff, ulen, crc) in zip(DEV_ACCEPTED, blks):
        assert got[uoff:uoff + ulen].tobytes() == e.expected, e.name
    assert (got[len(plain):] == 0xEE).all()


def _good_buffer():
    return b"".join(_wrap(e) for e in GOOD) + EOF_BLOCK, b"".join(e.expected for e in GOOD)


def _refused(dev, blocks, cap, bad_off, status):
    from portello_amd import abi

    with pytest.raises(dev.api.PortelloError) as err:
        dev.inflate(b"".join(blocks), cap)
    text = str(err.value)
    assert err.value.status == abi.PLO_ERR_IO and f"offset {bad_off} " in text and f"(status {status})" in text, text
    good, plain = _good_buffer()  # the engine is as good as before
    io, got = dev.inflate(good, len(plain))
    assert (int(io.bgzf_consumed), int(io.n_bytes), int(io.n_blocks)) == (len(good), len(plain), len(GOOD) + 1)
    assert got[:len(plain)].tobytes() == plain and (got[len(plain):] == 0xEE).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", [e.name for e in DEV_REJECTED])
def test_dev_refused_stream(dev, name):
    """one refused stream per status of inflate.hpp between two good blocks: PLO_ERR_IO, the block's offset and the emulator's status"""
    e = BY_NAME[name]
    rc = emu(name, True)[0]
    assert rc < 0
    a, b = _wrap(GOOD[0]), _wrap(GOOD[1])
    _refused(dev, [a, _wrap(e), b, EOF_BLOCK], len(GOOD[0].expected) + e.cap + len(GOOD[1].expected), len(a), rc)


@pytest.mark.gpu
def test_dev_isize_off_by_one_and_two_bad_blocks(dev):
    """ISIZE one too small is the decoder's overflow status, one too large the kernel's -9; of two bad blocks the lower offset is named"""
    a, b = _wrap(GOOD[0]), _wrap(GOOD[1])
    e = BY_NAME[ISIZE_LONG]
    n = len(e.expected)
    assert BY_NAME[ISIZE_SHORT].stream == e.stream and (BY_NAME[ISIZE_SHORT].cap, e.cap) == (n - 1, n + 1)
    assert emu(ISIZE_SHORT, True)[0] == -2 and emu(ISIZE_LONG, True) == (0, e.expected)
    total = len(GOOD[0].expected) + len(GOOD[1].expected)
    _refused(dev, [a, _wrap(e, isize=n - 1), b, EOF_BLOCK], total + n - 1, len(a), -2)
    _refused(dev, [a, _wrap(e, isize=n + 1), b, EOF_BLOCK], total + n + 1, len(a), -9)
    bad1, bad2 = BY_NAME["block_type_3"], BY_NAME["stored_nlen_mismatch"]
    assert (emu(bad1.name, True)[0], emu(bad2.name, True)[0]) == (-3, -4)
    _refused(dev, [a, _wrap(bad1), b, _wrap(bad2), EOF_BLOCK], total + bad1.cap + bad2.cap, len(a), -3)
    _refused(dev, [a, _wrap(bad2), b, _wrap(bad1), EOF_BLOCK], total + bad1.cap + bad2.cap, len(a), -4)
