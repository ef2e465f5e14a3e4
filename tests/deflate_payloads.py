"""Payloads that take the encoder of portello_amd/csrc/deflate.hpp to its own edges, each with the condition that proves it got there.
The condition is checked on the trace (tests/deflate_trace.py) of the block the encoder wrote: a case whose payload misses its edge fails.
What the builders know of the encoder is what deflate.hpp's header comment says: rounds of 64 positions, one table entry per 12-bit hash
with the highest position staying, candidates from earlier rounds only, distance 1 tried beside the table, a greedy parse, a 3-byte match
farther than 4096 dropped, a stored block where the dynamic one is not smaller.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from deflate_craft import DIST_BASE, LEN_BASE, dist_symbol, length_symbol
from deflate_trace import rounds, unlimited_depth

BLOCK = 0xff00
HASH_MULT, HASH_BITS = 0x9E3779B1, 12  # restated from deflate.hpp (def_tokenize); a changed hash fails the bucket cases, as it should


def bucket(t):
    v = t[0] | (t[1] << 8) | (t[2] << 16)
    return ((v * HASH_MULT) & 0xFFFFFFFF) >> (32 - HASH_BITS)


def rnd(seed, n, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, n, dtype=np.uint8).tobytes()


def counter(n, start=1):
    """n bytes of a 16-bit counter, high byte first: no trigram occurs twice, no byte three times in a row"""
    out = bytearray()
    i = start
    while len(out) < n:
        out += bytes([(i >> 8) & 255, i & 255])
        i += 1
    return bytes(out[:n])


def colliding(t, lo=0x80, hi=0x100):
    """the first trigram of three different bytes in [lo, hi) that shares t's bucket and none of its bytes"""
    want = bucket(t)
    for a in range(lo, hi):
        for b in range(lo, hi):
            for c in range(lo, hi):
                u = bytes([a, b, c])
                if len(set(u)) == 3 and not set(u) & set(t) and bucket(u) == want:
                    return u
    raise AssertionError("no colliding trigram")


PAD = bytes(517)  # a literal and two matches of 258 at distance 1: the round behind them starts at 517, as the first does at 0


class Case:
    def __init__(self, name, core, cond, stored, pad):
        self.name, self.core, self.cond, self.stored = name, bytes(core), cond, stored  # stored: the block must take the stored form
        self.start = len(PAD) if pad else 0
        self.payload = (PAD if pad else b"") + self.core

    def __repr__(self):
        return self.name


class View:
    """the tokens of a traced block that start in [start, start + n), positions counted from `start`; everything else is the block's"""

    def __init__(self, tr, start, n):
        self.tr, self.n = tr, n
        keep = [i for i, p in enumerate(tr.positions) if start <= p < start + n] if tr.btype else []
        self.tokens, self.positions = [tr.tokens[i] for i in keep], [tr.positions[i] - start for i in keep]

    def __getattr__(self, name):
        return getattr(self.tr, name)

    def matches(self):
        return [(p, t[0], t[1]) for p, t in zip(self.positions, self.tokens) if isinstance(t, tuple)]

    def rounds(self):
        return rounds(self, self.n)


CASES = []


def case(name, core, cond=None, stored=False, pad=False):
    """pad: zeros in front that make the block a dynamic one whatever the core is, and leave the rounds of the core as they would be alone
    (the core must not start with a zero, and its positions in the table are 517 higher)"""
    assert all(c.name != name for c in CASES) and not (pad and core[:1] == b"\0"), name
    CASES.append(Case(name, core, cond, stored, pad))
    assert len(CASES[-1].payload) <= BLOCK


def _lens(tr):
    return [(l, d) for _, l, d in tr.matches()]


def _dynamic(tr):
    assert tr.btype == 2, tr.btype


# ---- distances ---------------------------------------------------------------------------------------------------------------------------
def far(d, tail=b"\x07" * 50):
    r = rnd(5, 300, 1)
    return r + bytes(d - 300) + r + tail


def _far_cond(d):
    def cond(tr, p):
        _dynamic(tr)
        ms = tr.matches()
        assert all(dist <= 32768 for _, _, dist in ms)
        if d <= 32768:
            assert any(l >= 100 and dist == d and pos == d for pos, l, dist in ms), [m for m in ms if m[2] > 1]
        else:
            assert all(dist <= 1 for _, _, dist in ms), [m for m in ms if m[2] > 1]
    return cond


for _d in (32767, 32768, 32769):
    case(f"far_{_d}", far(_d), _far_cond(_d))


def too_far(rep, d):
    return rep + counter(d - len(rep)) + rep + b"\xee\xed"


case("three_at_4096", too_far(b"\xf1\xf2\xf3", 4096), lambda tr, p: (_dynamic(tr), _eq(tr.matches(), [(4096, 3, 4096)])))
case("three_at_4097", too_far(b"\xf1\xf2\xf3", 4097), lambda tr, p: (_dynamic(tr), _eq(tr.matches(), [])))
case("four_at_4097", too_far(b"\xf1\xf2\xf3\xf4", 4097), lambda tr, p: (_dynamic(tr), _eq(tr.matches(), [(4097, 4, 4097)])))


def _eq(a, b):
    assert a == b, (a, b)


_X = b"\xa1\xb2\xc3\xd4\xe5\xf6"
case("source_at_0", _X + counter(70) + _X + b"\x99\x98" + bytes(600),
     lambda tr, p: _eq([m for m in tr.matches() if m[0] - m[2] == 0], [(76, 6, 76)]))


def tail_source():
    # zeros: a literal, 252 matches of 258 and one of 179 end at 65196, where a round starts; the source fills its first 20 lanes,
    # 44 different bytes the rest; the copy is the next round's lane 0 and the payload's end
    s = rnd(9, 20, 0x80)
    p = bytes(65196) + s + bytes(range(1, 45)) + s
    assert len(p) == BLOCK
    return p


def _tail_cond(tr, p):
    pos, l, d = tr.matches()[-1]
    assert (pos, l, d) == (BLOCK - 20, 20, 64) and pos - d >= 65000 and pos + l == len(p)
    assert tr.rounds()[-1] == (BLOCK - 20, [(0, (20, 64))])


case("source_in_the_last_64_bytes", tail_source(), _tail_cond)

# ---- lengths -----------------------------------------------------------------------------------------------------------------------------
LENGTHS = [3, 4, 10, 11, 12, 18, 19, 130, 131, 257, 258, 259, 260, 261, 516, 517]  # (260, 261: a rest of 2 and of 3 behind a 258)


def _split(total):
    return [258] * (total // 258) + ([total % 258] if total % 258 >= 3 else [])


def _run_case(L):
    p = b"\x11\x22\x33" + b"R" * (L + 1) + b"\x44\x55"
    case(f"run_{L}", p, lambda tr, p: _eq(_lens(tr), [(l, 1) for l in _split(L)]), pad=True)


def _rep_case(L, fill=70):
    a = rnd(1000 + L, L, 0x80)
    p = a + counter(fill) + a + b"\x01\x02"
    case(f"repeat_{L}", p, lambda tr, p: _eq(_lens(tr), [(l, L + fill) for l in _split(L)]), pad=True)


for _L in LENGTHS:
    _run_case(_L)
    _rep_case(_L)

_A = rnd(77, 20, 0x80)


def _ends_with_match(tr, p):
    pos, l, d = tr.matches()[-1]
    assert pos + l == len(p) and (l, d) == (20, 90)


case("match_ends_the_payload", _A + counter(70) + _A, _ends_with_match, pad=True)
case("run_ends_the_payload", b"\x31\x32" + b"w" * 41, lambda tr, p: _eq(tr.matches(), [(3, 40, 1)]), pad=True)
case("last_two_unhashed", _A + counter(70) + _A[:2], lambda tr, p: (_dynamic(tr), _eq(tr.matches(), [])), pad=True)
case("last_one_unhashed", _A + counter(70) + _A[:1], lambda tr, p: (_dynamic(tr), _eq(tr.matches(), [])), pad=True)
case("last_two_equal", _A + counter(70) + b"zz", lambda tr, p: (_dynamic(tr), _eq(tr.matches(), [])), pad=True)
for _n in (3, 4, 5):  # (a dynamic header of 17 + 3 x 18 bits and a dozen code-length symbols is longer than 5 + n bytes)
    case(f"one_byte_x{_n}", b"a" * _n, stored=True)


# ---- rounds of 64 positions ----------------------------------------------------------------------------------------------------------------
def _lane_63_and_0(tr, p):
    r = tr.rounds()
    assert r[0][1][-1] == (63, (258, 1)) and r[1][0] == 321 and r[1][1][0] == (0, (10, 1)), r


case("match_at_lane_63_and_lane_0", counter(62) + b"z" * (1 + 258 + 10) + b"\x01\x02\x03", _lane_63_and_0)


def _lane_10(tr, p):
    r = tr.rounds()
    assert r[0][1][-1] == (10, (258, 1)) and r[1][0] == 268 and _lens(tr) == [(258, 1)], r


case("match_from_lane_10_skips_a_round", counter(9) + b"y" * 259 + counter(30, 500), _lane_10)


def covered():
    a, e = b"\x81\x92\xa3\xb4\xc5\xd6\xe7\xf8", b"\x8a\x9b\xac\xbd"
    p = a + counter(12) + a[4:] + e + counter(36, 100)
    assert len(p) == 64
    return p + a + e + b"\x01\x02"


def _covered_cond(tr, p):
    # lane 4 of the second round holds (8, 48), longer than lane 0's (8, 64) is far: the greedy parse never looks at it
    assert tr.matches() == [(64, 8, 64), (72, 4, 48)] and 68 not in tr.positions


case("match_under_an_earlier_match", covered(), _covered_cond, pad=True)
for _n in (63, 64, 65, 127, 128, 129, 191, 192):
    case(f"acgt_{_n}", bytes(np.random.default_rng(_n).choice(np.frombuffer(b"ACGT", np.uint8), _n)), (lambda tr, p: _dynamic(tr)) if _n >= 129 else None)

# ---- hash table ------------------------------------------------------------------------------------------------------------------------------
_T1 = b"Q7k"
_T2 = colliding(_T1)
_T3 = bytes([_T2[0], _T2[1], _T2[2] ^ 1])
assert bucket(_T2) == bucket(_T1) != bucket(_T3)


def evict(t2):
    p = _T1 + b"\x01\x02" + t2 + b"\x03\x04" + counter(54, 700)
    assert len(p) == 64 and bucket(_T1) not in [bucket(p[i:i + 3]) for i in range(1, 62) if p[i:i + 3] != t2]
    return p + _T1 + b"\x05\x06"


case("bucket_evicted_by_a_collision", evict(_T2), lambda tr, p: (_dynamic(tr), _eq(tr.matches(), [])), pad=True)
case("bucket_kept_without_the_collision", evict(_T3), lambda tr, p: _eq(tr.matches(), [(64, 3, 64)]), pad=True)
_T4 = colliding(b"aaa")
case("candidate_fails_distance_1_holds", _T4 + counter(60, 900) + b"\x05" + b"a" * 21 + b"\x06\x07", lambda tr, p: _eq(tr.matches(), [(65, 20, 1)]), pad=True)
# 64 lanes insert `bbb` in the first round; the highest, 63, stays: distance 4 from 67 (the lowest would give 67)
case("one_hash_from_64_lanes", b"b" * 66 + b"X" + b"bbb" + b"YZ", lambda tr, p: _eq(tr.matches(), [(1, 65, 1), (67, 3, 4)]))


# ---- Huffman header --------------------------------------------------------------------------------------------------------------------------
case("empty", b"", stored=True)
case("one_literal", b"a", stored=True)


def _one_kind(tr, p):
    _dynamic(tr)
    assert {t for t in tr.tokens if not isinstance(t, tuple)} == {ord("a")}
    assert tr.hdist == 2 and tr.d_lengths == [1, 1] and {d for _, _, d in tr.matches()} == {1}  # distance code 0 and the added code 1
    assert tr.hclen < 19


case("one_literal_kind_one_distance_code_0", b"a" * 1000, _one_kind)


def _no_match(tr, p):
    _dynamic(tr)
    assert tr.matches() == [] and tr.hdist == 2 and tr.d_lengths == [1, 1]  # HDIST field 1: two one-bit codes, neither used


case("no_match_in_a_dynamic_block", counter(2000), _no_match)


def _one_dist_13(tr, p):
    _dynamic(tr)
    assert len(_lens(tr)) == 7 and all(l >= 30 and d == 100 for l, d in _lens(tr)), _lens(tr)
    assert tr.hdist == 14 and [i for i, l in enumerate(tr.d_lengths) if l] == [0, 13] and tr.d_lengths[0] == tr.d_lengths[13] == 1  # code 0 is the added one


_B = rnd(78, 30, 0x80)
case("one_distance_code_13", b"".join(_B + bytes([0x10 + k]) + counter(69, 100 * k) for k in range(1, 8)) + _B + b"\x01", _one_dist_13)


def all_codes(seed):
    """a match in every distance class j = 0 .. 29 whose length lies in length class min(j, 28)"""
    rng = np.random.default_rng(seed)
    buf, cur, fresh, fill = bytearray(), [0], [0], counter(2000)

    def lits(data):
        buf.extend(data)
        while len(buf) >= cur[0] + 64:
            cur[0] += 64

    def pad_to_lane(k):
        while (len(buf) - cur[0]) != k:  # (literals: the counter's bytes in their order, no trigram twice)
            lits(fill[fresh[0]:fresh[0] + 1])
            fresh[0] += 1

    def copy(d, L):
        at = len(buf)
        for _ in range(L):
            buf.append(buf[-d])
        if len(buf) >= cur[0] + 64:
            cur[0] = len(buf)
        nxt = buf[-d]  # what would lengthen the match
        lits(bytes([(nxt + 1) & 255 or 1]))
        return at

    want = []
    lits(b"\xee")
    want.append((len(buf), 3, 1))
    copy(1, 3)
    for j in range(1, 12):  # distances below 64: the source ends a round, the copy starts the next
        d, L = DIST_BASE[j], LEN_BASE[j]
        pad_to_lane(64 - d)
        lits(bytes((rng.permutation(128)[:d] + 128).astype(np.uint8)))  # (different bytes: no run that distance 1 would take)
        assert len(buf) == cur[0]
        want.append((len(buf), L, d))
        copy(d, L)
    for j in range(12, 22):  # source, zeros, copy
        d, L = DIST_BASE[j] + 1, LEN_BASE[j]
        lits(bytes(rng.integers(0x80, 0x100, L, dtype=np.uint8)))
        buf.extend(bytes(d - L))
        want.append((len(buf), L, d))
        copy(d, L)
    src = {}
    for j in range(22, 30):  # the sources of the far matches side by side, their copies among zeros
        L = LEN_BASE[min(j, 28)] if j < 29 else 10
        src[j] = (len(buf), L)
        buf.extend(bytes(rng.integers(0x80, 0x100, L, dtype=np.uint8)))
        buf.append(j)  # (ends the string: the next one starts with another byte than the zeros behind a copy)
    for j in range(22, 30):
        s, L = src[j]
        q = s + DIST_BASE[j] + 5
        assert q >= len(buf) + 4
        buf.extend(bytes(q - len(buf)))
        want.append((q, L, q - s))
        buf.extend(buf[s:s + L])
        buf.append(0x7f)
    return bytes(buf), want


_ALL, _ALL_WANT = all_codes(6)  # (seeds 1 .. 5 lose one of the far sources to a later string in its bucket)


def _all_cond(tr, p):
    _dynamic(tr)
    ms = tr.matches()
    missing = [w for w in _ALL_WANT if w not in ms]
    assert not missing, missing
    assert {length_symbol(l)[0] for _, l, _ in ms} == set(range(257, 286)) and {dist_symbol(d)[0] for _, _, d in ms} == set(range(30))
    assert tr.hlit == 286 and tr.hdist == 30


case("all_length_symbols_and_distance_codes", _ALL, _all_cond)
case("hclen_trimmed", bytes(np.random.default_rng(4).choice(np.frombuffer(b"ACGT", np.uint8), 400)), lambda tr, p: (_dynamic(tr), _lt(tr.hclen, 19), _eq(tr.cl_lengths[15], 0)))


def _lt(a, b):
    assert a < b, (a, b)


def _cl_limited(tr, p):
    _dynamic(tr)
    cf = tr.histograms()[2]
    assert unlimited_depth(cf) > 7 and max(tr.cl_lengths) <= 7, (unlimited_depth(cf), tr.cl_lengths)


def mixed(seed):
    """random bytes over a random alphabet, zeros, random bytes again and a run: what the search for a limited code-length code ran
    over.  Of the seeds 0 .. 399 six meet _cl_limited (15, 66, 80, 86, 92, 179); the first two are kept."""
    rng = np.random.default_rng(seed)
    k, a = int(rng.integers(100, 700)), int(rng.integers(60, 256))
    r = bytes(rng.integers(1, a, k, dtype=np.uint8))
    return r + bytes(int(rng.integers(300, 1500))) + bytes(rng.integers(1, a, int(rng.integers(0, 300)), dtype=np.uint8)) + b"\x07" * int(rng.integers(0, 60))


CL_LIMIT_SEEDS = (15, 66)
case("code_length_code_limited_far_32769", far(32769, b"\x07" * 51), _cl_limited)
for _s in CL_LIMIT_SEEDS:
    case(f"code_length_code_limited_seed_{_s}", mixed(_s), _cl_limited)


def _runs(lengths):
    out, i = [], 0
    while i < len(lengths):
        j = i
        while j < len(lengths) and lengths[j] == lengths[i]:
            j += 1
        out.append((lengths[i], j - i))
        i = j
    return out


def zero_runs_a():
    """byte values present: 0-2 | 5-8 | 12-18 | 29-36 | 48 | 187, so that the literal lengths have zero runs of 2, 3, 10, 11 and 138; the
    counts 2 (0-2), 4 (5-8, 29-36), 1 (12-18, 48, 187) and the end-of-block symbol add up to 64 = a dyadic code: lengths 5, 4 and 6"""
    vals = [v for v in range(0, 3) for _ in range(2)] + [v for v in list(range(5, 9)) + list(range(29, 37)) for _ in range(4)] + list(range(12, 19)) + [48, 187]
    assert len(vals) == 63
    return bytes(np.random.default_rng(2).permutation(np.array(vals, np.uint8)))


def _zero_runs_a(tr, p):
    _dynamic(tr)
    assert tr.matches() == []
    assert _runs(tr.ll_lengths[:256]) == [(5, 3), (0, 2), (4, 4), (0, 3), (6, 7), (0, 10), (4, 8), (0, 11), (6, 1), (0, 138), (6, 1), (0, 68)]
    seq = tr.cl_seq
    for want in ([(5, 0)] * 3 + [(0, 0)] * 2 + [(4, 0), (16, 0)], [(17, 0), (6, 0), (16, 3), (17, 7), (4, 0), (16, 3), (4, 0), (18, 0), (6, 0), (18, 127), (6, 0)]):
        assert any(seq[i:i + len(want)] == want for i in range(len(seq))), (want, seq)


case("zero_runs_2_3_10_11_138", zero_runs_a(), _zero_runs_a)


def _zero_run_139(tr, p):
    _dynamic(tr)
    assert _runs(tr.ll_lengths[:256])[:2] == [(tr.ll_lengths[0], 1), (0, 139)]
    assert tr.cl_seq[1:4] == [(18, 127), (0, 0), (tr.ll_lengths[140], 0)], tr.cl_seq[:6]


case("zero_run_139", bytes(np.random.default_rng(3).choice(np.array([0, 140, 141, 142, 143], np.uint8), 300)), _zero_run_139)

# ---- stored fallback at level 1 ---------------------------------------------------------------------------------------------------------------
_TEXT = b"Pack my box with five dozen liquor jugs!"  # (31 different bytes among 40: their code lengths alone outweigh what the codes save)
for _n in (1, 2, 40):
    case(f"text_{_n}_stored", _TEXT[:_n], stored=True)
case("random_300_stored", rnd(300, 300), stored=True)


def sparse(seed):
    """600 bytes over 150 + seed % 80 values: the dynamic form wins or loses by a few bytes (what the search for the near-stored case ran over)"""
    rng = np.random.default_rng(seed)
    return bytes(rng.integers(0, 150 + seed % 80, 600, dtype=np.uint8))


NEAR_STORED_SEED = 24  # (of the seeds 0 .. 399 the first five the dynamic form wins by 1 .. 8 bytes: 20 .. 24; this one by the fewest, 5)


def _near_stored(tr, p):
    _dynamic(tr)
    assert 18 + 5 + len(p) + 8 - 8 <= 18 + (tr.bits + 7) // 8 + 8 < 18 + 5 + len(p) + 8


case("dynamic_wins_by_at_most_8_bytes", sparse(NEAR_STORED_SEED), _near_stored)


def full_size_cycle():
    """seven payloads of 0xff00 bytes with very different token counts, for a wave's second block on the device"""
    import test_bgzf_dev as tb

    rng = np.random.default_rng(21)
    return [bytes(rng.integers(32, 96, BLOCK, dtype=np.uint8)),                        # nearly all literals: 65 k tokens
            b"\x2a" * BLOCK,                                                            # all runs: 255 tokens
            b"".join(tb.hifi_like_stream(BLOCK))[:BLOCK],                                # a record stream with long runs
            (far(32768, b"") * 2)[:BLOCK],                                               # far matches
            b"".join(tb.bam_like_stream(BLOCK, seed=5))[:BLOCK],                         # a record stream without runs
            (b"the quick brown fox jumps over the lazy dog " * 1500)[:BLOCK],            # near repeats of every length
            bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), BLOCK))]                  # short matches
