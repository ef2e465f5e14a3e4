"""Hand-built DEFLATE streams (RFC 1951) for the decoder's tests: a bit writer, canonical codes from code lengths, writers for the three
block types that take the stream token by token, and the BGZF wrapper.  Nothing here checks that a stream is valid -- the point is to write
the ones no encoder emits, and the broken ones.  `Stream.expected` follows the literals, matches and stored bytes as they are written, so
that a test can hold the reference decoder's output against what the builder meant.  TEST INFRASTRUCTURE ONLY."""
import struct
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LITLEN = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32
DEFAULT_CL = [4] * 13 + [5] * 6  # a complete code over all 19 code-length symbols


def _reverse(code: int, n: int) -> int:
    rev = 0
    for b in range(n):
        rev |= ((code >> b) & 1) << (n - 1 - b)
    return rev


class BitWriter:
    """values least significant bit first, Huffman codes most significant bit first (RFC 1951, 3.1.1)"""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value: int, n: int):
        assert 0 <= value < (1 << n) or n == 0
        self.acc |= value << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, code: int, n: int):
        self.bits(_reverse(code, n), n)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data: bytes):
        assert self.n == 0
        self.out += data

    def bit_length(self) -> int:
        return 8 * len(self.out) + self.n

    def getvalue(self) -> bytes:
        return bytes(self.out) + (bytes([self.acc]) if self.n else b"")


def canonical(lengths):
    """code of every symbol from its length (RFC 1951, 3.2.2); for an over-subscribed set the codes are cut to their length"""
    count = [0] * 17
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, c = [0] * 17, 0
    for l in range(1, 17):
        c = (c + count[l - 1]) << 1
        nxt[l] = c
    codes = []
    for l in lengths:
        codes.append(nxt[l] & ((1 << l) - 1) if l else 0)
        nxt[l] += 1
    return codes


# ---- tokens -------------------------------------------------------------------------------------------------------------------------------
def lit(b):
    return ("lit", b)


def lits(data: bytes):
    return [("lit", b) for b in data]


def match(length, dist, alt258=False):
    """alt258: length 258 written as symbol 284 with 31 in its five extra bits instead of symbol 285"""
    return ("match", length, dist, alt258)


EOB = ("eob",)


def raw_ll(sym, extra=0, extra_bits=0):
    """a literal/length symbol by number (286 and 287 have codes in the fixed set), followed by extra_bits bits"""
    return ("rawl", sym, extra, extra_bits)


def raw_dist(sym, extra=0, extra_bits=0):
    """a distance symbol by number (30 and 31 have codes in the fixed set)"""
    return ("rawd", sym, extra, extra_bits)


def code_bits(code, n):
    """n bits written as a Huffman code is, whatever the block's tables say about them (a code that no symbol has)"""
    return ("bits", code, n)


def length_symbol(length, alt258=False):
    if length == 258:
        return (284, 31, 5) if alt258 else (285, 0, 0)
    for c in range(27, -1, -1):
        if length >= LEN_BASE[c]:
            return 257 + c, length - LEN_BASE[c], LEN_EXTRA[c]
    raise ValueError(length)


def dist_symbol(dist):
    for d in range(29, -1, -1):
        if dist >= DIST_BASE[d]:
            return d, dist - DIST_BASE[d], DIST_EXTRA[d]
    raise ValueError(dist)


def rle_sequence(lengths, use16=True, use17=True):
    """code lengths as the code-length symbols an encoder would write: runs of zeros as 17 / 18, repeats as 16 (for `cl_sequence`)"""
    seq, i, n = [], 0, len(lengths)
    while i < n:
        v, j = lengths[i], i
        while j < n and lengths[j] == v:
            j += 1
        run = j - i
        if v == 0:
            while run >= 11:
                k = min(run, 138)
                seq.append((18, k - 11))
                run -= k
            if run >= 3 and use17:
                seq.append((17, run - 3))
                run = 0
        else:
            seq.append(v)
            run -= 1
            while run >= 3 and use16:
                k = min(run, 6)
                seq.append((16, k - 3))
                run -= k
        seq += [v] * run
        i = j
    return seq


class Stream:
    def __init__(self):
        self.w = BitWriter()
        self.expected = bytearray()  # what the blocks written so far mean (as far as their tokens are literals, matches and stored bytes)

    def getvalue(self) -> bytes:
        return self.w.getvalue()

    def stored(self, data: bytes, last: bool, nlen=None, length=None):
        """nlen: instead of the complement of LEN; length: LEN itself, where it shall differ from len(data)"""
        n = len(data) if length is None else length
        self.w.bits(1 if last else 0, 1)
        self.w.bits(0, 2)
        self.w.align()
        self.w.raw(struct.pack("<HH", n, (n ^ 0xFFFF) if nlen is None else nlen))
        self.w.raw(data)
        self.expected += data
        return self

    def block_type(self, btype: int, last: bool):
        self.w.bits(1 if last else 0, 1)
        self.w.bits(btype, 2)
        return self

    def _tokens(self, tokens, ll_len, ll_code, d_len, d_code):
        w = self.w
        lit_rev = [_reverse(ll_code[b], ll_len[b]) for b in range(256)]  # (most tokens of a long stream are literals)
        for t in tokens:
            k = t[0]
            if k == "lit":
                w.bits(lit_rev[t[1]], ll_len[t[1]])
                self.expected.append(t[1])
            elif k == "match":
                _, length, dist, alt = t
                s, ev, eb = length_symbol(length, alt)
                assert ll_len[s], ("no code for length symbol", s)
                w.code(ll_code[s], ll_len[s])
                w.bits(ev, eb)
                d, dv, db = dist_symbol(dist)
                assert d < len(d_len) and d_len[d], ("no code for distance symbol", d)
                w.code(d_code[d], d_len[d])
                w.bits(dv, db)
                if dist <= len(self.expected):
                    for _ in range(length):
                        self.expected.append(self.expected[-dist])
            elif k == "eob":
                w.code(ll_code[256], ll_len[256])
            elif k == "rawl":
                w.code(ll_code[t[1]], ll_len[t[1]])
                w.bits(t[2], t[3])
            elif k == "rawd":
                w.code(d_code[t[1]], d_len[t[1]])
                w.bits(t[2], t[3])
            elif k == "bits":
                w.code(t[1], t[2])
            else:
                raise ValueError(t)

    def fixed(self, tokens, last: bool):
        self.block_type(1, last)
        self._tokens(tokens, FIXED_LITLEN, canonical(FIXED_LITLEN), FIXED_DIST, canonical(FIXED_DIST))
        return self

    def dynamic(self, litlen_lengths, dist_lengths, tokens, last: bool, cl_lengths=None, cl_sequence=None, hlit=None, hdist=None):
        """litlen_lengths / dist_lengths: the code lengths the header carries (at least 257 / 1 of them).  cl_lengths: the lengths of the 19
        code-length codes by symbol.  cl_sequence: the code-length symbols to write instead of one plain symbol per length, 16 / 17 / 18 as
        (symbol, value of the extra bits).  hlit / hdist: the header's five-bit fields, which need not agree with anything."""
        ll, dl = list(litlen_lengths), list(dist_lengths)
        cl = list(DEFAULT_CL if cl_lengths is None else cl_lengths)
        assert len(cl) == 19 and len(ll) >= 257 and len(dl) >= 1
        w = self.w
        self.block_type(2, last)
        w.bits(len(ll) - 257 if hlit is None else hlit, 5)
        w.bits(len(dl) - 1 if hdist is None else hdist, 5)
        ncl = 19
        while ncl > 4 and cl[CL_ORDER[ncl - 1]] == 0:
            ncl -= 1
        w.bits(ncl - 4, 4)
        for i in range(ncl):
            w.bits(cl[CL_ORDER[i]], 3)
        cl_code = canonical(cl)
        for s in (ll + dl if cl_sequence is None else cl_sequence):
            sym, extra = s if isinstance(s, tuple) else (s, 0)
            assert cl[sym], ("no code for code-length symbol", sym)
            w.code(cl_code[sym], cl[sym])
            if sym >= 16:
                w.bits(extra, {16: 2, 17: 3, 18: 7}[sym])
        self._tokens(tokens, ll + [0] * (288 - len(ll)), canonical(ll) + [0] * (288 - len(ll)), dl + [0] * (32 - len(dl)), canonical(dl) + [0] * (32 - len(dl)))
        return self


def lengths_of(n, assign):
    """n code lengths, zero but for {symbol: length}"""
    out = [0] * n
    for s, l in assign.items():
        out[s] = l
    return out


def bgzf_wrap(deflate: bytes, payload: bytes, isize=None, crc=None) -> bytes:
    """one BGZF block around a deflate stream said to inflate to `payload` (the layout of test_window_cut_dev.bgzf_block)"""
    assert len(deflate) + 26 <= 65536
    return (b"\x1f\x8b\x08\x04" + bytes(6) + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, len(deflate) + 25) + deflate +
            struct.pack("<II", (zlib.crc32(payload) & 0xFFFFFFFF) if crc is None else crc, len(payload) if isize is None else isize))
