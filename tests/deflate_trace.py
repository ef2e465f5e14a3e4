"""A tracing DEFLATE decoder (RFC 1951) for the encoder's tests: where zlib says only whether a block inflates, this one says what the
block is made of -- its header fields, the code-length sequence as written, the two sets of code lengths, every token, and where in the
encoder's rounds of 64 positions a token starts.  Written from the RFC on the tables of tests/deflate_craft.py; plain Python, slow, and
strict: anything the RFC does not allow raises TraceError.  Beside it the yardsticks for a Huffman code: `optimal_cost` and
`unlimited_depth` of a plain heapq tree.  TEST INFRASTRUCTURE ONLY."""
import heapq

from deflate_craft import CL_ORDER, DIST_BASE, DIST_EXTRA, FIXED_DIST, FIXED_LITLEN, LEN_BASE, LEN_EXTRA, canonical, dist_symbol, length_symbol


class TraceError(Exception):
    pass


class _Bits:
    def __init__(self, data):
        self.data, self.at, self.acc, self.n = data, 0, 0, 0

    def need(self, n):  # zeros behind the end: a code is looked up in a window wider than itself; `pos` tells how far the stream went
        while self.n < n:
            self.acc |= (self.data[self.at] if self.at < len(self.data) else 0) << self.n
            self.at += 1
            self.n += 8

    def take(self, n):
        if n == 0:
            return 0
        self.need(n)
        v = self.acc & ((1 << n) - 1)
        self.acc >>= n
        self.n -= n
        return v

    @property
    def pos(self):  # bits consumed
        return 8 * self.at - self.n

    def align(self):
        self.take(self.n & 7)


def _reverse(code, n):
    rev = 0
    for b in range(n):
        rev |= ((code >> b) & 1) << (n - 1 - b)
    return rev


class _Code:
    """a canonical code from its lengths; a lookup table over the next `width` bits of the stream"""

    def __init__(self, lengths, what):
        used = [l for l in lengths if l]
        self.width = max(used) if used else 0
        kraft = sum(1 << (self.width - l) for l in used)
        if kraft > 1 << self.width:
            raise TraceError(f"{what}: over-subscribed code")
        self.table = [None] * (1 << self.width)
        for s, (l, c) in enumerate(zip(lengths, canonical(lengths))):
            if l:
                r = _reverse(c, l)
                for k in range(1 << (self.width - l)):
                    self.table[r | (k << l)] = (s, l)
        self.what = what

    def read(self, br):
        br.need(self.width)
        e = self.table[br.acc & ((1 << self.width) - 1)] if self.width else None
        if e is None:
            raise TraceError(f"{self.what}: a code that no symbol has")
        br.acc >>= e[1]
        br.n -= e[1]
        return e


class Block:
    """one traced block.  tokens: an int (a literal byte) or (length, distance); positions[i]: where in the output token i starts"""
    btype = final = None
    hlit = hdist = hclen = None   # the COUNTS (257 .. 286, 1 .. 30, 4 .. 19), not the header's fields
    cl_lengths = None             # the 19 lengths of the code-length code, by symbol
    cl_seq = None                 # the code-length symbols as written: (symbol, value of the extra bits)
    ll_lengths = d_lengths = None
    tokens = positions = None
    widest = 0                    # the widest token, in bits, extra bits included
    eob_bits = 0
    bits = 0                      # bits of the block, header and end-of-block symbol included
    stored = b""

    def matches(self):
        return [(p, t[0], t[1]) for p, t in zip(self.positions, self.tokens) if isinstance(t, tuple)]

    def histograms(self):
        """(literal/length[286], distance[30], code-length[19]) counts rebuilt from the tokens and the code-length sequence"""
        lf, df, cf = [0] * 286, [0] * 30, [0] * 19
        for t in self.tokens:
            if isinstance(t, tuple):
                lf[length_symbol(t[0])[0]] += 1
                df[dist_symbol(t[1])[0]] += 1
            else:
                lf[t] += 1
        lf[256] += 1
        for s, _ in self.cl_seq or []:
            cf[s] += 1
        return lf, df, cf


def trace_stream(data, max_out=None):
    """every block of a deflate stream -> ([Block], output bytes, bits consumed)"""
    br, out, blocks = _Bits(data), bytearray(), []
    while True:
        b = Block()
        start = br.pos
        b.final, b.btype = br.take(1), br.take(2)
        b.tokens, b.positions = [], []
        if b.btype == 0:
            br.align()
            n, nn = br.take(16), br.take(16)
            if n ^ nn != 0xFFFF:
                raise TraceError("stored block: LEN and NLEN disagree")
            at = br.pos // 8
            if at + n > len(data):
                raise TraceError("stored block: past the end of the stream")
            b.stored = bytes(data[at:at + n])
            b.positions = [len(out)]
            out += b.stored
            br.at, br.acc, br.n = at + n, 0, 0
        elif b.btype in (1, 2):
            if b.btype == 1:
                b.ll_lengths, b.d_lengths = list(FIXED_LITLEN), list(FIXED_DIST)
            else:
                _dynamic_header(br, b)
            _tokens(br, b, out, max_out)
        else:
            raise TraceError("block type 3")
        b.bits = br.pos - start
        blocks.append(b)
        if br.pos > 8 * len(data):
            raise TraceError("the stream ends inside a block")
        if b.final:
            return blocks, bytes(out), br.pos


def trace_block(data):
    """the deflate data of ONE final block that fills `data` to its last byte -> (Block, output bytes)"""
    blocks, out, bits = trace_stream(data)
    if len(blocks) != 1:
        raise TraceError(f"{len(blocks)} blocks")
    if (bits + 7) // 8 != len(data):
        raise TraceError(f"{len(data) - (bits + 7) // 8} bytes behind the block")
    return blocks[0], out


def _dynamic_header(br, b):
    b.hlit, b.hdist, b.hclen = br.take(5) + 257, br.take(5) + 1, br.take(4) + 4
    if b.hlit > 286 or b.hdist > 30:
        raise TraceError("HLIT / HDIST out of range")
    b.cl_lengths = [0] * 19
    for i in range(b.hclen):
        b.cl_lengths[CL_ORDER[i]] = br.take(3)
    cl = _Code(b.cl_lengths, "code-length code")
    lengths, b.cl_seq = [], []
    total = b.hlit + b.hdist
    while len(lengths) < total:
        s, _ = cl.read(br)
        if s < 16:
            b.cl_seq.append((s, 0))
            lengths.append(s)
            continue
        eb = {16: 2, 17: 3, 18: 7}[s]
        ev = br.take(eb)
        b.cl_seq.append((s, ev))
        if s == 16:
            if not lengths:
                raise TraceError("repeat with nothing in front")
            lengths += [lengths[-1]] * (3 + ev)
        else:
            lengths += [0] * ((3 if s == 17 else 11) + ev)
    if len(lengths) != total:
        raise TraceError("a run crosses the end of the code lengths")
    b.ll_lengths, b.d_lengths = lengths[:b.hlit], lengths[b.hlit:]
    if not b.ll_lengths[256]:
        raise TraceError("no code for end of block")


def _tokens(br, b, out, max_out):
    ll = _Code(b.ll_lengths, "literal/length code")
    dc = _Code(b.d_lengths, "distance code")
    while True:
        s, l = ll.read(br)
        if s < 256:
            b.tokens.append(s)
            b.positions.append(len(out))
            out.append(s)
            b.widest = max(b.widest, l)
        elif s == 256:
            b.eob_bits = l
            return
        else:
            if s > 285:
                raise TraceError("length symbol 286 / 287")
            c = s - 257
            w = l + LEN_EXTRA[c]
            length = LEN_BASE[c] + br.take(LEN_EXTRA[c])
            d, l2 = dc.read(br)
            if d > 29:
                raise TraceError("distance symbol 30 / 31")
            dist = DIST_BASE[d] + br.take(DIST_EXTRA[d])
            w += l2 + DIST_EXTRA[d]
            if dist > len(out):
                raise TraceError("distance in front of the output")
            b.tokens.append((length, dist))
            b.positions.append(len(out))
            b.widest = max(b.widest, w)
            if dist == 1:
                out += out[-1:] * length
            else:
                for _ in range(length):
                    out.append(out[-dist])
        if max_out is not None and len(out) > max_out:
            raise TraceError("output too long")


def rounds(block, n):
    """The encoder's rounds of 64 positions, restated from deflate.hpp's header comment and derived from the tokens alone: a round starts at
    `cur`, the tokens that start in [cur, cur + 64) belong to it, and the next round starts where the last of them ends (a match may run
    past the 64 positions).  -> [(cur, [(lane, token), ...])]"""
    ends = block.positions[1:] + [n]
    out, cur, i = [], 0, 0
    while cur < n:
        here, end = [], cur
        while i < len(block.tokens) and block.positions[i] < cur + 64:
            here.append((block.positions[i] - cur, block.tokens[i]))
            end = ends[i]
            i += 1
        out.append((cur, here))
        assert end > cur
        cur = max(end, min(cur + 64, n))
    return out


# ---- the yardsticks of a Huffman code ----------------------------------------------------------------------------------------------------
def _tree(freqs):
    """code lengths of a Huffman tree over the non-zero counts, by a heap.  Equal weights: the shallower subtree first, which gives the
    least depth among the optimal trees (the cost is the same for all of them)."""
    used = [(f, 0, s) for s, f in enumerate(freqs) if f]
    depth = {s: 0 for _, _, s in used}
    if len(used) == 1:
        return {used[0][2]: 1}
    heap = [(f, 0, s, [s]) for f, _, s in used]
    heapq.heapify(heap)
    tie = len(freqs)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        for s in a[3] + b[3]:
            depth[s] += 1
        tie += 1
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1, tie, a[3] + b[3]))
    return depth


def unlimited_depth(freqs):
    d = _tree(freqs)
    return max(d.values()) if d else 0


def optimal_cost(freqs):
    d = _tree(freqs)
    return sum(freqs[s] * l for s, l in d.items())


def cost(freqs, lengths):
    return sum(f * l for f, l in zip(freqs, lengths))
