"""Hand-built batches at the edges of the enumerate pass and of the batch checks (k_seg_count and its neighbours in engine.hip): the
catalogue of tests/test_enumerate_edges.py.  TEST INFRASTRUCTURE ONLY.

Every case is a named (index, batch) pair with the verdict written by hand beside it and a line on what it is there for.  Nothing here
depends on PLO_SEG_LANES: where a lane or step border matters the grid covers every multiple of 4 up to 64.

One small hand index serves all cases (INDEX).  Every contig segment has a one-block CIGAR, so its block map has the two keys
[start, end) of the block in the coordinates of its strand and an item's region is its merged op count + 4 (enumerate_expect.region_dwords
with one key inside the item's span).  Contigs:
    C_TWO    2000 bases: [0, 1000) forward on chr0, [1000, 2000) REVERSE on chr1
    C_NONE   2000 bases the index never saw (no segments)
    C_ONE    1000 bases: [100, 900) reverse
    C_THREE  1000 bases: [0, 300) forward, [300, 600) reverse, [700, 1000) forward (a gap in front of the last)
    C_FIVE   1000 bases: five segments of 200, strands alternating from forward
    C_NINE    900 bases: nine segments of 100, strands alternating from reverse"""
from dataclasses import dataclass
from typing import Optional

import numpy as np

import enumerate_expect as ex
from enumerate_expect import OK, INVALID_ARG, RANGE, OP_M, OP_I, OP_D, OP_N, OP_S, OP_H, OP_P, OP_EQ, OP_X, op
from portello_amd import abi

C_TWO, C_NONE, C_ONE, C_THREE, C_FIVE, C_NINE = range(6)
_CONTIGS = [
    (2000, [(0, 1000, 1, 0, 100, 50), (1000, 2000, 0, 1, 200, 20)]),
    (2000, []),
    (1000, [(100, 900, 0, 0, 1200, 33)]),
    (1000, [(0, 300, 1, 1, 1300, 11), (300, 600, 0, 0, 2100, 12), (700, 1000, 1, 1, 1700, 13)]),
    (1000, [(200 * k, 200 * k + 200, (k + 1) % 2, k % 2, 2400 + 210 * k, 40 + k) for k in range(5)]),
    (900, [(100 * k, 100 * k + 100, k % 2, (k + 1) % 2, 2600 + 120 * k, 20 + k) for k in range(9)]),
]


def make_index() -> abi.IndexData:
    rng = np.random.default_rng(77)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    contig_len, seg_off, chrom, pos, fwd, mapq, s0, s1, cigs, rev = [], [0], [], [], [], [], [], [], [], []
    for clen, segs in _CONTIGS:
        contig_len.append(clen)
        for (a, b, f, ch, rp, mq) in segs:
            lead, tail = (a, clen - b) if f else (clen - b, a)  # (a reverse segment's CIGAR runs on the reversed contig)
            cigs.append([c for c in (op(lead, OP_S), op(b - a, OP_M), op(tail, OP_S)) if c >> 4])
            chrom.append(ch), pos.append(rp), fwd.append(f), mapq.append(mq), s0.append(a), s1.append(b)
        seg_off.append(len(pos))
        rev.append(acgt[rng.integers(0, 4, clen)] if any(not s[2] for s in segs) else None)
    coff = np.zeros(len(cigs) + 1, np.uint32)
    coff[1:] = np.cumsum([len(c) for c in cigs])
    return abi.IndexData(contig_len=contig_len, contig_seg_off=seg_off, seg_chrom_index=chrom, seg_pos=pos, seg_is_fwd_strand=fwd, seg_mapq=mapq,
                         seg_seq_order_start=s0, seg_seq_order_end=s1, seg_cigar_off=coff, seg_cigar=np.array(sum(cigs, []), np.uint32),
                         chrom_seq=[acgt[rng.integers(0, 4, 4000)] for _ in range(2)], rev_contig_seq=rev)


INDEX = make_index()
N_CONTIGS = len(_CONTIGS)


@dataclass
class Case:
    name: str
    batch: abi.BatchData
    verdict: int            # written by hand where the case is made, never computed
    why: str
    stages: int = abi.STAGES_ALL
    n_lane_items: Optional[int] = None   # by hand, where the case pins a class: items the lane-per-item kernel must take
    family: str = ""


class Builder:
    """segments one by one; every segment gets a read of its own whose length is its CIGAR's read span unless the caller says otherwise"""

    def __init__(self, seq_fmt=abi.SEQ_ASCII, seed=5, lead=0):
        """`lead`: ops in front of the first segment's (seg_cigar_off[0] need not be 0)"""
        self.fmt, self.rng = seq_fmt, np.random.default_rng(seed)
        self.read_rev, self.read_len, self.read_off, self.seq = [], [], [], []
        self.nbytes = 0
        self.s_read, self.s_contig, self.s_pos, self.s_fwd, self.coff, self.ops = [], [], [], [], [lead], [op(1, OP_M)] * lead

    def read(self, length, reverse=0, real=True):
        """`real` = False: a length without bases behind it (for reads no item of an accepted batch touches)"""
        self.read_rev.append(reverse), self.read_len.append(length), self.read_off.append(self.nbytes)
        n = ex.bases_needed(self.fmt, length) if real else 0
        if self.fmt == abi.SEQ_ASCII:
            self.seq.append(np.frombuffer(b"ACGT", np.uint8)[self.rng.integers(0, 4, n)])
        else:
            self.seq.append(np.frombuffer(bytes([0x11, 0x12, 0x14, 0x18, 0x21, 0x22, 0x24, 0x28, 0x41, 0x42, 0x44, 0x48, 0x81, 0x82, 0x84, 0x88]), np.uint8)[self.rng.integers(0, 16, n)])
        self.nbytes += n
        return len(self.read_len) - 1

    def seg(self, contig, pos, ops, fwd=1, read=None, read_len=None, read_rev=None):
        ops = [int(c) for c in ops]
        if read is None:
            span = ex.read_span(ops)
            real = span < (1 << 20)
            read = self.read((span if real else 0) if read_len is None else read_len, len(self.s_read) % 2 if read_rev is None else read_rev, real)
        self.s_read.append(read), self.s_contig.append(contig), self.s_pos.append(pos), self.s_fwd.append(fwd)
        self.ops += ops
        self.coff.append(len(self.ops))
        return len(self.s_read) - 1

    def residue(self, r):
        """a segment without items in front of the next one, so that the next one's first op stands at r mod 4"""
        k = (r - len(self.ops)) % 4
        if k:
            self.seg(C_NONE, 3, [op(1, OP_M)] * k)

    def batch(self, item_seg=None, item_cseg=None) -> abi.BatchData:
        return abi.BatchData(read_is_reverse=self.read_rev, read_seq_len=self.read_len, read_seq_off=self.read_off,
                             seq=np.concatenate(self.seq) if self.seq else np.zeros(0, np.uint8), seq_fmt=self.fmt, seg_read=self.s_read,
                             seg_contig=self.s_contig, seg_pos=np.array(self.s_pos, np.int64), seg_is_fwd_strand=self.s_fwd, seg_cigar_off=self.coff,
                             cigar=np.array(self.ops, np.uint32), item_seg=item_seg, item_cseg=item_cseg)


# ---- A. the CIGAR walk -------------------------------------------------------------------------------------------------------------

OP_COUNTS = (0, 1, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 97)
_PATTERN = [op(3, OP_M), op(1, OP_I), op(2, OP_M), op(2, OP_D), op(4, OP_EQ), op(1, OP_X), op(2, OP_I), op(5, OP_M), op(3, OP_N), op(2, OP_EQ),
            op(1, OP_D), op(2, OP_X), op(1, OP_M), op(4, OP_P), op(2, OP_M), op(3, OP_I)]
BIG = [op(1 << 27, OP_M)] * 7  # a neighbour's first ops: 7 x 2^27 bases, a span of its own below 2^30


def walk_ops(n, shift=0):
    return [_PATTERN[(i + shift) % len(_PATTERN)] for i in range(n)]


def _astride(b: Builder, ops):
    """a segment of C_TWO astride the border between the forward and the reverse contig segment: two items, and a wrong reference span moves
    the reverse one's start"""
    span = ex.ref_span(ops)
    return b.seg(C_TWO, 1000 - span // 2, ops)


def cases_walk():
    out = []
    b = Builder(seed=11)
    for n in OP_COUNTS:
        for r in range(4):
            b.residue(r)
            _astride(b, walk_ops(n, r))
            b.seg(C_NONE, 0, BIG)  # the vector loads of the segment in front reach into these ops
    b.seg(C_NONE, 5, [op(1, OP_M)] * 40)
    out.append(Case("A_walk_mid", b.batch(), OK, "op counts 0 .. 97 at every offset residue, each followed by a neighbour whose first ops are 2^27-base M", family="A"))
    for n in OP_COUNTS:
        for r in range(4):
            b = Builder(seed=12 + n)
            b.seg(C_NONE, 0, BIG)
            b.residue(r)
            _astride(b, walk_ops(n, r + 1))
            out.append(Case(f"A_walk_last_n{n}_r{r}", b.batch(), OK, "the same segment as the batch's last: the scalar tail", family="A"))
    # read span: equal lifts, one more or one less does not (the status is the oracle's; test_read_span_is_observed asserts the pattern)
    b = Builder(seed=13)
    for n in (5, 17, 33, 65):
        ops = walk_ops(n)
        for d in (0, 1, -1):
            b.seg(C_TWO, 100, ops, read_len=ex.read_span(ops) + d)
    out.append(Case("A_read_span", b.batch(), OK, "read_seq_len equal to the read span, one more, one less", family="A"))
    # each op code alone, with a length of its own: a wrong bit in one of the three masks changes one observable
    b = Builder(seed=14)
    for code in range(9):
        ln = 2 << code
        e = 100 * (-(-ln // 100) + 1)  # r_end if the op consumes reference: a multiple of 100 -> the contig segment that starts there is met
        for back in (0, 1):
            b.seg(C_NINE, e - ln - back, [op(ln, code)])
    for code in range(9):
        b.seg(C_TWO, 990, [op(2 << code, code)])  # ... and astride the strand border of C_TWO
    out.append(Case("A_one_op_each", b.batch(), OK, "M I D N S H P = X alone, lengths 2 .. 512; r_end on a contig segment's start and one short of it", family="A"))
    # ... and beside a match, so that the segment lifts and its read span is compared with read_seq_len: the clips in front, the others between
    b = Builder(seed=16)
    for code in range(9):
        ln = 2 << code
        b.seg(C_TWO, 300 if code % 2 else 1300, [op(ln, code), op(20, OP_M)] if code in (OP_S, OP_H) else [op(20, OP_M), op(ln, code), op(20, OP_M)])
    out.append(Case("A_one_op_beside_a_match", b.batch(), OK, "each op code with a length of its own in a segment that lifts: a read-span mask without its bit ends LEN_MISMATCH", family="A"))
    b = Builder(seed=15)
    for code in range(9):
        b.seg(C_TWO, 995, [op(5, OP_M), op(0, code), op(5, OP_M)])
        b.seg(C_TWO, 1000, [op(0, code)])
    out.append(Case("A_zero_length_ops", b.batch(), OK, "a zero-length op of each kind, between two M and alone", family="A"))
    return out


def padded_ops(total, run_at, run):
    """`total` ops: a run of `run` neighbouring match ops from position run_at, non-mergeable everywhere else (matches alternate with I and D)"""
    ops = []
    for i in range(total):
        if run_at <= i < run_at + run:
            m = True
        elif i < run_at:
            m = (run_at - 1 - i) % 2 == 1
        else:
            m = (i - run_at - run) % 2 == 1
        ops.append(op(1, (OP_M, OP_EQ, OP_X)[i % 3]) if m else op(1, (OP_I, OP_D)[(i // 2) % 2]))
    return ops


N_LIGHT_MAX = ex.LANE_MAX_W - ex.region_dwords(0, 0, 1)  # the largest merged op count of a light item on a one-block contig segment


def merge_layouts():
    """(first op of the run, its length): a pair astride every multiple of 4 up to 64, a pair astride none, runs of three across a border
    with one and with two ops in front of it"""
    lay = [(k - 1, 2) for k in range(4, 65, 4)] + [(1, 2)]
    lay += [(k - 1, 3) for k in range(4, 65, 4)] + [(k - 2, 3) for k in range(4, 65, 4)]
    return lay


def cases_merge():
    out = []
    for extra, name, lanes in ((0, "light", None), (1, "heavy", 0)):
        b = Builder(seed=21 + extra)
        for i, (at, run) in enumerate(merge_layouts()):
            ops = padded_ops(N_LIGHT_MAX + extra + run - 1, at, run)
            b.residue(i % 4)
            b.seg(C_TWO, 100 if i % 2 else 1100, ops)  # (forward and reverse contig segment in turn)
        n = len(merge_layouts())
        out.append(Case(f"A_merge_{name}", b.batch(), OK,
                        f"merged op count exactly {N_LIGHT_MAX + extra}: region lane_max_w{' + 1' if extra else ''}; a carry lost or doubled at a border moves the item to the other class",
                        n_lane_items=n if lanes is None else lanes, family="A"))
    return out


# ---- B. the overlap rule -------------------------------------------------------------------------------------------------------------

def cases_overlap():
    b = Builder(seed=31)
    for contig in (C_ONE, C_TWO, C_THREE, C_FIVE, C_NINE):
        clen, segs = _CONTIGS[contig]
        for k in sorted({0, len(segs) // 2, len(segs) - 1}):
            cs, ce = segs[k][0], segs[k][1]
            for e in (cs - 1, cs, cs + 1):  # r_end
                if e >= 0:
                    span = min(10, e)
                    b.seg(contig, e - span, [op(span, OP_M)] if span else [op(5, OP_I)])
            b.seg(contig, ce - 1, [op(1, OP_M)])   # r_start one inside (on the contig's last segment r_end is the contig's length)
            b.seg(contig, ce, [op(5, OP_I)])       # r_start at the end: not met
            for p in (cs, ce):                     # span 0 standing at cs and at ce
                b.seg(contig, p, [op(5, OP_I)])
                b.seg(contig, p, [op(7, OP_S)])
    b.seg(C_NONE, 500, [op(50, OP_M)])            # a contig the index never saw
    rd = b.read(20)
    for contig, pos in ((C_TWO, 990), (C_THREE, 290), (C_NINE, 395)):  # one read, three segments on different contigs
        b.seg(contig, pos, [op(20, OP_M)], read=rd, fwd=contig % 2)
    b.seg(C_NINE, 150, [op(500, OP_M)])           # items come out in contig-segment order: segments 1 .. 6
    b.seg(C_FIVE, 0, [op(1000, OP_EQ)])           # all five
    b.seg(C_THREE, 600, [op(99, OP_M)])           # in the gap: r_end one short of the last segment
    b.seg(C_THREE, 600, [op(100, OP_M)])          # ... and on its start
    return [Case("B_overlap", b.batch(), OK, "r_end at cs - 1, cs, cs + 1 and r_start at ce - 1, ce against first, middle and last segments of contigs with 0 .. 9 segments", family="B")]


# ---- C. the verdict --------------------------------------------------------------------------------------------------------------------

N_BASE = 129


def base_batch(n, fmt=abi.SEQ_ASCII, seed=41):
    """n good segments (light items on C_TWO, both strands); the refusals replace one of them"""
    b = Builder(fmt, seed)
    for s in range(n):
        b.seg(C_TWO, 100 + 7 * s if s % 2 else 1100 + 5 * s, [op(10, OP_M), op(2, OP_I), op(6 + s % 5, OP_M)])
    return b


PLACES = (("only", 1, 0), ("first", N_BASE, 0), ("middle", N_BASE, 64), ("last", N_BASE, N_BASE - 1))


def _with_segment(n, at, contig, pos, ops, fmt=abi.SEQ_ASCII, read_len=None, lead=0):
    """base_batch(n) with segment `at` replaced"""
    b = Builder(fmt, 41, lead)
    for s in range(n):
        if s == at:
            b.seg(contig, pos, ops, read_len=read_len)
        else:
            b.seg(C_TWO, 100 + 7 * s if s % 2 else 1100 + 5 * s, [op(10, OP_M), op(2, OP_I), op(6 + s % 5, OP_M)])
    return b


def span_ops(last):
    """31 ops: five reference-consuming ones below 2^28 at 0, 5, 17, 21, 30 -- four of 2^28 - 1 and `last` -- with 1-base insertions between, so
    that every half of a lane group carries part of the sum"""
    ops = [op(1, OP_I)] * 31
    for at, code in ((0, OP_M), (5, OP_D), (17, OP_N), (21, OP_EQ)):
        ops[at] = op((1 << 28) - 1, code)
    ops[30] = op(last, OP_X)
    return ops


def code_ops(code, at, n=33):
    ops = walk_ops(n)
    ops[at] = op(1, code)
    return ops


def cases_verdict():
    """Every line a last accepted and a first refused case, each refusal over PLACES: as the only segment of a batch of one, and as the first,
    a middle and the last of 129.  Three refusals cannot take every placement:
      coff_behind_the_batch   first and middle only: the last entry of seg_cigar_off IS seg_cigar_off[n_segs] (and a batch of one has no other)
      coff_2p31               the last entry only: 2^31 anywhere else is above seg_cigar_off[n_segs] or above its successor, an index fault
      index_beats_range       129 segments only: two faults in different segments need two segments"""
    out = []

    def add(name, batch, verdict, why, **kw):
        out.append(Case("C_" + name, batch, verdict, why, family="C", **kw))

    for place, n, at in PLACES:
        # seg_pos
        add(f"pos_7ffffff0_{place}", _with_segment(n, at, C_NONE, 0x7FFFFFF0, [op(5, OP_M)]).batch(), OK, "last accepted seg_pos")
        add(f"pos_7ffffff1_{place}", _with_segment(n, at, C_NONE, 0x7FFFFFF1, [op(5, OP_M)]).batch(), RANGE, "first refused seg_pos")
        add(f"pos_0_{place}", _with_segment(n, at, C_TWO, 0, [op(5, OP_M)]).batch(), OK, "seg_pos 0")
        add(f"pos_minus1_{place}", _with_segment(n, at, C_TWO, -1, [op(5, OP_M)]).batch(), RANGE, "seg_pos -1")
        # span
        add(f"span_2p30m1_{place}", _with_segment(n, at, C_NONE, 7, span_ops(3)).batch(), OK, "a span of 2^30 - 1 from five ops below 2^28")
        add(f"span_2p30_{place}", _with_segment(n, at, C_NONE, 7, span_ops(4)).batch(), RANGE, "a span of 2^30")
        # seg_contig, seg_read
        add(f"contig_last_{place}", _with_segment(n, at, N_CONTIGS - 1, 10, [op(5, OP_M)]).batch(), OK, "seg_contig n_contigs - 1")
        bad = _with_segment(n, at, N_CONTIGS - 1, 10, [op(5, OP_M)]).batch()
        bad.seg_contig[at] = N_CONTIGS
        add(f"contig_n_{place}", bad, INVALID_ARG, "seg_contig n_contigs")
        bad = base_batch(n).batch()
        bad.seg_read[at] = n - 1
        add(f"read_last_{place}", bad, OK, "seg_read n_reads - 1 (the length check sees another read's length)")
        bad = base_batch(n).batch()
        bad.seg_read[at] = n
        add(f"read_n_{place}", bad, INVALID_ARG, "seg_read n_reads")
        # seg_cigar_off[s + 1] against seg_cigar_off[s] (two unused ops in front of the batch's, so that the first offset has a value below it)
        add(f"coff_equal_{place}", _with_segment(n, at, C_TWO, 300, [], lead=2).batch(), OK, "seg_cigar_off[s + 1] == seg_cigar_off[s]: a segment without ops")
        b = _with_segment(n, at, C_TWO, 300, [], lead=2).batch()
        b.seg_cigar_off[at + 1] -= 1
        add(f"coff_below_{place}", b, INVALID_ARG, "seg_cigar_off[s + 1] one below seg_cigar_off[s]")
    # a seg_cigar_off entry above seg_cigar_off[n_segs]: the first and a middle segment would end behind the batch's ops.  (No batch of one
    # segment and no last segment: the last entry IS seg_cigar_off[n_segs].)
    for place, n, at in PLACES[1:3]:
        b = base_batch(n).batch()
        b.seg_cigar_off[at + 1] = int(b.seg_cigar_off[n]) + 2
        add(f"coff_behind_the_batch_{place}", b, INVALID_ARG, "seg_cigar_off[s + 1] above seg_cigar_off[n_segs]")
    # seg_cigar_off[n_segs] = 2^31 (the last segment only: any other entry that high is above or below a neighbour, an index fault)
    b = base_batch(3).batch()
    b.seg_cigar_off[3] = 0x80000000
    add("coff_2p31", b, RANGE, "seg_cigar_off[n_segs] = 2^31: more ops than an int addresses (none is read)")
    add("span_2p30m1_beside_clips", _with_segment(N_BASE, 64, C_NONE, 7, span_ops(3) + [op((1 << 28) - 1, c) for c in (OP_I, OP_S, OP_I)]).batch(), OK,
        "a span of 2^30 - 1 beside 3 x (2^28 - 1) of I and S, which do not count")
    # op codes: 8 accepted, 9 and 15 refused; first, at 15, 16, 31, 32 = last; in the vector path (a segment with ops behind it) and in the
    # tail (the batch's last segment, the only one)
    for at_op in (0, 15, 16, 31, 32):
        for place, n, at in PLACES:
            add(f"code8_op{at_op}_{place}", _with_segment(n, at, C_TWO, 300, code_ops(OP_P, at_op)).batch(), OK, "op code 8")
            for code in (9, 15):
                add(f"code{code}_op{at_op}_{place}", _with_segment(n, at, C_TWO, 300, code_ops(code, at_op)).batch(), RANGE, f"op code {code}")
    # bases: read_seq_off + need against seq_bytes.  The read whose bases end with the buffer is the last one; segment `at` is its segment
    for fmt, name, ln in ((abi.SEQ_ASCII, "ascii", 18), (abi.SEQ_BAM4, "bam4_even", 18), (abi.SEQ_BAM4, "bam4_odd", 17), (abi.SEQ_BAM4_SPARSE, "sparse", 1500)):
        for place, n, at in PLACES:
            def last_read(extra):
                # `extra`: bases added to the last read's declared length (sparse: a granule)
                bb = Builder(fmt, 43)
                for s in range(n):
                    if fmt == abi.SEQ_BAM4_SPARSE:
                        bb.read(ln, s % 2)
                        bb.seg(C_NONE, 10, [op(ln, OP_M)], read=s)
                    else:
                        bb.seg(C_TWO, 100 + s, [op(ln, OP_M)])
                bt = bb.batch()
                bt.seg_read[at], bt.seg_read[n - 1] = n - 1, at  # (all reads are of one length)
                bt.read_seq_len[n - 1] += extra
                return bt
            step = 1024 if fmt == abi.SEQ_BAM4_SPARSE else 2 if fmt == abi.SEQ_BAM4 else 1
            fit = last_read(0)
            assert int(fit.read_seq_off[n - 1]) + ex.bases_needed(fmt, int(fit.read_seq_len[n - 1])) == fit.seq.nbytes and int(fit.seg_read[at]) == n - 1
            add(f"bases_fit_{name}_{place}", fit, OK, "read_seq_off + need == seq_bytes")
            add(f"bases_past_{name}_{place}", last_read(step), INVALID_ARG, "one byte of bases past seq_bytes")
    for place, n, at in PLACES:
        for extra, verdict, name in ((0, OK, "bases_off_at_end_len0"), (1, INVALID_ARG, "bases_off_past_end")):
            b = _with_segment(n, at, C_TWO, 300, []).batch()  # (a segment without ops, a read without bases)
            assert int(b.read_seq_len[at]) == 0
            b.read_seq_off[at] = b.seq.nbytes + extra
            add(f"{name}_{place}", b, verdict, "read_seq_off == seq_bytes with length 0 / read_seq_off == seq_bytes + 1")
        # sparse header of segment `at`'s read at a multiple of 16 / 8 bytes further (the reads behind it stand at multiples of 16 again)
        for off, verdict in ((16, OK), (8, INVALID_ARG)):
            bb = Builder(abi.SEQ_BAM4_SPARSE, 44)
            for s in range(n):
                if s == at:
                    bb.seq.append(np.zeros(off, np.uint8))
                    bb.nbytes += off
                bb.seg(C_NONE, 10, [op(900, OP_M)])
                if s == at:
                    bb.seq.append(np.zeros(16 - off, np.uint8))
                    bb.nbytes += 16 - off
            b = bb.batch()
            assert int(b.read_seq_off[at]) % 16 == off % 16 and all(int(o) % 16 == 0 for k, o in enumerate(b.read_seq_off) if k != at)
            add(f"sparse_offset_{off}_{place}", b, verdict, "sparse header at a multiple of 16 / at 8")
    # an index fault and a range fault in different segments (two segments at least: no batch of one): the index fault in the first, a middle
    # and the last segment, the range fault behind it or in front of it
    for place, idx_at, rng_at in (("first", 0, 100), ("middle", 64, 20), ("last", N_BASE - 1, 20)):
        b = _with_segment(N_BASE, rng_at, C_NONE, 0x7FFFFFF1, [op(5, OP_M)]).batch()
        if place == "middle":
            b.seg_read[idx_at] = N_BASE
        else:
            b.seg_contig[idx_at] = N_CONTIGS
        add(f"index_beats_range_{place}", b, INVALID_ARG, f"seg_pos out of range in segment {rng_at}, an index out of range in segment {idx_at}")
    # explicit lists: the item in question as the only, the first, a middle and the last of its list
    for place, n, at in PLACES:
        segs = [0] if n == 1 else [0, 5, 64, 100, N_BASE - 1]
        j = {"only": 0, "first": 0, "middle": 2, "last": len(segs) - 1}[place]
        for seg_j, cseg_j, verdict, name in ((n - 1, 1, OK, "last_accepted"), (n, 1, INVALID_ARG, "item_seg_n_segs"), (n - 1, 2, INVALID_ARG, "item_cseg_past_the_contig")):
            b = base_batch(n).batch()
            item_seg, item_cseg = list(segs), [k % 2 for k in range(len(segs))]
            item_seg[j], item_cseg[j] = seg_j, cseg_j
            b.item_seg, b.item_cseg = np.array(item_seg, np.uint32), np.array(item_cseg, np.uint32)
            add(f"explicit_{name}_{place}", b, verdict, "item_seg at n_segs - 1 / n_segs, item_cseg at the contig's last segment / one past it")
    return out


def case_read_span_wraps():
    """17 S ops of 2^28 - 1 around 10M: the read span is above 2^32; a read whose length is the span mod 2^32 must not pass the length check"""
    ops = [op((1 << 28) - 1, OP_S)] * 8 + [op(10, OP_M)] + [op((1 << 28) - 1, OP_S)] * 9
    span = 17 * ((1 << 28) - 1) + 10
    ln = span % (1 << 32)
    b = Builder(abi.SEQ_BAM4, 45)
    b.seg(C_TWO, 100, [op(30, OP_M)])
    rd = b.read(0, 0)
    b.read_len[rd] = ln
    b.seq.append(np.zeros((ln + 1) // 2, np.uint8))  # (never touched: no stage that reads bases runs)
    b.nbytes += (ln + 1) // 2
    b.seg(C_TWO, 200, ops, read=rd)
    return Case("C_read_span_wraps", b.batch(), OK, "read span above 2^32 with read_seq_len = span mod 2^32: LEN_MISMATCH, not LIFTED",
                stages=abi.STAGES_ALL & ~(abi.STAGE_SIMPLIFY | abi.STAGE_LSHIFT), family="C")


# ---- D. counts, scans and class order --------------------------------------------------------------------------------------------------

SCAN_SIZES = (1, 7, 8, 9, 2047, 2048, 2049, 4097)   # either side of SCAN_PER_THREAD (8) and SCAN_BLOCK (2048), and two blocks + 1
CLASS_SIZES = (2047, 2048, 2049, 4095, 4096, 4097)  # either side of CLS_BLOCK (2048) and of two of them


def case_scan(n):
    """one-op segments on C_NINE with 0 .. 3 items each by a fixed pattern; light items only"""
    b = Builder(seed=51)
    for s in range(n):
        k = (5 * s + s // 8) % 4
        if k == 0:
            b.seg(C_NONE, 10, [op(10, OP_M)])
        else:
            j = s % 6  # items on contig segments j .. j + k - 1
            b.seg(C_NINE, 100 * j + 95 if k > 1 else 100 * j + 10, [op(10 if k < 3 else 110, OP_M)])
    return Case(f"D_scan_{n}", b.batch(), OK, "item offsets across the scan's borders; light items only (the one-round-trip path)", family="D")


HEAVY_OPS = padded_ops(N_LIGHT_MAX + 2, 1, 2)  # merged count one above the light maximum


def case_classes(n, light_only=False):
    """n segments with one item each; the four classes (strand x light / heavy) item by item"""
    b = Builder(seed=52)
    light = [op(10, OP_M), op(1, OP_D), op(9, OP_M)]
    for s in range(n):
        heavy = (s % 4) >= 2 and not light_only
        b.seg(C_TWO, (100 if s % 2 == 0 else 1100) + s % 50, HEAVY_OPS if heavy else light)
    lanes = n if light_only else (n + 3) // 4 + (n + 2) // 4
    return Case(f"D_classes_{n}{'_light' if light_only else ''}", b.batch(), OK, "class order across CLS_BLOCK borders", n_lane_items=lanes, family="D")


# ---- E. read segments that leave their contig -----------------------------------------------------------------------------------------

def cases_leaving():
    """the fuzz keeps reads inside their contigs on purpose; these do not.  One case each, so that each can be kept from the card by name."""
    out = []
    for name, contig, pos, ops, verdict, why in (
            ("E_end_on_contig_end", C_TWO, 1990, [op(10, OP_M)], OK, "r_end == contig_len on a reverse segment: rev_pos 0"),
            ("E_end_on_contig_end_indels", C_TWO, 1980, [op(8, OP_M), op(2, OP_D), op(2, OP_I), op(10, OP_M)], OK, "the same with indels for the left shift"),
            ("E_one_past_contig_end", C_TWO, 1991, [op(10, OP_M)], RANGE, "r_end == contig_len + 1 on a reverse segment: rev_pos -1"),
            ("E_one_past_contig_end_indels", C_TWO, 1981, [op(8, OP_M), op(2, OP_D), op(2, OP_I), op(10, OP_M)], RANGE, "rev_pos -1 with indels for the left shift"),
            ("E_far_past_contig_end", C_TWO, 1995, [op(5, OP_M), op(3, OP_I), op(300, OP_M)], RANGE, "most of the segment behind the contig's end: rev_pos -300"),
            ("E_past_end_forward_segment", C_THREE, 995, [op(5, OP_M), op(3, OP_I), op(30, OP_M)], OK, "behind the contig's end on a forward segment: no rev_pos, lifted as the oracle lifts it"),
            ("E_wholly_behind", C_TWO, 2000, [op(10, OP_M)], OK, "r_start == contig_len: no contig segment is met"),
            ("E_wholly_behind_far", C_TWO, 2500, [op(10, OP_M), op(2, OP_D), op(5, OP_M)], OK, "the whole segment 500 behind the contig's end")):
        b = Builder(seed=61)
        b.seg(C_TWO, 50, [op(20, OP_M)])
        b.seg(contig, pos, ops)
        b.seg(C_TWO, 1500, [op(20, OP_M)])
        out.append(Case(name, b.batch(), verdict, why, family="E"))
        if name in ("E_end_on_contig_end", "E_one_past_contig_end"):  # ... and as an explicit list (k_item_desc)
            out.append(Case(name + "_explicit", b.batch(np.array([0, 1, 2], np.uint32), np.array([0, 1, 1], np.uint32)), verdict, why + ", items listed by the caller", family="E"))
    return out


def accepted_small():
    """every accepted case the three voices compare (families A, B, C, E and the small sizes of D)"""
    return [c for c in cases_walk() + cases_merge() + cases_overlap() + cases_verdict() if c.verdict == OK] + [case_read_span_wraps()]


def refused():
    return [c for c in cases_verdict() + cases_leaving() if c.verdict != OK]
