"""Hand-built batches for the finishing and SA stages: reads and lift items given one by one, bases and qualities placed at chosen byte
offsets inside larger buffers of random bytes.  What tests/test_finish_edges.py and tests/emu_finish_lib.py run.  TEST INFRASTRUCTURE ONLY."""
from dataclasses import dataclass

import numpy as np

from portello_amd import abi
from test_records_dev import hand_lift

L_, NOLIFT, MISMATCH, PANIC, NEED = abi.ITEM_LIFTED, abi.ITEM_NO_LIFTOVER, abi.ITEM_LEN_MISMATCH, abi.ITEM_PANIC, abi.ITEM_NEED_BASES

# The placement grid.  The pads bracket the constants of revcomp_record (finish_core.hpp): a fast chunk wants 4 bytes in front of its
# window, 8 (qualities, several chunks), 24 (qualities, one chunk) or 28 (bases) bytes from its window's start to the buffer's end.
GRID_L = list(range(100)) + [127, 128, 129, 255, 256, 257, 1000]
LONG_L = 100_003
FRONTS = (0, 1, 2, 3, 4, 5, 8, 17)
TAILS = (0, 1, 7, 8, 9, 19, 23, 24, 25, 27, 28, 29)
GAPS = (0, 1, 3, 13)
SHIFTS = (0, 1, 2, 3)
THREADS = (1, 7, 64, 256)  # 256: the device's


@dataclass
class Case:
    batch: abi.BatchData
    flags: np.ndarray
    qual: np.ndarray
    qoff: np.ndarray
    lift: abi.BatchResult
    name: str = ""

    def fin(self):
        return self.batch, self.flags, self.qual, self.qoff, self.lift


def M(n):
    return (int(n) << 4) | 0


def pack_bam4(codes, rng):
    """nibble codes -> bytes; the low nibble behind an odd read is random"""
    c = np.asarray(codes, np.uint8)
    if len(c) & 1:
        c = np.concatenate([c, rng.integers(0, 16, 1, dtype=np.uint8)])
    return ((c[0::2] << 4) | c[1::2]).astype(np.uint8)


def build(reads, items, seq_fmt=abi.SEQ_BAM4, front=0, gap=0, tail=0, shift=0, one_buffer=False, seed=0, name="", segs=None):
    """reads: (length, source flag, bases or None, qualities or None) -- bases are nibble codes (BAM4) or bytes (ASCII), None: random.
    items: (read, status, flip, mapq, chrom, pos, ops) in item order, reads ascending; every item gets a read segment of its own.
    segs (instead of items, for a batch that a real lift takes): (read, contig, pos, is_fwd_strand, ops) per read segment; lift is None.
    Placement: `front` bytes in front of the first read, `gap` between reads, `tail` behind the last one, all random; `shift`: the
    buffers are views that start `shift` bytes into a larger array.  one_buffer: bases and qualities of a read follow each other in ONE
    buffer (batch.seq and qual are the same view), as on the raw-window route."""
    rng = np.random.default_rng(seed)
    seqs, quals = [], []
    for L, _, bases, q in reads:
        if bases is None:
            bases = rng.integers(0, 16, L, dtype=np.uint8) if seq_fmt == abi.SEQ_BAM4 else rng.choice(np.frombuffer(b"ACGTNacgtnRY=*", np.uint8), L)
        bases = np.asarray(bases, np.uint8)
        assert len(bases) == L
        seqs.append(pack_bam4(bases, rng) if seq_fmt == abi.SEQ_BAM4 else bases)
        q = rng.integers(0, 256, L, dtype=np.uint8) if q is None else np.asarray(q, np.uint8)
        assert len(q) == L
        quals.append(q)
    n = len(reads)

    def place(parts_per_read):
        """-> (view, offsets[k][j] of part j of read k)"""
        total = front + tail + gap * max(0, n - 1) + sum(len(p) for parts in parts_per_read for p in parts)
        big = rng.integers(0, 256, shift + total, dtype=np.uint8)
        view = big[shift:]
        assert big.ctypes.data % 4 == 0 or total + shift == 0  # so the view's address mod 4 is `shift`
        at, offs = front, []
        for k, parts in enumerate(parts_per_read):
            o = []
            for p in parts:
                view[at:at + len(p)] = p
                o.append(at)
                at += len(p)
            offs.append(o)
            if k + 1 < n:
                at += gap
        assert at + tail == total
        return view, offs

    if one_buffer:
        view, offs = place([[s, q] for s, q in zip(seqs, quals)])
        seq = qual = view
        soff, qoff = [o[0] for o in offs], [o[1] for o in offs]
    else:
        seq, so = place([[s] for s in seqs])
        qual, qo = place([[q] for q in quals])
        soff, qoff = [o[0] for o in so], [o[0] for o in qo]
    flags = np.array([r[1] for r in reads], np.uint16)
    if segs is not None:
        assert all(segs[i][0] <= segs[i + 1][0] for i in range(len(segs) - 1))
        coff = np.zeros(len(segs) + 1, np.uint32)
        coff[1:] = np.cumsum([len(s[4]) for s in segs])
        batch = abi.BatchData(read_is_reverse=(flags >> 4) & 1, read_seq_len=[r[0] for r in reads], read_seq_off=np.array(soff, np.uint64), seq=seq, seq_fmt=seq_fmt,
                              seg_read=[s[0] for s in segs], seg_contig=[s[1] for s in segs], seg_pos=[s[2] for s in segs], seg_is_fwd_strand=[s[3] for s in segs],
                              seg_cigar_off=coff, cigar=np.concatenate([np.asarray(s[4], np.uint32) for s in segs]) if segs else np.zeros(0, np.uint32))
        assert batch.seq.ctypes.data == seq.ctypes.data
        return Case(batch, flags, qual, np.array(qoff, np.uint64), None, name)
    ni = len(items)
    assert all(items[i][0] <= items[i + 1][0] for i in range(ni - 1))
    batch = abi.BatchData(read_is_reverse=(flags >> 4) & 1, read_seq_len=[r[0] for r in reads], read_seq_off=np.array(soff, np.uint64), seq=seq, seq_fmt=seq_fmt,
                          seg_read=[it[0] for it in items], seg_contig=np.zeros(ni), seg_pos=np.zeros(ni), seg_is_fwd_strand=np.ones(ni),
                          seg_cigar_off=np.zeros(ni + 1), cigar=np.zeros(0, np.uint32))
    assert batch.seq.ctypes.data == seq.ctypes.data  # a view, no copy: the address mod 4 is the one asked for
    lift = hand_lift([(i, 0) + tuple(it[1:]) for i, it in enumerate(items)])
    return Case(batch, flags, qual, np.array(qoff, np.uint64), lift, name)


def one_read(L, seq_fmt, front, tail, shift, seed=0, one_buffer=False):
    """a batch of one read of L bases with one flipped lifted record"""
    return build([(L, 0x0, None, None)], [(0, L_, 1, 30, 0, 100, [M(L)] if L else [])], seq_fmt, front, 0, tail, shift, one_buffer, seed,
                 "L%d f%d t%d s%d" % (L, front, tail, shift))


def packed(lengths, seq_fmt, front=0, tail=0, shift=0, gap=0, seed=0, one_buffer=False):
    """reads of the given lengths back to back: even reads get a flipped record, every third read a second, unflipped one; odd reads have
    no item and a reverse source flag, so that their unmapped copy is the flipped entry"""
    reads, items = [], []
    for r, L in enumerate(lengths):
        if r & 1:
            reads.append((L, 0x10 | (0x400 if r % 4 == 1 else 0), None, None))
        else:
            reads.append((L, 0x1, None, None))
            items.append((r, L_, 1, 20 + r % 7, r % 2, 1000 + r, [M(L)] if L else []))
            if r % 3 == 0:
                items.append((r, L_, 0, 20, 1, 5000 + r, [M(L)] if L else []))
    return build(reads, items, seq_fmt, front, gap, tail, shift, one_buffer, seed, "packed n%d f%d t%d s%d g%d" % (len(lengths), front, tail, shift, gap))


def grid_cases(seq_fmt, lengths=GRID_L, fronts=FRONTS, tails=TAILS, shifts=SHIFTS):
    """the single-read placement grid, in a fixed order (the thread counts are dealt over it in that order)"""
    k = 0
    for L in lengths:
        for fr in fronts:
            for tl in tails:
                for sh in shifts:
                    yield k, one_read(L, seq_fmt, fr, tl, sh, seed=k)
                    k += 1


def gap_cases(seq_fmt):
    """three reads of one length with 0, 1, 3 or 13 bytes between them"""
    k = 0
    for L in GRID_L:
        for gap in GAPS:
            for sh in SHIFTS:
                fr, tl = FRONTS[k % len(FRONTS)], TAILS[k % len(TAILS)]
                yield k, packed([L, L, L], seq_fmt, fr, tl, sh, gap, seed=1000 + k)
                k += 1


def packed_cases(seq_fmt, with_zero=True):
    """all lengths back to back, ascending and descending: the offsets take every residue mod 4 and mod 16 and both parities, and short
    reads sit at both buffer ends"""
    ls = [L for L in GRID_L if with_zero or L]
    for shift in SHIFTS:
        yield packed(ls, seq_fmt, shift=shift, seed=40 + shift)
        yield packed(ls[::-1], seq_fmt, shift=shift, seed=50 + shift)


# ---- item rows ---------------------------------------------------------------------------------------------------------------------------

BIG = (1 << 28) - 1
EDGES = (1 << 14, 1 << 17, 1 << 20, 1 << 23, 1 << 26)


def end_bin_case():
    """item_ref_end and the bin: every op code with lengths 0, 1 and 2^28 - 1; pos / end around every bin level; end == pos; long CIGARs"""
    items = []
    for op in range(16):
        for ln in (0, 1, BIG):
            items.append((0, L_, 0, 10, 0, 77, [(ln << 4) | op]))
    for e in EDGES:
        for pos, ln in ((e - 1, 1), (e - 1, 2), (e, 1), (e - 2, 2), (e - 2, 1), (e - 5, 10), (0, e), (0, e + 1), (e, 0), (e - 1, 0), (e + 1, 0)):
            items.append((0, L_, 0, 10, 0, pos, [M(ln)] if ln else []))
            items.append((0, L_, 0, 10, 0, pos, [(3 << 4) | 4, (ln << 4) | 7, (2 << 4) | 1] if ln else [(5 << 4) | 4]))
    for pos, ops in ((0, []), (0, [M(0)]), (5, []), ((1 << 29) - 1, [M(1)]), ((1 << 29) - BIG, [M(BIG)]), (0, [M(BIG), (BIG << 4) | 2]), ((1 << 29) - 2, [(2 << 4) | 8]),
                     (12345, [M(1)] * 64), (12345, [M(1), (1 << 4) | 2] * 32 + [(1 << 4) | 3]), (16000, [(2 << 4) | 7, (1 << 4) | 1] * 35_000)):
        items.append((0, L_, 0, 10, 0, pos, ops))
    return build([(10, 0, None, None)], items, seed=3, name="end_bin")


FLAG_BITS = (0x1, 0x10, 0x40, 0x80, 0x100, 0x400, 0x800)


def flag_case(seq_fmt=abi.SEQ_BAM4):
    """every pattern of the source bits, each on three reads: a record that is not flipped, a flipped one (both primaries, so a source
    0x800 must go), and no record at all (the unmapped copy); then the same patterns on supplementary records"""
    reads, items = [], []
    for pat in range(1 << len(FLAG_BITS)):
        fl = sum(b for k, b in enumerate(FLAG_BITS) if pat >> k & 1)
        L = 1 + pat % 37
        for kind in range(4):
            r = len(reads)
            reads.append((L, fl, None, None))
            if kind < 2:
                items.append((r, L_, kind, 30, 0, 10 + r, [M(L)]))
            elif kind == 3:  # primary first, then a flipped and an unflipped supplementary record
                items.append((r, L_, 0, 40, 0, 10 + r, [M(L)]))
                items.append((r, L_, 1, 30, 0, 10 + r, [M(L)]))
                items.append((r, L_, 0, 30, 0, 10 + r, [M(L)]))
    return build(reads, items, seq_fmt, seed=4, name="flags")


def primary_case():
    """the MAPQ rows, a non-lifted item with the highest MAPQ between lifted ones (each status in turn), reads without a lifted item at
    the first, middle and last read and several in a row, a read with 70 items"""
    rows = [None, [(L_, 60), (L_, 60)], [(L_, 7), (L_, 60), (L_, 60)], [(L_, 0), (L_, 0), (L_, 0)], [(L_, 255), (L_, 0)], [(L_, 0), (L_, 255)]]
    for st in (NOLIFT, MISMATCH, PANIC, NEED):
        rows.append([(L_, 10), (st, 200), (L_, 10), (L_, 11)])
        rows.append([(st, 200), (L_, 5)])
        rows.append([(L_, 5), (st, 200)])
    rows += [None, None, [(NOLIFT, 9)], [(NOLIFT, 9), (MISMATCH, 99)], None]
    rows.append([(L_, 1 + (k * 37) % 250) if k % 5 else (NOLIFT, 255) for k in range(70)])
    rows += [[(L_, 3)], None]
    reads, items = [], []
    for r, row in enumerate(rows):
        reads.append((5 + r, 0x10 if r % 2 else 0, None, None))
        for k, (st, mq) in enumerate(row or []):
            items.append((r, st, (r + k) & 1, mq, k % 2, 100 * r + k, [M(5 + r)]))
    return build(reads, items, seed=5, name="primary")


def fault_case(statuses):
    reads = [(8, 0, None, None) for _ in statuses]
    items = [(r, st, 0, 10, 0, 50, [M(8)]) for r, st in enumerate(statuses)]
    return build(reads, items, seed=6, name="fault")


def empty_cases():
    yield build([], [], name="no reads")
    yield build([(5, 0x10, None, None), (0, 0x10, None, None), (6, 0, None, None)], [], name="no items")


# ---- SA rows ---------------------------------------------------------------------------------------------------------------------------------

SA_NAMES = ["1", "chr2", "x" * 40, "chrUn_last"]
SA_POS = (8, 9, 98, 99, 999_998, 999_999, 1 << 31)
SA_MAPQ = (0, 9, 10, 99, 100, 255)
SA_LEN = (9, 10, 99_999_999, BIG)


def sa_case():
    """the widths of every decimal field, all ten op letters, CIGARs of 0, 1, 65 and 70 000 ops, labels of 1 and 40 bytes, the first and
    the last chromosome, reads of 1, 2, 3 and 5 lifted records, unlifted records between lifted ones, the strand behind the flip"""
    ten = [((k + 1) << 4) | k for k in range(10)]
    reads, items = [], []

    def read(flag, row):
        r = len(reads)
        reads.append((4, flag, None, None))
        for st, flip, mq, chrom, pos, ops in row:
            items.append((r, st, flip, mq, chrom, pos, ops))

    read(0x0, [(L_, 0, 60, 0, 8, ten)])                                                     # one record: no tag
    read(0x0, [(L_, 0, 0, 0, 8, [M(9)]), (L_, 1, 9, 3, 9, [M(10)])])                        # strand: forward read, flipped record -> '-'
    read(0x10, [(L_, 0, 10, 2, 98, [M(99_999_999)]), (L_, 1, 99, 1, 99, [M(BIG)]), (L_, 0, 100, 0, 999_998, ten)])   # reverse read: flipped -> '+'
    read(0x10, [(L_, 1, 255, 3, 999_999, []), (L_, 0, 0, 0, 1 << 31, [M(1)]), (L_, 1, 9, 2, 0, [M(1), (1 << 4) | 1] * 32 + [M(2)]),
                (L_, 0, 10, 1, 9, ten[::-1]), (L_, 1, 100, 3, 99, [(2 << 4) | 7, (1 << 4) | 1] * 35_000)])   # five records; 0, 1, 65 and 70 000 ops
    read(0x0, [(NOLIFT, 0, 200, 0, 5, [M(4)]), (L_, 0, 7, 0, 98, [M(4)]), (NOLIFT, 1, 200, 1, 5, [M(4)]), (L_, 1, 7, 3, 8, [M(4)])])   # 4 items, 2 lifted
    read(0x0, [(NOLIFT, 0, 1, 0, 5, [M(4)]), (L_, 0, 7, 0, 98, [M(4)])])                    # 2 items, 1 lifted: no tag
    read(0x10, [])                                                                            # no item
    for k, pos in enumerate(SA_POS):
        read(0x0, [(L_, k & 1, SA_MAPQ[k % 6], k % 4, pos, [(SA_LEN[k % 4] << 4) | (k % 10)]), (L_, 0, SA_MAPQ[(k + 3) % 6], (k + 1) % 4, pos, [(SA_LEN[(k + 1) % 4] << 4) | ((k + 5) % 10)])])
    return build(reads, items, seed=7, name="sa")


# ---- batches for a real lift (the GPU tests: plo_finish_batch_dev works on the context's own lift) --------------------------------------------
# One contig whose stretches map 1:1 ('=') onto N-filled chromosomes, each with a strand and a MAPQ of its own; [130000, 140000) is
# covered by no segment; segment G carries 200 inserted contig bases at 1000 (a read inside them has no liftover).

LIFT_NAMES = SA_NAMES
LIFT_CHROM_LEN = (125_100, 40_000, 1_010_100, 40_000)
LIFT_CONTIG_LEN = 200_000
#            start    end      fwd mapq chrom pos
LIFT_SEGS = {"A": (0, 110_000, 1, 60, 0, 8),
             "B": (110_000, 120_000, 0, 60, 1, 50),
             "C": (120_000, 130_000, 1, 7, 2, 999_990),
             "D": (140_000, 150_000, 1, 0, 3, 30_000),
             "E": (150_000, 160_000, 0, 0, 0, 115_000),
             "F": (160_000, 170_000, 1, 0, 1, 12_000),
             "G": (170_000, 180_000, 1, 255, 3, 12_000),
             "H": (180_000, 182_000, 1, 9, 3, 90),
             "I": (182_000, 184_000, 0, 10, 3, 3_000),
             "J": (184_000, 186_000, 1, 99, 3, 6_000),
             "K": (186_000, 188_000, 1, 100, 3, 9_000)}
LIFT_GAP = 130_000
INS_SEG, INS_AT, INS_LEN = "G", 1000, 200


def lift_index():
    from portello_amd import cigar as cg

    order = sorted(LIFT_SEGS, key=lambda k: LIFT_SEGS[k][0])
    cigs = []
    for k, name in enumerate(order):
        a, b, fwd, _, chrom, pos = LIFT_SEGS[name]
        assert 0 <= pos and pos + (b - a) <= LIFT_CHROM_LEN[chrom] and b <= LIFT_CONTIG_LEN  # every segment lies inside its chromosome
        lead, trail = (a, LIFT_CONTIG_LEN - b) if fwd else (LIFT_CONTIG_LEN - b, a)
        body = f"{b - a}=" if name != INS_SEG else f"{INS_AT}={INS_LEN}I{b - a - INS_AT - INS_LEN}="
        clip = "S" if k == 0 else "H"
        cigs.append(np.array(cg.encode((f"{lead}{clip}" if lead else "") + body + (f"{trail}{clip}" if trail else "")), np.uint32))
    off = np.zeros(len(order) + 1, np.uint32)
    off[1:] = np.cumsum([len(c) for c in cigs])
    col = lambda j: np.array([LIFT_SEGS[k][j] for k in order])
    return abi.IndexData(contig_len=np.array([LIFT_CONTIG_LEN]), contig_seg_off=np.array([0, len(order)], np.uint32), seg_chrom_index=col(4).astype(np.uint32),
                         seg_pos=col(5), seg_is_fwd_strand=col(2).astype(np.uint8), seg_mapq=col(3).astype(np.uint8), seg_seq_order_start=col(0),
                         seg_seq_order_end=col(1), seg_cigar_off=off, seg_cigar=np.concatenate(cigs),
                         chrom_seq=[np.full(n, ord("N"), np.uint8) for n in LIFT_CHROM_LEN], rev_contig_seq=[np.full(LIFT_CONTIG_LEN, ord("N"), np.uint8)])


def lift_case(reads, seq_fmt=abi.SEQ_BAM4, **placement):
    """reads: (length, source flag, [(segment name or "gap" or "ins", offset into it, read segment is_fwd_strand, ops or None: length M), ...]).
    -> (Case without a lift, the item table the lift must produce: (read, status, flip, mapq, chrom, pos) per item).  A read segment in the
    gap produces no item, one inside G's inserted bases an item without a liftover; a read segment lies in front of or behind those bases."""
    rs, segs, table = [], [], []
    for r, (L, flag, placed) in enumerate(reads):
        rs.append((L, flag, None, None))
        for name, at, sfwd, ops in placed:
            ops = [M(L)] if ops is None else list(ops)
            clen = sum(int(c) >> 4 for c in ops if (int(c) & 15) in (0, 2, 3, 7, 8))  # contig bases the read segment spans
            if name == "gap":
                assert 0 <= at and at + clen <= 10_000
                segs.append((r, 0, LIFT_GAP + at, sfwd, ops))
                continue
            a, b, cfwd, mq, chrom, pos = LIFT_SEGS[INS_SEG if name == "ins" else name]
            p = a + (INS_AT + at if name == "ins" else at)
            assert a <= p and p + clen <= b and (name != "ins" or at + clen <= INS_LEN)  # inside its stretch: the table below holds
            assert name != INS_SEG or at + clen <= INS_AT or at >= INS_AT + INS_LEN
            segs.append((r, 0, p, sfwd, ops))
            flip = int((not cfwd) ^ (bool(flag & 0x10) == bool(sfwd)))
            if name == "ins":
                table.append((r, NOLIFT, 0, mq, chrom, -1))
            else:
                table.append((r, L_, flip, mq, chrom, pos + (p - a if cfwd else b - p - clen) - (INS_LEN if name == INS_SEG and at >= INS_AT + INS_LEN else 0)))
    return build(rs, None, seq_fmt, segs=segs, **placement), table
