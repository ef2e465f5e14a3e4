"""The front of every plo_liftover_batch* call in plain Python: the verdict of a batch, the spans and the merged op count of a read
segment, the item list and the class of every item.  TEST INFRASTRUCTURE ONLY.

Written from the documents, not from k_seg_count: include/portello_liftover.h (the checks of plo_liftover_batch_dev), IntRange::intersect_range
(lib/rust-vc-utils/src/int_range.rs:56-58: `other.end >= self.start && other.start < self.end`, self = the contig segment) and
get_contig_split_segments_from_read_mapping (src/read_alignment_scanner.rs:80-103).  Python ints, one segment at a time, no numpy
arithmetic: nothing here can wrap.

Coupling (as tests/test_bgzf_crafted.py notes for its grid formula): `region_dwords` restates lane_region_dwords / lane_region_gap /
LANE_SLACK of portello_amd/csrc/enumerate.hpp with PLO_LANE_GAP_HALVES = 4 and PLO_LANE_GAP_CONST = 0, and LANE_MAX_W restates the default
of plo_ctx::lane_max_w (192, engine.hip).  Which items count as light is a sizing decision of the engine, not a rule of the reference: if
those constants move, this file moves with them."""
from bisect import bisect_left, bisect_right

from portello_amd import abi

OK, INVALID_ARG, RANGE = abi.PLO_OK, abi.PLO_ERR_INVALID_ARG, abi.PLO_ERR_RANGE

OP_M, OP_I, OP_D, OP_N, OP_S, OP_H, OP_P, OP_EQ, OP_X = range(9)
REF_OPS = (OP_M, OP_D, OP_N, OP_EQ, OP_X)           # get_cigar_ref_offset
READ_OPS = (OP_M, OP_I, OP_S, OP_H, OP_EQ, OP_X)    # get_cigar_read_offset(cigar, false)
MATCH_OPS = (OP_M, OP_EQ, OP_X)                     # is_alignment_match

POS_MAX = 0x7FFFFFF0        # last accepted seg_pos
SPAN_LIMIT = 1 << 30        # first refused reference span
OPS_MAX = 0x7FFFFFFF        # last accepted seg_cigar_off value
READ_SPAN_SAT = 0xFFFFFFFF

LANE_MAX_W = 192
LANE_SLACK = 2
LANE_GAP_HALVES = 4
LANE_GAP_CONST = 0


def op(length: int, code: int) -> int:
    return (length << 4) | code


def seg_ops(batch, s):
    """the ops of read segment s as Python ints (an inverted offset pair holds none)"""
    c0, c1 = int(batch.seg_cigar_off[s]), int(batch.seg_cigar_off[s + 1])
    return [int(x) for x in batch.cigar[c0:c1]] if c1 > c0 else []


def ref_span(ops) -> int:
    return sum(c >> 4 for c in ops if (c & 15) in REF_OPS)


def read_span(ops) -> int:
    return sum(c >> 4 for c in ops if (c & 15) in READ_OPS)


def read_span_sat(ops) -> int:
    """what the length check compares read_seq_len with: a span of 2^32 - 1 or more is 2^32 - 1 (no read is that long)"""
    return min(read_span(ops), READ_SPAN_SAT)


def n_merged(ops) -> int:
    """ops once neighbouring alignment-match ops (M = X, any mixture, zero lengths included) are one"""
    n, prev = 0, False
    for c in ops:
        m = (c & 15) in MATCH_OPS
        if not (m and prev):
            n += 1
        prev = m
    return n


def sparse_header_bytes(seq_len: int) -> int:
    """PLO_SEQ_BAM4_SPARSE: 8 bytes per granule of 1024 bases, rounded up to 16"""
    return ((((seq_len + 1023) >> 10) * 8) + 15) & ~15


def bases_needed(seq_fmt: int, seq_len: int) -> int:
    if seq_fmt == abi.SEQ_BAM4:
        return (seq_len + 1) // 2
    if seq_fmt == abi.SEQ_BAM4_SPARSE:
        return sparse_header_bytes(seq_len)
    return seq_len


def contig_segments(index, contig):
    g0, g1 = int(index.contig_seg_off[contig]), int(index.contig_seg_off[contig + 1])
    return g0, g1


def segment_faults(index, batch, s):
    """(index fault, range fault) of read segment s"""
    idx = rng = False
    n_ops_all = int(batch.seg_cigar_off[batch.n_segs])
    c0, c1 = int(batch.seg_cigar_off[s]), int(batch.seg_cigar_off[s + 1])
    if c1 < c0 or c1 > n_ops_all:
        idx = True      # the segment's ops are not a stretch of the batch's
    elif c1 > OPS_MAX:
        rng = True
    pos = int(batch.seg_pos[s])
    if pos < 0 or pos > POS_MAX:
        rng = True
    if int(batch.seg_contig[s]) >= index.n_contigs:
        idx = True
    rd = int(batch.seg_read[s])
    if rd >= batch.n_reads:
        idx = True
    else:
        ln, off, total = int(batch.read_seq_len[rd]), int(batch.read_seq_off[rd]), int(batch.seq.nbytes)
        if off > total or bases_needed(batch.seq_fmt, ln) > total - off:
            idx = True
        if batch.seq_fmt == abi.SEQ_BAM4_SPARSE and off % 16:
            idx = True
    if not (c1 < c0 or c1 > n_ops_all):
        ops = seg_ops(batch, s)
        if any((c & 15) > 8 for c in ops):
            rng = True
        if ref_span(ops) >= SPAN_LIMIT:
            rng = True
    return idx, rng


def verdict(index, batch, stages=abi.STAGES_ALL) -> int:
    """PLO_OK, PLO_ERR_INVALID_ARG or PLO_ERR_RANGE; an index fault anywhere in the batch wins over a range fault anywhere"""
    idx = rng = False
    clean = []
    for s in range(batch.n_segs):
        i, r = segment_faults(index, batch, s)
        idx, rng = idx or i, rng or r
        if not (i or r):
            clean.append(s)
    # a segment that ends behind its contig's end and meets a reverse-strand contig segment: rev_pos (read_alignment_scanner.rs:164-166) would
    # be negative, the reference casts it to usize and panics in the block map's range query
    if batch.item_seg is None:
        pairs = [(s, k) for s in clean for k in segment_items(index, batch, s)]
    else:
        def n_csegs(s):
            g0, g1 = contig_segments(index, int(batch.seg_contig[s]))
            return g1 - g0
        pairs = [(int(a), int(b)) for a, b in zip(batch.item_seg, batch.item_cseg) if int(a) in clean and int(b) < n_csegs(int(a))]
    if any(item_pos1(index, batch, s, k, stages) < 0 for s, k in pairs):
        rng = True
    if batch.item_seg is not None:
        for seg, cseg in zip(batch.item_seg, batch.item_cseg):
            seg, cseg = int(seg), int(cseg)
            if seg >= batch.n_segs:
                idx = True
                continue
            contig = int(batch.seg_contig[seg])
            if contig >= index.n_contigs:
                idx = True
                continue
            g0, g1 = contig_segments(index, contig)
            if cseg >= g1 - g0:
                idx = True
    return INVALID_ARG if idx else RANGE if rng else OK


def segment_items(index, batch, s):
    """the contig segments read segment s meets, in order (indices inside its contig's list)"""
    contig = int(batch.seg_contig[s])
    g0, g1 = contig_segments(index, contig)
    r_start = int(batch.seg_pos[s])
    r_end = r_start + ref_span(seg_ops(batch, s))
    return [g - g0 for g in range(g0, g1)
            if r_end >= int(index.seg_seq_order_start[g]) and r_start < int(index.seg_seq_order_end[g])]  # left adjacency counts


def item_list(index, batch):
    """[(item_seg, item_cseg)] of an accepted batch: the explicit list as it stands, else segment by segment in contig-segment order"""
    if batch.item_seg is not None:
        return [(int(a), int(b)) for a, b in zip(batch.item_seg, batch.item_cseg)]
    return [(s, k) for s in range(batch.n_segs) for k in segment_items(index, batch, s)]


def block_map_keys(index, g):
    """the keys of contig segment g's block map (get_read_segment_to_ref_pos_tree_map, read_to_ref_map.rs:101-137): start and end of every
    run of match ops in contig coordinates; a run that starts where the last one ended shares that key"""
    c0, c1 = int(index.seg_cigar_off[g]), int(index.seg_cigar_off[g + 1])
    keys, read_pos, run = [], 0, 0
    for c in [int(x) for x in index.seg_cigar[c0:c1]] + [op(0, OP_S)]:
        t, ln = c & 15, c >> 4
        if t in MATCH_OPS:
            run += ln
        elif run > 0:
            k0, k1 = read_pos - run, read_pos
            if not (keys and keys[-1] == k0):
                keys.append(k0)
            keys.append(k1)
            run = 0
        if t in READ_OPS:
            read_pos += ln
    return keys


def item_pos1(index, batch, s, k, stages=abi.STAGES_ALL) -> int:
    """where the item starts on its contig segment's strand (rev_pos, read_alignment_scanner.rs:164-166)"""
    contig = int(batch.seg_contig[s])
    g = int(index.contig_seg_off[contig]) + k
    pos = int(batch.seg_pos[s])
    if (stages & abi.STAGE_STRAND) and not int(index.seg_is_fwd_strand[g]):
        return int(index.contig_len[contig]) - (pos + ref_span(seg_ops(batch, s)))
    return pos


def region_dwords(n: int, w0: int, w1: int) -> int:
    return n + (LANE_GAP_HALVES * max(0, w1 - w0) + 1) // 2 + LANE_GAP_CONST + LANE_SLACK


def item_class(index, batch, s, k, keys=None, stages=abi.STAGES_ALL, lane_max_w=LANE_MAX_W) -> int:
    """bit 0: the item goes through the left shift (reverse contig segment); bit 1: heavy (its region is above lane_max_w).  `keys`: the
    block-map keys of the contig segment (plo_index_segment_map's where a device is at hand, block_map_keys otherwise)"""
    contig = int(batch.seg_contig[s])
    g = int(index.contig_seg_off[contig]) + k
    if keys is None:
        keys = block_map_keys(index, g)
    ops = seg_ops(batch, s)
    span = ref_span(ops)
    pos1 = item_pos1(index, batch, s, k, stages)
    lo, hi = max(pos1, -0x7FFFFFFF), min(pos1 + span, 0x7FFFFFFF)
    w0 = max(bisect_right(keys, lo) - 1, 0)             # the entry that holds the item's start (or the first)
    w1 = bisect_left(keys, hi, w0)                      # the first entry at or behind the item's end
    fwd = bool(int(index.seg_is_fwd_strand[g]))
    do_shift = bool(stages & abi.STAGE_LSHIFT) and (not (stages & abi.STAGE_STRAND) or not fwd)
    merges = do_shift or bool(stages & abi.STAGE_LIFTOVER)
    region = region_dwords(n_merged(ops) if merges else len(ops), w0, w1)
    return (1 if do_shift else 0) | (2 if region > lane_max_w else 0)


def class_counts(index, batch, keys_of=None):
    """[items of class 0, 1, 2, 3] of an accepted batch"""
    cnt = [0, 0, 0, 0]
    for s, k in item_list(index, batch):
        g = int(index.contig_seg_off[int(batch.seg_contig[s])]) + k
        cnt[item_class(index, batch, s, k, None if keys_of is None else keys_of(g))] += 1
    return cnt
