"""The liftover of one read alignment through one contig segment's block map, restated in plain Python from the reference's Rust text:
a third voice beside oracle/portello_oracle.c and the device code.  TEST INFRASTRUCTURE ONLY.  Imports nothing from oracle/ and nothing
compiled.

    R = lib/rust-vc-utils/src/bam_utils/read_to_ref_map.rs    C = lib/rust-vc-utils/src/bam_utils/cigar/mod.rs
    L = src/liftover_read_alignment.rs                         S = src/read_alignment_scanner.rs

A CIGAR is a list of (length, op) with op = 0 .. 8 for M I D N S H P = X (the BAM codes).  A block map is a pair of lists (keys, vals),
keys ascending, vals[i] None for an unmapped block."""
import bisect
import re

M, I, D, N, S, H, P, EQ, X = range(9)
OPS = "MIDNSHP=X"
LIFTED, NO_LIFTOVER, LEN_MISMATCH = 0, 1, 2
STAGE_STRAND, STAGE_LIFTOVER, STAGE_LENCHECK = 1, 4, 8
_RE = re.compile(r"(\d+)([MIDNSHP=X])")


def parse(text):
    ops = [(int(n), OPS.index(c)) for n, c in _RE.findall(text)]
    assert "".join(f"{n}{OPS[c]}" for n, c in ops) == text, text
    return ops


def fmt(ops):
    return "".join(f"{n}{OPS[c]}" for n, c in ops)


def from_words(words):
    return [(int(w) >> 4, int(w) & 15) for w in words]


def is_match(op):  # C:22-24
    return op in (M, EQ, X)


def read_offset(ln, op, ignore_hard_clip=False):  # C:26-39
    if op in (I, S, X, EQ, M):
        return ln
    if op == H:
        return 0 if ignore_hard_clip else ln
    return 0


def ref_offset(ln, op):  # C:41-47
    return ln if op in (D, N, X, EQ, M) else 0


def ref_span(ops):  # C:174-180
    return sum(ref_offset(n, c) for n, c in ops)


def read_span(ops):  # C:164-170, ignore_hard_clip = false
    return sum(read_offset(n, c) for n, c in ops)


def tree_map(ref_pos, ops, ignore_hard_clip=False):
    """get_read_segment_to_ref_pos_tree_map, R:101-137.  A block that starts where the last one ended (a D or N between two matches: the read
    position does not move) overwrites that block's closing None: BTreeMap::insert on an equal key."""
    m = {}
    read_pos, match_len = 0, 0

    def flush():  # R:111-119
        nonlocal match_len
        if match_len > 0:
            m[read_pos - match_len] = ref_pos - match_len
            m[read_pos] = None
            match_len = 0

    for n, c in ops:
        if is_match(c):  # R:125-127
            match_len += n
        else:  # R:128-130
            flush()
        read_pos += read_offset(n, c, ignore_hard_clip)  # R:132
        ref_pos += ref_offset(n, c)
    flush()  # R:134
    keys = sorted(m)
    return keys, [m[k] for k in keys]


def get_ref_pos(keys, vals, read_pos):  # R:67-72
    i = bisect.bisect_right(keys, read_pos) - 1
    if i < 0 or vals[i] is None:
        return None
    return vals[i] + (read_pos - keys[i])


def get_ref_range(keys, a, b):
    """R:74-85 as indices [i0, i1) into keys: from the last key <= a (from a itself if there is none) up to, not including, b"""
    i = bisect.bisect_right(keys, a) - 1
    start = keys[i] if i >= 0 else a  # R:79-82
    i0 = bisect.bisect_left(keys, start)
    i1 = bisect.bisect_left(keys, b)  # R:84: start .. b, b excluded
    return i0, max(i0, i1)


def clean_up_cigar_edge_indels(ops):
    """C:265-291, in place; returns the shift of the start"""
    def update(k):  # C:266-275
        n, c = ops[k]
        if c == D:
            ops[k] = (0, S)
            return n
        if c == I:
            ops[k] = (n, S)
        return 0

    shift = 0
    for k in range(len(ops)):  # C:278-280
        if is_match(ops[k][1]):
            break
        shift += update(k)
    for k in range(len(ops) - 1, -1, -1):  # C:282-288
        if is_match(ops[k][1]):
            break
        update(k)
    return shift


def compress_cigar(ops):
    """C:204-228.  (Pad has no length to add to in C:210-215: two neighbouring P would keep the first one's.  The liftover never emits P.)"""
    out = []
    last = (0, M)
    for n, c in ops:
        if n == 0:  # C:207
            continue
        if c == last[1]:
            last = (last[0] + (n if c != P else 0), c)
        else:
            if last[0] != 0:
                out.append(last)
            last = (n, c)
    if last[0] != 0:
        out.append(last)
    return out


def liftover_read_alignment(keys, vals, start, ops):
    """L:137-223 with update_ref2_cigar_segment (L:35-133) inside.  -> (None or (pos, cigar), (w0, w1)): the result, and the range of map
    indices that the range queries of the alignment's ops touch, their union (for an alignment without a reference-consuming op, which asks
    nothing: the query of its empty span)."""
    ref2_start = None
    ref2_end = None
    out = []
    w0, w1 = None, None
    seg_start = start
    for n, c in ops:
        if c in (I, S, H):  # L:157-160
            out.append((n, c))
        elif c in (X, EQ, M, D, N):  # L:161-212
            last = None
            block_pos = seg_start  # L:177
            seg_end = seg_start + n
            i0, i1 = get_ref_range(keys, seg_start, seg_end)
            w0 = i0 if w0 is None else min(w0, i0)
            w1 = i1 if w1 is None else max(w1, i1)
            for this in [(keys[i], vals[i]) for i in range(i0, i1)] + [None]:  # L:181-211
                end = min(this[0], seg_end) if this is not None else seg_end  # L:62-67
                if end > block_pos:  # L:69
                    ln = end - block_pos
                    if last is not None:
                        lk, lv = last
                        if lv is not None:  # L:83-110
                            if is_match(c) and ref2_start is None:
                                ref2_start = lv + (block_pos - lk)
                            if ref2_end is not None:
                                d = lv - ref2_end
                                if d > 0 and ref2_start is not None:
                                    out.append((d, D))
                            ref2_end = lv + (end - lk)
                            if is_match(c) or ref2_start is not None:
                                out.append((ln, c if c in (D, N) else M))
                        elif is_match(c):  # L:111-115
                            out.append((ln, I))
                    elif is_match(c):  # L:117-123
                        out.append((ln, S))
                    block_pos = end  # L:124
                last = this if this is not None else last  # L:199
        # Pad: L:213
        seg_start += ref_offset(n, c)  # L:215
    if w0 is None:
        w0, w1 = get_ref_range(keys, start, start)
    if ref2_start is None:  # L:218
        return None, (w0, w1)
    shift = clean_up_cigar_edge_indels(out)
    return (ref2_start + shift, compress_cigar(out)), (w0, w1)


# ---- one item of a batch: the caller glue of S:146-183 for the stage sets without the shift and simplify stages ------------------------

def segment_map(index, g):
    """the block map of contig segment g of an abi.IndexData (src/contig_alignment_scanner/mod.rs:98-102: ignore_hard_clip = false)"""
    c0, c1 = int(index.seg_cigar_off[g]), int(index.seg_cigar_off[g + 1])
    return tree_map(int(index.seg_pos[g]), from_words(index.seg_cigar[c0:c1]))


def item_list(index, batch):
    """(seg, cseg) in the reference's order: S:80-103, a contig segment is met when r_end >= start and r_start < end"""
    out = []
    for s in range(batch.n_segs):
        ops = from_words(batch.cigar[int(batch.seg_cigar_off[s]):int(batch.seg_cigar_off[s + 1])])
        r0 = int(batch.seg_pos[s])
        r1 = r0 + ref_span(ops)
        ct = int(batch.seg_contig[s])
        g0, g1 = int(index.contig_seg_off[ct]), int(index.contig_seg_off[ct + 1])
        for g in range(g0, g1):
            if r1 >= int(index.seg_seq_order_start[g]) and r0 < int(index.seg_seq_order_end[g]):
                out.append((s, g - g0))
    return out


def lift_item(index, batch, seg, cseg, stages=STAGE_STRAND | STAGE_LIFTOVER):
    """-> (status, pos, cigar, (w0, w1), number of keys): position and CIGAR None unless the status is LIFTED or LEN_MISMATCH; the window
    counts from the first key of the segment's map.  Stages: STRAND | LIFTOVER, with or without LENCHECK."""
    assert stages & STAGE_LIFTOVER and not stages & ~(STAGE_STRAND | STAGE_LIFTOVER | STAGE_LENCHECK)
    ct = int(batch.seg_contig[seg])
    g = int(index.contig_seg_off[ct]) + cseg
    ops = from_words(batch.cigar[int(batch.seg_cigar_off[seg]):int(batch.seg_cigar_off[seg + 1])])
    pos = int(batch.seg_pos[seg])
    if stages & STAGE_STRAND and not int(index.seg_is_fwd_strand[g]):  # S:164-166
        pos = int(index.contig_len[ct]) - (pos + ref_span(ops))
        ops = ops[::-1]
    keys, vals = segment_map(index, g)
    res, win = liftover_read_alignment(keys, vals, pos, ops)  # S:179-183
    if res is None:
        return NO_LIFTOVER, None, None, win, len(keys)
    status = LIFTED
    if stages & STAGE_LENCHECK and int(batch.read_seq_len[int(batch.seg_read[seg])]) != read_span(res[1]):  # S:204-229
        status = LEN_MISMATCH
    return status, res[0], res[1], win, len(keys)
