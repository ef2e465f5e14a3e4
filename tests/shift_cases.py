"""Hand-built items for the left-shift stage of the lane-per-item kernel (lane_core.hpp: the lockstep loop for clean items, the
event-aligned walk for the others): the catalogue of tests/test_shift_lockstep.py and tests/test_shift_lockstep_gpu.py.
TEST INFRASTRUCTURE ONLY.

An item is written in WALKING coordinates -- the order in which the shift stage sees it: `ref`, the reversed contig (two letters, long
runs, so that homologies are long), the position `pos` on it, the ops `ops` in walking order and the bases an insertion or a clip brings.
The read is derived from these (match ops copy the contig), and batch() turns the items into what a stage set reads them from:
  * with the strand stage: one REVERSE contig segment per item's contig, the CIGAR reversed, seg_pos counted from the contig's other end,
    the read stored as walked (need_flipped = 0) or reverse-complemented (need_flipped = 1);
  * without it (STAGE_LSHIFT alone): the ops, the position and the read as walked.
model() restates the stage for a clean item by the closed form M(a0 - s1) X1 M(s1 + a1 - s2) .. Xn M(sn + an), s_j = min(s_{j-1} + a_{j-1}, h_j):
the catalogue uses it to CHOOSE items with a wanted property (fixed seeds, searched when the module is loaded) and the tests assert each
property before they use the item; what the stages must compute is the oracle's business."""
from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from portello_amd import abi

OP_M, OP_I, OP_D, OP_N, OP_S, OP_H, OP_P, OP_EQ, OP_X = range(9)
_READ = (OP_M, OP_I, OP_S, OP_H, OP_EQ, OP_X)  # (the stage's read head moves over hard clips too)
_REF = (OP_M, OP_D, OP_N, OP_EQ, OP_X)
_COMP = bytes.maketrans(b"ACGT", b"TGCA")


def op(n, t):
    return (n << 4) | t


@dataclass
class Item:
    name: str
    ref: bytes                 # the reversed contig
    pos: int
    ops: List[int]             # walking order
    read: bytes = b""          # derived
    flip: int = 0              # need_flipped under the strand stage
    fwd_contig: bool = False   # the contig segment maps forward: no shift stage under STAGE_STRAND
    why: str = ""

    @property
    def ref_span(self):
        return sum(c >> 4 for c in self.ops if (c & 15) in _REF)


def derive_read(ref: bytes, pos: int, ops, ins=None, clip=b"C") -> bytes:
    """match ops copy the contig (bases behind its end are 'A'), an insertion brings `ins` (default: the read base in front of it,
    repeated -- a homopolymer grows), a clip brings `clip` repeated"""
    out, r = bytearray(), pos
    ins = list(ins or [])
    for c in ops:
        t, n = c & 15, c >> 4
        if t in (OP_M, OP_EQ, OP_X):
            out += bytes(ref[r + k] if 0 <= r + k < len(ref) else 65 for k in range(n))
        elif t == OP_I:
            out += ins.pop(0) if ins else bytes([out[-1] if out else 65]) * n
        elif t in (OP_S, OP_H):
            out += clip * n
        r += n if t in _REF else 0
    return bytes(out)


def item(name, ref, pos, ops, ins=None, flip=0, fwd_contig=False, why=""):
    return Item(name, bytes(ref), pos, [int(c) for c in ops], derive_read(ref, pos, ops, ins), flip, fwd_contig, why)


# ---- the stage restated for clean items -------------------------------------------------------------------------------------------------

def is_clean(ops) -> bool:
    """(S|H)* M (X M)* (S|H)* after match runs are merged: every length > 0, X one I or one D, no equal neighbours, no N, no P"""
    st = []
    for c in ops:
        t, n = c & 15, c >> 4
        t = OP_M if t in (OP_EQ, OP_X) else t
        if st and st[-1][0] == OP_M and t == OP_M:
            st[-1][1] += n
        else:
            st.append([t, n])
    if any(n == 0 for _, n in st) or any(a[0] == b[0] for a, b in zip(st, st[1:])):
        return False
    s = "".join("M" if t == OP_M else "X" if t in (OP_I, OP_D) else "C" if t in (OP_S, OP_H) else "?" for t, _ in st)
    import re
    return re.fullmatch(r"C*M(XM)*C*", s) is not None


@dataclass
class Cluster:
    a: int          # the match in front
    bound: int      # s_{j-1} + a_{j-1}
    max_left: int   # min(rs, qs)
    h: int          # the homology, at most min(max_left, bound)
    raw: int        # ... at most max_left
    rs: int
    qs: int
    re: int
    qe: int
    panic: bool


def model(it: Item) -> Optional[List[Cluster]]:
    """the clusters of a clean item (merged ops), None for an unclean one"""
    if not is_clean(it.ops):
        return None
    st = []
    for c in it.ops:
        t, n = c & 15, c >> 4
        t = OP_M if t in (OP_EQ, OP_X) else t
        if st and st[-1][0] == OP_M and t == OP_M:
            st[-1][1] += n
        else:
            st.append([t, n])
    ref, read = it.ref, it.read
    r, q, carry, a, out = it.pos, 0, 0, 0, []
    for t, n in st:
        if t == OP_M:
            a = n
            r += n
            q += n
        elif t in (OP_I, OP_D):
            rs, qs = r, q
            re_, qe = rs + (n if t == OP_D else 0), qs + (n if t == OP_I else 0)
            max_left = min(rs, qs)
            panic = max_left > 0 and (re_ - 1 >= len(ref) or qe - 1 >= len(read))
            raw = 0
            if not panic:
                while raw < max_left and ref[re_ - 1 - raw] == read[qe - 1 - raw]:
                    raw += 1
            bound = carry + a
            h = min(raw, bound)
            out.append(Cluster(a, bound, max_left, h, raw, rs, qs, re_, qe, panic))
            carry = h
            r, q = re_, qe
        else:
            q += n  # clips
    return out


def shifted_ops(it: Item):
    """the closed form, for items no match of which is emptied"""
    cl = model(it)
    st = []
    for c in it.ops:
        t, n = c & 15, c >> 4
        t = OP_M if t in (OP_EQ, OP_X) else t
        if st and st[-1][0] == OP_M and t == OP_M:
            st[-1][1] += n
        else:
            st.append([t, n])
    j, carry = 0, 0
    ms = [k for k, (t, _) in enumerate(st) if t == OP_M]
    for j, c in enumerate(cl):
        st[ms[j]][1] = c.bound - c.h
        assert st[ms[j]][1] > 0
        carry = c.h
    st[ms[-1]][1] += carry
    return [op(n, t) for t, n in st]


# ---- contigs and shapes -------------------------------------------------------------------------------------------------------------------

def runs(rng, n, lo=1, hi=12) -> bytes:
    """n bases of alternating runs of A and C"""
    out, ch = bytearray(), int(rng.integers(0, 2))
    while len(out) < n:
        out += (b"A", b"C")[ch] * int(rng.integers(lo, hi + 1))
        ch ^= 1
    return bytes(out[:n])


def random_clean(rng, name, n_cl, a_lo=1, a_hi=24, lead=(), trail=(), pos_max=40, ref_len=400, run_hi=12, wild=False, **kw) -> Item:
    """a clean item whose indels grow or shrink the homopolymer they stand in (the deleted bases continue the run in front of them);
    `wild`: half of the indels bring or remove whatever bases come instead"""
    ref = bytearray(runs(rng, ref_len, 1, run_hi))
    pos = int(rng.integers(0, pos_max + 1))
    ops, r, ins = list(lead), pos, []
    for j in range(n_cl):
        a = int(rng.integers(a_lo, a_hi + 1))
        ops.append(op(a, OP_M))
        r += a
        n = int(rng.integers(1, 4))
        tame = not (wild and rng.integers(0, 2))
        if rng.integers(0, 2):
            for k in range(n if tame else 0):
                ref[r + k] = ref[r - 1]
            ops.append(op(n, OP_D))
            r += n
        else:
            ins.append(bytes([ref[r - 1]]) * n if tame else bytes(b"AC"[int(x)] for x in rng.integers(0, 2, n)))
            ops.append(op(n, OP_I))
    ops.append(op(int(rng.integers(a_lo, a_hi + 1)), OP_M))
    ops += list(trail)
    return item(name, bytes(ref), pos, ops, ins=ins, **kw)


def search(name, want, why, seeds=range(4000), **kw) -> Item:
    for s in seeds:
        it = random_clean(np.random.default_rng(1000 + s), name, **kw)
        cl = model(it)
        if cl is not None and want(it, cl):
            it.why = why
            return it
    raise AssertionError("no item for " + name)


def _none_emptied(cl):
    return all(c.bound - c.h > 0 for c in cl)


def edge_items() -> List[Item]:
    """one clean item per edge of the lockstep loop"""
    S, H = OP_S, OP_H
    out = [
        search("partial_del", lambda it, cl: it.ops[1] & 15 == OP_D and 0 < cl[0].h < cl[0].a, "a deletion shifts by 0 < h < a", n_cl=1, a_lo=8),
        search("partial_ins", lambda it, cl: it.ops[1] & 15 == OP_I and 0 < cl[0].h < cl[0].a, "an insertion shifts by 0 < h < a", n_cl=1, a_lo=8),
        search("eat_middle", lambda it, cl: cl[0].bound > cl[0].h and any(c.bound == c.h for c in cl[1:]) and not any(c.panic for c in cl),
               "a match in the middle is emptied: its neighbours meet", n_cl=4, a_hi=4),
        search("eat_first_del", lambda it, cl: it.ops[1] & 15 == OP_D and cl[0].bound == cl[0].h, "the first match is emptied: the deletion is dropped, the position moves",
               n_cl=2, a_hi=5),
        search("eat_first_ins", lambda it, cl: it.ops[1] & 15 == OP_I and cl[0].bound == cl[0].h, "the first match is emptied: the insertion becomes a clip",
               n_cl=2, a_hi=5),
        search("eat_first_ins_clip", lambda it, cl: it.ops[2] & 15 == OP_I and cl[0].bound == cl[0].h, "... and joins the clip in front of it",
               n_cl=2, a_hi=5, lead=(op(4, S),)),
        search("chain_clamp_inside", lambda it, cl: cl[0].h > 0 and cl[1].a <= 2 and cl[1].a < cl[1].h < cl[1].bound and _none_emptied(cl),
               "cluster 2 shifts into the bases cluster 1 handed on", n_cl=2, a_lo=1, a_hi=9, wild=True, run_hi=4, seeds=range(40000)),
        search("chain_clamp_hit", lambda it, cl: cl[0].h > 0 and cl[1].a <= 2 and cl[1].raw > cl[1].bound > cl[1].a and cl[0].bound > cl[0].h,
               "cluster 2's homology ends at its clamp s1 + a1", n_cl=2, a_lo=1, a_hi=9),
        search("h16", lambda it, cl: cl[0].h == 16 and cl[0].raw == 16 and cl[0].a > 16, "homology of exactly one window", n_cl=1, a_lo=30, a_hi=60, run_hi=30),
        search("h_over_16", lambda it, cl: 16 < cl[0].h < 32 and cl[0].a > cl[0].h, "the window is continued once", n_cl=1, a_lo=40, a_hi=60, run_hi=40),
        search("h_over_32", lambda it, cl: cl[0].h > 33 and cl[0].a > cl[0].h, "the window is continued twice", n_cl=1, a_lo=60, a_hi=90, run_hi=80),
        search("to_contig_start", lambda it, cl: it.pos == 0 and cl[0].raw == cl[0].max_left == cl[0].rs, "the homology ends at the contig's first base",
               n_cl=2, a_hi=12, pos_max=0),
        search("to_read_start", lambda it, cl: it.pos > 0 and cl[0].raw == cl[0].max_left == cl[0].qs, "the homology ends at the read's first base",
               n_cl=2, a_hi=12),
        search("window_outside", lambda it, cl: cl[0].re < 16 and 0 < cl[0].h < cl[0].a and cl[1].h > 0, "the first window starts in front of the contig",
               n_cl=2, a_lo=4, a_hi=10, pos_max=2),
        search("clips_lead_s", lambda it, cl: cl[0].h > 0 and _none_emptied(cl), "a leading soft clip", n_cl=3, lead=(op(5, S),)),
        search("clips_lead_hs", lambda it, cl: cl[1].h > 0 and _none_emptied(cl), "leading H S", n_cl=3, lead=(op(3, H), op(5, S))),
        search("clips_trail_s", lambda it, cl: cl[2].h > 0 and _none_emptied(cl), "a trailing soft clip", n_cl=3, trail=(op(7, S),)),
        search("clips_trail_sh", lambda it, cl: cl[2].h > 0 and _none_emptied(cl), "trailing S H", n_cl=3, trail=(op(7, S), op(2, H))),
        search("clips_both", lambda it, cl: cl[0].h > 0 and cl[2].h > 0 and _none_emptied(cl), "clips at both ends", n_cl=3, lead=(op(2, H), op(6, S)), trail=(op(1, S), op(9, H))),
        search("clips_h_only", lambda it, cl: cl[0].h > 0, "hard clips alone", n_cl=2, lead=(op(4, H),), trail=(op(4, H),)),
        search("many_clusters", lambda it, cl: sum(c.h > 0 for c in cl) >= 8 and _none_emptied(cl), "a long chain", n_cl=21, a_lo=2, a_hi=9),
        search("flipped", lambda it, cl: cl[0].h > 0 and cl[1].h > 0, "need_flipped = 1", n_cl=3, flip=1),
        search("flipped_eaten", lambda it, cl: any(c.bound == c.h for c in cl), "need_flipped = 1, a match emptied", n_cl=3, a_hi=4, flip=1),
    ]
    # no cluster at all
    rng = np.random.default_rng(5)
    ref = runs(rng, 300)
    p = next(p for p in range(20, 200) if ref[p] != ref[p - 1])  # a run starts at p: deleting its first base leaves nothing to shift over
    out.append(item("no_homology", ref, p - 12, [op(12, OP_M), op(1, OP_D), op(15, OP_M)], why="nothing moves"))
    out.append(item("no_cluster", ref, 7, [op(50, OP_M)], why="one match"))
    out.append(item("no_cluster_eqx", ref, 7, [op(3, S), op(20, OP_EQ), op(1, OP_X), op(30, OP_EQ), op(2, S)], why="= X = between clips: one match once merged"))
    out.append(item("lone_eq", ref, 9, [op(40, OP_EQ)], why="a lone = is written as M"))
    out.append(item("eqx_clusters", ref, 3, [op(9, OP_EQ), op(1, OP_X), op(4, OP_EQ), op(2, OP_D), op(1, OP_X), op(1, OP_I), op(12, OP_EQ)], why="= / X runs between lone indels"))
    return out


def panic_items() -> List[Item]:
    """the cluster's reference range ends behind the contig (re - 1 >= ref_len): the reference's slice index panics.  In walking
    coordinates such an item leaves its contig, so a batch holds it only without the strand stage (with it, seg_pos would be negative)."""
    rng = np.random.default_rng(6)
    ref = runs(rng, 60)
    return [item("panic_del", ref, 30, [op(28, OP_M), op(5, OP_D), op(6, OP_M)], why="the deletion ends three bases behind the contig"),
            item("panic_second", ref, 30, [op(10, OP_M), op(1, OP_I), op(19, OP_M), op(2, OP_D), op(6, OP_M)], why="the second cluster panics, the first is fine")]


def unclean_items() -> List[Item]:
    """one item per reason for the event-aligned walk"""
    rng = np.random.default_rng(7)
    S, H, M, I, D, N, P = OP_S, OP_H, OP_M, OP_I, OP_D, OP_N, OP_P
    mk = lambda name, ops, why, **kw: item(name, runs(rng, 300), 11, ops, why=why, **kw)
    return [
        mk("u_ss", [op(2, S), op(3, S), op(20, M), op(1, D), op(9, M)], "S S in front"),
        mk("u_ss_trail", [op(20, M), op(1, I), op(9, M), op(2, S), op(3, S)], "S S behind"),
        mk("u_n", [op(12, M), op(1, D), op(6, M), op(30, N), op(9, M), op(2, I), op(5, M)], "N"),
        mk("u_p", [op(12, M), op(1, I), op(6, M), op(2, P), op(9, M), op(2, D), op(5, M)], "P"),
        mk("u_id", [op(12, M), op(2, I), op(1, D), op(9, M), op(1, D), op(7, M)], "I D neighbours"),
        mk("u_di", [op(12, M), op(2, D), op(1, I), op(9, M)], "D I neighbours"),
        mk("u_ii", [op(12, M), op(2, I), op(1, I), op(9, M)], "I I neighbours"),
        mk("u_zero_m", [op(12, M), op(2, I), op(0, M), op(1, D), op(9, M)], "a zero-length match"),
        mk("u_zero_i", [op(12, M), op(0, I), op(9, M), op(1, D), op(4, M)], "a zero-length insertion"),
        mk("u_zero_s", [op(0, S), op(12, M), op(1, D), op(9, M)], "a zero-length clip"),
        mk("u_lead_i", [op(2, I), op(12, M), op(1, D), op(9, M)], "a leading insertion"),
        mk("u_lead_d", [op(3, S), op(2, D), op(12, M), op(1, I), op(9, M)], "a leading deletion behind a clip"),
        mk("u_trail_d", [op(12, M), op(1, I), op(9, M), op(2, D)], "a trailing deletion"),
        mk("u_trail_i_clip", [op(12, M), op(1, D), op(9, M), op(2, I), op(3, S)], "a trailing insertion in front of a clip"),
        mk("u_clip_inside", [op(12, M), op(1, D), op(9, M), op(3, S), op(5, M)], "a clip between matches"),
        mk("u_only_clips", [op(5, S), op(4, H)], "no match at all"),
    ]


def mixed_items(n=70, seed=3) -> List[Item]:
    """about `n` items, two groups of the shift class: clean lanes, lanes that empty a match, unclean lanes, forward contigs"""
    rng = np.random.default_rng(seed)
    out, pool = [], unclean_items()
    for k in range(n):
        r = k % 7
        if r == 5:
            u = pool[(k // 7) % len(pool)]
            out.append(Item(f"mix{k}_{u.name}", u.ref, u.pos, u.ops, u.read, int(rng.integers(0, 2)), False, u.why))
        else:
            # (r = 2: short matches, most of them emptied; r = 0, 4: matches longer than the runs, none emptied as a rule)
            it = random_clean(rng, f"mix{k}", n_cl=int(rng.integers(0, 26)), a_lo=(9 if r in (0, 4) else 1), a_hi=(3 if r == 2 else 20),
                              run_hi=(6 if r in (0, 4) else 12), flip=int(rng.integers(0, 2)), fwd_contig=(r == 6),
                              lead=((op(3, OP_S),) if r == 1 else ()), trail=((op(2, OP_S), op(5, OP_H)) if r == 3 else ()), ref_len=700)
            out.append(it)
    return out


# ---- items -> index + batch ---------------------------------------------------------------------------------------------------------------

def _revcomp(b: bytes) -> bytes:
    return b.translate(_COMP)[::-1]


def build(items: List[Item], stages: int, seq_fmt=abi.SEQ_ASCII):
    """one contig (one segment over all of it, one block onto chr0) and one read per item"""
    strand = bool(stages & abi.STAGE_STRAND)
    n = len(items)
    rng = np.random.default_rng(99)
    clen = [len(it.ref) for it in items]
    cpos = np.concatenate([[100], 100 + np.cumsum(clen)[:-1] + 50 * np.arange(1, n)]) if n else np.zeros(0, np.int64)
    coff = np.arange(n + 1, dtype=np.uint32)
    index = abi.IndexData(contig_len=clen, contig_seg_off=np.arange(n + 1), seg_chrom_index=np.zeros(n), seg_pos=cpos,
                          seg_is_fwd_strand=[1 if it.fwd_contig else 0 for it in items], seg_mapq=np.full(n, 60), seg_seq_order_start=np.zeros(n),
                          seg_seq_order_end=clen, seg_cigar_off=coff, seg_cigar=np.array([op(L, OP_M) for L in clen], np.uint32),
                          chrom_seq=[np.frombuffer(b"AC", np.uint8)[rng.integers(0, 2, int(sum(clen)) + 50 * n + 400)]],
                          rev_contig_seq=[np.frombuffer(it.ref, np.uint8) for it in items])
    read_rev, seqs, spos, ops, offs = [], [], [], [], [0]
    for it in items:
        rev = strand and not it.fwd_contig
        flip = bool(it.flip) and rev
        # need_flipped = (contig reverse) != (read_is_reverse == seg_is_fwd_strand), seg_is_fwd_strand = 1
        read_rev.append((0 if flip else 1) if rev else 0)
        seqs.append(np.frombuffer(_revcomp(it.read) if flip else it.read, np.uint8))
        spos.append(len(it.ref) - it.pos - it.ref_span if rev else it.pos)
        ops += it.ops[::-1] if rev else it.ops
        offs.append(len(ops))
    slen = np.array([len(s) for s in seqs], np.uint32)
    soff = np.zeros(n, np.uint64)
    soff[1:] = np.cumsum(slen[:-1])
    seq = np.concatenate(seqs) if n else np.zeros(0, np.uint8)
    if seq_fmt == abi.SEQ_BAM4:
        code = np.zeros(256, np.uint8)
        for ch, v in zip(b"ACGT", (1, 2, 4, 8)):
            code[ch] = v
        packed, soff = [], np.zeros(n, np.uint64)
        at = 0
        for k, s in enumerate(seqs):
            c = code[s]
            if len(c) & 1:
                c = np.append(c, 0)
            packed.append(((c[0::2] << 4) | c[1::2]).astype(np.uint8))
            soff[k] = at
            at += len(packed[-1])
        seq = np.concatenate(packed) if n else np.zeros(0, np.uint8)
    batch = abi.BatchData(read_is_reverse=read_rev, read_seq_len=slen, read_seq_off=soff, seq=seq, seq_fmt=seq_fmt, seg_read=np.arange(n),
                          seg_contig=np.arange(n), seg_pos=np.array(spos, np.int64), seg_is_fwd_strand=np.ones(n), seg_cigar_off=offs,
                          cigar=np.array(ops, np.uint32))
    return index, batch


STAGE_SETS = (abi.STAGES_ALL, abi.STAGE_LSHIFT, abi.STAGE_STRAND | abi.STAGE_LSHIFT)
