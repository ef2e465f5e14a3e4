"""Hand-built block maps and placements at the edges of the liftover stage -- the composition of a read's CIGAR through a contig segment's
block map (lane_tile in lane_core.hpp, wave B of lane_stream.hpp, the scan formulation of lift_core.hpp) and the window search in front of
it (build_item_desc, enumerate.hpp): the catalogue of tests/test_liftover_edges.py.  TEST INFRASTRUCTURE ONLY.

One index serves all cases (INDEX).  Every map of MAPS stands on two contigs of its own, each with ONE contig segment that covers the whole
contig: `<name>_f` forward, `<name>_r` reverse (the segment's CIGAR then runs on the reversed contig and an item is placed mirrored with its
ops reversed, so that the SAME (start, CIGAR) reaches the liftover on either strand; every contig has a rev_contig_seq, so under STAGES_ALL
the left shift runs in front of the liftover on the reverse one).  Order in ix.kv: J U Z K KS O (forward, reverse each), then A_f B_f A_r
B_r -- map B follows map A directly (kv0(B) == kv1(A)), and B_r is the last map of the index: its last key is the last word of ix.kv.

Family P (pieces): a placement is (name, map, start, CIGAR, expected, why) with `expected` = None (NO_LIFTOVER) or (pos, CIGAR) WRITTEN BY
HAND beside it from the Rust text, never computed, for the stage set STRAND | LIFTOVER (where the start and CIGAR below reach the liftover
as written; under STAGES_ALL the shift and simplify stages stand around it and the oracle is the expectation).  The same values are stored
in tests/golden/liftover_vectors.json.

Family S (staging): generated from the number of staged entries (`kvs`: LANE_KVS = 128, or what PLO_LANE_KVS sets on the card); a group
case is a batch of at most 64 light items of one class, so it is one group of the lane kernel whatever the sort does."""
from dataclasses import dataclass
from typing import Optional

import numpy as np

import liftover_expect as lx
from portello_amd import abi

STRAND_LIFT = abi.STAGE_STRAND | abi.STAGE_LIFTOVER
N_A, N_B, N_K = 299, 39, 40
TAIL = 6  # contig bases behind the last key of A, B (a trailing clip of the contig's alignment)

# name -> (position on the chromosome, the contig segment's CIGAR)
MAPS = {
    "J": (1000, "10M1D10M10000D10M"),                      # keys 0 10 20 30: a jump of 1 and one of 10 000
    "U": (2000, "5S10M5I10M3I2D10M4D6I10M5S"),             # keys 5 15 20 30 33 43 49 59: unmapped blocks, I D and D I neighbours, clips
    "Z": (3000, "12S"),                                    # no match: no key (kv0 == kv1)
    "K": (5000, "1M1D" * N_K),                             # keys 0 .. 40, every one a jump of 1
    "KS": (8000, "2S" + "1M1D" * N_K),                     # keys 2 .. 42, the same behind a leading clip
    "O": (4000, "30M"),                                    # keys 0 30: one block
    "A": (6000, "1M1D" * N_A + f"{TAIL}S"),                # keys 0 .. 299, 6 bases behind the last
    "B": (7000, "1M1D" * N_B + f"{TAIL}S"),                # keys 0 .. 39, 6 bases behind the last
}
_ORDER = [(m, f) for m in ("J", "U", "Z", "K", "KS", "O") for f in (1, 0)] + [("A", 1), ("B", 1), ("A", 0), ("B", 0)]
CONTIG = {(m, f): k for k, (m, f) in enumerate(_ORDER)}
CHROM_LEN = 12000


def contig_len(m):
    return lx.read_span(lx.parse(MAPS[m][1]))


def make_index() -> abi.IndexData:
    rng = np.random.default_rng(2024)
    acgt = np.frombuffer(b"ACGT", np.uint8)
    cigs = [[(n << 4) | c for n, c in lx.parse(MAPS[m][1])] for m, _ in _ORDER]
    coff = np.zeros(len(cigs) + 1, np.uint32)
    coff[1:] = np.cumsum([len(c) for c in cigs])
    n = len(_ORDER)
    return abi.IndexData(contig_len=[contig_len(m) for m, _ in _ORDER], contig_seg_off=list(range(n + 1)), seg_chrom_index=[k % 2 for k in range(n)],
                         seg_pos=[MAPS[m][0] for m, _ in _ORDER], seg_is_fwd_strand=[f for _, f in _ORDER], seg_mapq=[10 + k for k in range(n)],
                         seg_seq_order_start=[0] * n, seg_seq_order_end=[contig_len(m) for m, _ in _ORDER], seg_cigar_off=coff,
                         seg_cigar=np.array(sum(cigs, []), np.uint32), chrom_seq=[acgt[rng.integers(0, 4, CHROM_LEN)] for _ in range(2)],
                         rev_contig_seq=[acgt[rng.integers(0, 4, contig_len(m))] for m, _ in _ORDER])


INDEX = make_index()
KV0 = {}  # (map, fwd) -> index of the map's first key in ix.kv, by the order above
_at = 0
for _m, _f in _ORDER:
    KV0[(_m, _f)] = _at
    _at += len(lx.tree_map(MAPS[_m][0], lx.parse(MAPS[_m][1]))[0])
N_KV = _at


class Builder:
    """read segments one by one, each with a read of its own whose length is its CIGAR's read span; a placement is given in the map's own
    coordinates and mirrored for a reverse contig"""

    def __init__(self, seed=3):
        self.rng = np.random.default_rng(seed)
        self.read_rev, self.read_len, self.read_off, self.seq, self.nbytes = [], [], [], [], 0
        self.s_read, self.s_contig, self.s_pos, self.s_fwd, self.coff, self.ops = [], [], [], [], [0], []

    def place(self, m, fwd, start, ops):
        """ops: text or [(len, op)]"""
        ops = lx.parse(ops) if isinstance(ops, str) else list(ops)
        if not fwd:
            start, ops = contig_len(m) - (start + lx.ref_span(ops)), ops[::-1]
        assert start >= 0
        n = lx.read_span(ops)
        self.read_rev.append(len(self.s_read) % 2), self.read_len.append(n), self.read_off.append(self.nbytes)
        self.seq.append(np.frombuffer(b"ACGT", np.uint8)[self.rng.integers(0, 4, n)])
        self.nbytes += n
        self.s_read.append(len(self.s_read)), self.s_contig.append(CONTIG[(m, fwd)]), self.s_pos.append(start), self.s_fwd.append(1)
        self.ops += [(n_ << 4) | c for n_, c in ops]
        self.coff.append(len(self.ops))

    def batch(self) -> abi.BatchData:
        return abi.BatchData(read_is_reverse=self.read_rev, read_seq_len=self.read_len, read_seq_off=self.read_off,
                             seq=np.concatenate(self.seq) if self.seq else np.zeros(0, np.uint8), seq_fmt=abi.SEQ_ASCII, seg_read=self.s_read,
                             seg_contig=self.s_contig, seg_pos=np.array(self.s_pos, np.int64), seg_is_fwd_strand=self.s_fwd, seg_cigar_off=self.coff,
                             cigar=np.array(self.ops, np.uint32))


@dataclass
class Case:
    name: str
    batch: abi.BatchData
    why: str
    family: str
    fwd: int
    expected: Optional[list] = None      # family P: per item None or (pos, CIGAR text), by hand (STRAND | LIFTOVER)
    names: Optional[list] = None         # family P: the placements' names, item order
    light: bool = False                  # family S: a group of light items of one class -> exactly one group of the lane kernel
    heavy: bool = False                  # family S: items for the heavy routes (lane_max_w = HEAVY_MAX_W)
    stream: bool = False                 # family S: the restaging case of the streaming kernel


# ---- family P --------------------------------------------------------------------------------------------------------------------------

def _k(n):
    """an M op of K across n further keys: 1M, then a jump deletion and 1M per key"""
    return "1M" + "1D1M" * n


P = [
    # (name, map, start, CIGAR, expected by hand, what it is there for)
    # -- a reference-consuming op that starts / ends at key - 1, key, key + 1 (J: keys 0 10 20 30 -> 1000 1011 11021 None)
    ("start_key_m1", "J", 9, "5M", (1009, "1M1D4M"), "starts one in front of key 10: one base in the old block, the jump, four in the new"),
    ("start_key", "J", 10, "5M", (1011, "5M"), "starts on key 10: the block of key 10 is the first, no deletion (ref2_end_pos is None)"),
    ("start_key_p1", "J", 11, "5M", (1012, "5M"), "starts one behind key 10"),
    ("end_key_m1", "J", 14, "5M", (1015, "5M"), "ends one in front of key 20"),
    ("end_key", "J", 15, "5M", (1016, "5M"), "ends ON key 20: the range query excludes its end, the block is not entered"),
    ("end_key_p1", "J", 16, "5M", (1017, "4M10000D1M"), "ends one behind key 20: the jump of 10 000 as a later piece"),
    ("first_piece_big_jump", "J", 20, "5M", (11021, "5M"), "the block behind the jump of 10 000 as the item's first mapped piece: no deletion"),
    ("end_on_block_start_1", "J", 8, "2M", (1008, "2M"), "the op ends exactly at the first base of the block behind the jump of 1"),
    ("end_behind_block_start_1", "J", 8, "3M", (1008, "2M1D1M"), "... and one base behind it"),
    ("end_on_block_start_10k", "J", 18, "2M", (1019, "2M"), "the op ends exactly at the first base of the block behind the jump of 10 000"),
    ("end_behind_block_start_10k", "J", 18, "3M", (1019, "2M10000D1M"), "... and one base behind it"),
    # -- each reference-consuming kind astride a key
    ("eq_astride", "J", 8, "4=", (1008, "2M1D2M"), "= astride key 10: pieces are written as M"),
    ("x_astride", "J", 8, "4X", (1008, "2M1D2M"), "X astride key 10"),
    ("d_astride_1", "J", 5, "3M4D3M", (1005, "3M5D3M"), "a read D astride the jump of 1: D pieces and the jump sum"),
    ("n_astride_1", "J", 5, "3M4N3M", (1005, "3M2N1D2N3M"), "a read N astride the jump of 1: N pieces stay N around the jump's D"),
    ("d_astride_10k", "J", 16, "2M4D2M", (1017, "2M10004D2M"), "a read D astride the jump of 10 000"),
    ("n_astride_10k", "J", 16, "2M4N2M", (1017, "2M2N10000D2N2M"), "a read N astride the jump of 10 000"),
    ("zero_length_on_key", "J", 7, "3M0M0=0X0D0N3M", (1007, "3M1D3M"), "zero-length M = X D N standing on key 10: empty range queries, nothing emitted"),
    ("match_run_astride", "J", 7, "2=2X2M", (1007, "3M1D3M"), "= X M that LOAD merges into one run, astride key 10"),
    ("pad_and_hard_clip", "J", 4, "2H3S4M2P4M1H", (1004, "2H3S6M1D2M1H"), "P emits nothing, H and S are copied"),
    ("copied_between_pieces", "J", 6, "4M2I4M", (1006, "4M2I1D4M"), "an I copied between the last piece of one block and the jump into the next"),
    ("s_between_pieces", "J", 6, "4M2S1H4M", (1006, "4M2S1H1D4M"), "S and H copied between two pieces (as the reference copies them, wherever they stand)"),
    # -- in front of ref2_start_pos
    ("lead_d_dropped", "J", 8, "4D3M", (1013, "3M"), "a leading D astride the jump: no piece and no deletion is emitted although both lengths are > 0"),
    ("lead_n_dropped", "J", 8, "4N3M", (1013, "3M"), "the same with N"),
    ("lead_d_ends_on_key", "J", 8, "2D3M", (1012, "3M"),
     "a leading D that ends on key 10: it sets ref2_end_pos, so the M behind it emits the jump's 1D in front of the first match; the edge clean-up drops it and adds its length: pos = r2s + lead_shift = 1011 + 1"),
    ("lead_i_behind_s", "U", 20, "2S3I2D4M", (2012, "5S4M"), "leading S I D: the D is dropped by the lift, the I becomes S in the edge clean-up"),
    ("trail_i_d", "U", 20, "4M2I3D", (2010, "4M2S"), "trailing I and D: the I becomes S, the D a zero-length S that compress drops"),
    ("trail_d_over_jump", "J", 8, "2M3D", (1008, "2M"), "a trailing D astride the jump: the jump's D and the D pieces all go"),
    # -- unmapped blocks (U: keys 5 15 20 30 33 43 49 59 -> 2000 None 2010 None 2022 None 2036 None)
    ("m_over_unmapped", "U", 10, "15M", (2005, "5M5I5M"), "a match over an unmapped block gives I; the block behind it follows without a jump"),
    ("d_over_unmapped", "U", 10, "3M9D3M", (2005, "3M4D3M"), "a D over an unmapped block gives nothing for it"),
    ("inside_unmapped", "U", 16, "3M", None, "an item inside an unmapped block: I only, NO_LIFTOVER"),
    ("i_d_neighbours", "U", 25, "12M", (2015, "5M3I2D4M"), "3I2D in the contig's CIGAR: a deletion behind an unmapped block"),
    ("d_i_neighbours", "U", 40, "12M", (2029, "3M6I4D3M"), "4D6I in the contig's CIGAR: the same"),
    # -- in front of the first key, behind the last
    ("astride_first_key", "U", 2, "6M", (2000, "3S3M"), "positions in front of the first key give S (no block: the query starts at the op's start)"),
    ("wholly_in_front", "U", 0, "4M", None, "an item wholly in front of the first key: S only, NO_LIFTOVER"),
    ("wholly_behind", "U", 60, "3M", None, "an item wholly behind the last key: I only, NO_LIFTOVER"),
    ("astride_last_key", "U", 55, "7M", (2042, "4M3S"), "runs on past the last key: I, which the edge clean-up turns into S"),
    ("no_match_map", "Z", 3, "4M", None, "a contig segment without a match: no key (kv0 == kv1), NO_LIFTOVER"),
    ("one_block_map", "O", 5, "4M1D3M2I2M", (4005, "4M1D3M2I2M"), "a map of one block: the identity"),
    # -- a start that the shift stage moves past keys on the reverse contig (K: key i -> 5000 + 2 i).  As written (no shift stage) the D
    #    sets ref2_end_pos and the first match emits the jump's D in front of itself: lead_shift 1
    ("shift_past_one_key", "K", 4, "1D6M", (5011, _k(5)), "a leading D of 1 from key 4: the left shift strips it and the start moves past key 5"),
    ("shift_past_two_keys", "K", 4, "2D6M", (5013, _k(5)), "a leading D of 2 from key 4: past keys 5 and 6 (lane_core.hpp: 'the shift stage moved the start past another key')"),
    # -- an M op across n keys, every key a jump
] + [
    (f"m_across_{n}", "K", 3, f"{n + 1}M", (5006, _k(n)), f"an M across {n} keys, every one a jump: {1 + 2 * n} ops from one") for n in (1, 2, 7, 8, 9, 16, 17, 33)
] + [
    # W0 = kv0 without a block that holds the start, W1 - W0 = 34: S, M and (D, M) for 33 more keys = 68 ops = lane_region_gap(W0, W1)
    # EXACTLY -- the whole allowance of two ops per key, which an item that starts inside a block (m_across_*: 2 (W1 - W0) - 1) leaves
    # one short.  lane_region_dwords is the input op, the gap and LANE_SLACK more: 71 dwords for 68 ops out.
    ("most_ops_per_key", "KS", 0, "36M", (8000, "2S" + _k(33)), "the most output ops per key: attains lane_region_gap exactly; must be lifted by the lane kernel (no retry)"),
]
P_NAMES = [p[0] for p in P]


def cases_p():
    out = []
    for fwd in (1, 0):
        b = Builder(seed=7 + fwd)
        for _, m, start, ops, _, _ in P:
            b.place(m, fwd, start, ops)
        out.append(Case(f"P_{'fwd' if fwd else 'rev'}", b.batch(), "every placement of family P on the " + ("forward" if fwd else "reverse") + " contigs",
                        "P", fwd, expected=[p[4] for p in P], names=P_NAMES))
    return out


def golden_vectors():
    """what tests/golden/liftover_vectors.json holds: the maps and the placements with their hand-written expectations"""
    return {"_about": "Hand-worked expectations of the liftover stage at block-map edges (tests/liftover_cases.py, family P): inputs and expected outputs only.",
            "maps": {m: {"pos": p, "cigar": c} for m, (p, c) in MAPS.items() if m in {q[1] for q in P}},
            "liftover": [{"id": name, "map": m, "start": start, "cigar": ops, "expect": None if e is None else {"pos": e[0], "cigar": e[1]}, "why": why}
                         for name, m, start, ops, e, why in P]}


# ---- family S --------------------------------------------------------------------------------------------------------------------------

HEAVY_MAX_W = 4  # lane_max_w / PLO_LANE_MAX_W of the heavy routes: every item with a reference-consuming op is heavy (region >= 1 + 2 + 2)


def _group(name, fwd, places, why, kvs=128, **kw):
    assert len(places) <= 64
    b = Builder(seed=11)
    for m, start, ops in places:
        b.place(m, fwd, start, ops)
    return Case(f"{name}{'' if kvs == 128 else f'_kvs{kvs}'}_{'fwd' if fwd else 'rev'}", b.batch(), why, "S", fwd, **kw)


def cases_s_light(kvs=128):
    """groups of light items: 1M items, window [p, p + 1), the cursor asks for entries p .. p + 2 (need_hi = p + 3)"""
    out = []
    for fwd in (1, 0):
        for d in (kvs - 1, kvs, kvs + 1):
            tag = {kvs - 1: "m1", kvs: "eq", kvs + 1: "p1"}[d]
            far = d - 3
            out.append(_group(f"S_near63_far1_{tag}", fwd, [("A", j, "1M") for j in range(63)] + [("A", far, "1M")],
                              f"63 items at A's first keys and one whose need_hi is base + {d} (kvs {kvs})", kvs, light=True))
            out.append(_group(f"S_near1_far63_{tag}", fwd, [("A", 0, "1M")] + [("A", far - j, "1M") for j in range(63) if far - j > 0],
                              f"one item at A's first key and up to 63 whose need_hi ends at base + {d}", kvs, light=True))
            # the far item on B: B's first key is entry 300 of A's numbering, the item at B 10 asks up to 313; the near items stand at s ..
            s = N_A + 1 + 13 - d
            out.append(_group(f"S_nearA_farB_{tag}", fwd, [("A", j, "1M") for j in range(s, min(s + 63, N_A))] + [("B", 10, "1M")],
                              f"near items from A {s} and one item on B whose need_hi is base + {d}", kvs, light=True))
        # map end: windows that end at the last key, the last op past it; neighbours on the other map's first keys
        for m, n, other in (("A", N_A, "B"), ("B", N_B, "A")):
            places = [(m, n - 2, "4M"), (m, n - 3, "3M"), (m, n - 4, "3M"), (m, n - 1, "3M"), (m, n, "2M"), (m, n + TAIL - 1, "1M")]
            places += [(other, j, "2M") for j in range(8)] if (m, other) == ("A", "B") else [(other, N_A - 1 - j, "2M") for j in range(8)]
            out.append(_group(f"S_map_end_{m}", fwd, places,
                              f"W1 == kv1, W1 + 1 == kv1, W1 + 2 == kv1 at {m}'s last key, items on and behind it, neighbours on {other}" +
                              ("; B_r's last key is the last word of ix.kv" if m == "B" else ""), light=True))
    return out


def cases_s_heavy(kvs=128):
    """a single item whose own window needs kvs - 2 .. kvs + 1 and 200 entries (nM at A 10: n + 2 entries), alone and in front of 63 short heavy
    items; heavy by construction (region 1 + 2 n + 2 > lane_max_w of any route)"""
    out = []
    for fwd in (1, 0):
        for need in (kvs - 2, kvs - 1, kvs, kvs + 1, 200):
            n = need - 2
            out.append(_group(f"S_heavy_need{need}_alone", fwd, [("A", 10, f"{n}M")], f"one heavy item whose window needs {need} entries", kvs, heavy=True))
            out.append(_group(f"S_heavy_need{need}_beside63", fwd, [("A", 10, f"{n}M")] + [("A", 10 + j, "1M") for j in range(63)],
                              "the same in front of 63 short heavy items", kvs, heavy=True))
    return out


def cases_s_stream():
    """One team of the streaming kernel (lane_heavy_per = the item count; the harness's teams are 64 lanes wide whatever the count): a 120-key
    item from A 150 is under way while its neighbour lanes finish short items and take new ones -- at a lower W0 (base drops to A 0: the long
    item's entries leave the 128 staged ones, its kv_lds goes off), then far above it and on B (base is the long item's W0 again: on).  A
    window of 250 keys could never be staged (LANE_KVS = 128), so it could not flip; 120 can.  In teams of 64 items (lane_heavy_per 64; on the card
    also 5) no lane takes a second item: those routes check results only."""
    out = []
    for fwd in (1, 0):
        places = [("A", 150, "120M")] + [("A", 150 + j, "3M") for j in range(63)]
        places += [("A", j % 20, "3M") for j in range(40)] + [("A", 280 + j % 10, "3M") for j in range(40)] + [("B", j % 30, "3M") for j in range(40)]
        b = Builder(seed=13)
        for m, start, ops in places:
            b.place(m, fwd, start, ops)
        out.append(Case(f"S_stream_restage_{'fwd' if fwd else 'rev'}", b.batch(), "a long item mid-way while the team restages below it, above it and on B", "S", fwd, stream=True))
    return out


def all_cases(kvs=128):
    return cases_p() + cases_s_light(kvs) + cases_s_heavy(kvs) + cases_s_stream()
