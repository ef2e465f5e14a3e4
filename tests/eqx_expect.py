"""The = / X CIGAR of a lifted record (plo_eqx_dev), restated from the rule (not from the device code), over an output record's own bytes.

Walk the record's CIGAR.  An op with code M, = or X and length L is compared: its L base pairs are classified by the pair rule of NM
(nm_expect: with c1 the read's 4-bit code and c2 the reference byte's code in "=ACMGRSVTWYHKDBN", any other byte 15, a pair matches iff
c1 == 0, or c1 == c2 and c1 != 15), and the op is replaced by its maximal runs, '=' for a run of matching pairs and 'X' for a run of
mismatching pairs, in order.  Runs do not cross op boundaries, so every output op is no longer than the op it came from; a compared op of
length 0 yields nothing.  Every other op (I, D, N, S, H, P, codes 9-15) is copied as it stands, in its place.  Reference length, read
length, pos, bin and the reference end therefore do not change; the bases under X plus the I and D lengths are the item's NM, and the X
positions are the mismatch letters of its MD text that do not stand behind '^'.

Together with plo_records_build on the same window this is the yardstick of the = / X feature: neither touches the code under test.
TEST INFRASTRUCTURE ONLY."""
import re
import struct

import numpy as np

import nm_expect as nx

EQ, X = 7, 8


def eqx_ops(ops, codes: np.ndarray, ref: np.ndarray, pos: int) -> np.ndarray:
    """the rewritten ops, the bases of all compared ops at once; IndexError when the CIGAR leaves the read or the chromosome"""
    ops = np.asarray(ops, np.uint32)
    ref = np.asarray(ref)
    t, l = (ops & 15).astype(np.int64), (ops >> 4).astype(np.int64)
    rd_adv, rf_adv = np.where(np.isin(t, nx._READ_OPS), l, 0), np.where(np.isin(t, nx._REF_OPS), l, 0)
    if int(rd_adv.sum()) > len(codes) or pos < 0 or pos + int(rf_adv.sum()) > len(ref):
        raise IndexError("the CIGAR leaves the read or the chromosome")
    rd0, rf0 = np.cumsum(rd_adv) - rd_adv, pos + np.cumsum(rf_adv) - rf_adv
    where = np.arange(len(ops))
    sel = np.isin(t, nx._CMP_OPS)
    other = where[~sel]  # the ops that are copied
    sel &= l > 0
    ls = l[sel]
    total = int(ls.sum())
    if not total:
        return ops[other].astype(np.uint32)
    within = np.arange(total) - np.repeat(np.cumsum(ls) - ls, ls)
    c1 = codes[np.repeat(rd0[sel], ls) + within]
    c2 = nx.CODE_OF[ref[np.repeat(rf0[sel], ls) + within]]
    mism = ~((c1 == 0) | ((c1 == c2) & (c1 != 15)))
    first = within == 0  # a run starts with its op, and where the kind changes
    first[1:] |= mism[1:] != mism[:-1]
    starts = np.flatnonzero(first)
    lens = np.diff(np.concatenate([starts, [total]]))
    runs = ((lens << 4) | np.where(mism[starts], X, EQ)).astype(np.uint32)
    run_op = np.repeat(where[sel], ls)[starts]  # the op a run came from: the runs take its place, in order
    order = np.argsort(np.concatenate([run_op, other]), kind="stable")
    return np.concatenate([runs, ops[other].astype(np.uint32)])[order]


def eqx_slow(ops, codes, ref, pos):
    """the same, one base at a time (the hand-made cases are written both ways)"""
    out = []
    rd, rf = 0, pos
    for op in ops:
        t, l = int(op) & 15, int(op) >> 4
        if t in nx._CMP_OPS:
            run, kind = 0, None
            for k in range(l):
                c1, c2 = int(codes[rd + k]), int(nx.CODE_OF[ref[rf + k]])
                code = EQ if (c1 == 0 or (c1 == c2 and c1 != 15)) else X
                if code != kind and run:
                    out.append((run << 4) | kind)
                    run = 0
                kind = code
                run += 1
            if run:
                out.append((run << 4) | kind)
            rd += l
            rf += l
        else:
            out.append(int(op))
            if t in (1, 4):
                rd += l
            elif t in (2, 3):
                rf += l
    return np.array(out, np.uint32)


def text(ops) -> str:
    return "".join("%d%s" % (int(o) >> 4, "MIDNSHP=X???????"[int(o) & 15]) for o in ops)


def parse(s: str) -> np.ndarray:
    return np.array([(int(n) << 4) | "MIDNSHP=X".index(c) for n, c in re.findall(r"(\d+)([MIDNSHP=X])", s)], np.uint32)


def collapse_to_m(ops) -> np.ndarray:
    """= and X turned into M and adjacent M merged: what the rewrite started from wherever that had no two adjacent compared ops"""
    out = []
    for o in ops:
        t, l = int(o) & 15, int(o) >> 4
        if t in (EQ, X):
            t = 0
        if t == 0 and out and (out[-1] & 15) == 0:
            out[-1] += l << 4
        else:
            out.append((l << 4) | t)
    return np.array(out, np.uint32)


def n_edits(ops) -> int:
    """the bases under X plus the I and D lengths: the item's NM"""
    ops = np.asarray(ops, np.uint32)
    return int((ops >> 4)[np.isin(ops & 15, (X, 1, 2))].sum())


def x_positions(ops):
    """the positions of the bases under X, counted over the bases of M / = / X and D ops (the bases an MD text walks)"""
    at, out = 0, []
    for o in ops:
        t, l = int(o) & 15, int(o) >> 4
        if t == X:
            out.extend(range(at, at + l))
        if t in (0, EQ, X, 2):
            at += l
    return out


def md_mismatch_positions(md: bytes):
    """the positions, counted the same way, of the letters of an MD text that do not stand behind '^'"""
    at, out = 0, []
    for num, dele, letter in re.findall(rb"([0-9]+)|\^([A-Z]+)|([A-Z])", md):
        if num:
            at += int(num)
        elif dele:
            at += len(dele)
        else:
            out.append(at)
            at += 1
    return out


def eqx_of_record(rec: bytes, chroms) -> np.ndarray:
    """the rewritten CIGAR of an output record against chroms[refID] (uint8 arrays)"""
    tid, pos, _, ops, codes = nx.record_alignment(rec)
    return eqx_ops(ops, codes, chroms[tid], pos)


def _resize(body: bytes) -> bytes:
    return struct.pack("<I", len(body) - 4) + body[4:]


def splice_cigar(rec: bytes, new_ops) -> bytes:
    """a lifted record with its CIGAR replaced the way bam_write1 stores one: up to 65535 ops in the record; more as the <l_seq>S<ref_len>N
    placeholder with the ops in a CG:B,I field, the record's last.  The record's own CIGAR may be stored either way."""
    new_ops = np.asarray(new_ops, np.uint32)
    lq, ncg, lseq = rec[12], struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<I", rec, 20)[0]
    c0 = 36 + lq
    old = np.frombuffer(rec, "<u4", ncg, c0)
    body, tail = rec[:c0], rec[c0 + 4 * ncg:]
    if ncg == 2 and int(old[0]) == ((lseq << 4) | 4) and (int(old[1]) & 15) == 3:  # the record's own CG:B,I field, its last, goes
        a, n, tag, t = nx.aux_fields(rec)[-1]
        assert tag == b"CG" and t == "B" and rec[a + 3:a + 4] == b"I"
        tail = rec[c0 + 4 * ncg:a]
    if len(new_ops) <= 0xFFFF:
        cig, cg_field = new_ops.astype("<u4").tobytes(), b""
        n_new = len(new_ops)
    else:
        ref_len = int((new_ops >> 4)[np.isin(new_ops & 15, nx._REF_OPS)].sum())
        cig = struct.pack("<II", (lseq << 4) | 4, (ref_len << 4) | 3)
        cg_field = b"CGBI" + struct.pack("<I", len(new_ops)) + new_ops.astype("<u4").tobytes()
        n_new = 2
    body = body[:16] + struct.pack("<H", n_new) + body[18:]
    return _resize(body + cig + tail + cg_field)
