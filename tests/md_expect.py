"""MD:Z as samtools calmd writes it (bam_md.c, bam_fillmd1_core), restated from the rule (not from the device code), over an output
record's own bytes.

A counter u of matched bases starts at 0.  M, = and X go base by base; a pair matches exactly as for NM (nm_expect: with c1 the read's
4-bit code and c2 the reference byte's code in "=ACMGRSVTWYHKDBN", any other byte 15, iff c1 == 0, or c1 == c2 and c1 != 15).  A match
does u += 1; a mismatch writes u in decimal (also 0), then the reference letter, and sets u = 0.  A D of length > 0 writes u (also 0), '^',
its reference letters, and sets u = 0.  I, S, N, H, P write nothing and keep u (I and S advance the read, N the reference); ops of length
0 are skipped.  At the end u is written.  The reference letter is the chromosome's byte: A..Z as it is, a..z upper-cased, any other
byte 'N'.

Together with plo_records_build on the same window this is the yardstick of the MD feature: neither touches the code under test.
TEST INFRASTRUCTURE ONLY."""
import re
import struct

import numpy as np

import nm_expect as nx

GRAMMAR = re.compile(rb"[0-9]+(([A-Z]|\^[A-Z]+)[0-9]+)*")
LETTER = np.full(256, ord("N"), np.uint8)
for _b in range(ord("A"), ord("Z") + 1):
    LETTER[_b] = _b
    LETTER[_b + 32] = _b


def md_text(ops, codes: np.ndarray, ref: np.ndarray, pos: int) -> bytes:
    """the text, the bases of all ops at once; IndexError when the CIGAR leaves the read or the chromosome"""
    ops = np.asarray(ops, np.uint32)
    ref = np.asarray(ref)
    t, l = (ops & 15).astype(np.int64), (ops >> 4).astype(np.int64)
    rd_adv, rf_adv = np.where(np.isin(t, nx._READ_OPS), l, 0), np.where(np.isin(t, nx._REF_OPS), l, 0)
    if int(rd_adv.sum()) > len(codes) or pos < 0 or pos + int(rf_adv.sum()) > len(ref):
        raise IndexError("the CIGAR leaves the read or the chromosome")
    rd0, rf0 = np.cumsum(rd_adv) - rd_adv, pos + np.cumsum(rf_adv) - rf_adv
    sel = (np.isin(t, nx._CMP_OPS) | (t == 2)) & (l > 0)  # the ops that yield tokens: one per reference base, in the text's order
    ls = l[sel]
    total = int(ls.sum())
    if not total:
        return b"0"
    within = np.arange(total) - np.repeat(np.cumsum(ls) - ls, ls)
    is_del = np.repeat(t[sel] == 2, ls)
    rf = np.repeat(rf0[sel], ls) + within
    rd = np.where(is_del, 0, np.repeat(rd0[sel], ls) + within)
    c1 = np.where(is_del, 0, codes[rd] if len(codes) else 0)
    c2 = nx.CODE_OF[ref[rf]]
    match = ~is_del & ((c1 == 0) | ((c1 == c2) & (c1 != 15)))
    letters = LETTER[ref[rf]]
    first_del = is_del & (within == 0)
    closes = (~match & ~is_del) | first_del  # the tokens in front of which u is written
    cm = np.cumsum(match)  # matches up to and including token k
    ev = np.flatnonzero(~match)  # mismatches and every deleted base
    # u in front of event k: the matches since the event before it
    before = cm[ev]
    u = before - np.concatenate([[0], before[:-1]])
    out = []
    for k, e in enumerate(ev):
        if closes[e]:
            out.append(b"%d" % int(u[k]))
            if first_del[e]:
                out.append(b"^")
        out.append(bytes([int(letters[e])]))
    out.append(b"%d" % (int(cm[-1]) - (int(before[-1]) if len(ev) else 0)))
    return b"".join(out)


def md_slow(ops, codes, ref, pos) -> bytes:
    """the same, one base at a time (the hand-made cases are written both ways)"""
    out = bytearray()
    u = rd = 0
    rf = pos
    for op in ops:
        t, l = int(op) & 15, int(op) >> 4
        if l == 0:
            continue
        if t in nx._CMP_OPS:
            for k in range(l):
                c1, b = int(codes[rd + k]), int(ref[rf + k])
                c2 = int(nx.CODE_OF[b])
                if c1 == 0 or (c1 == c2 and c1 != 15):
                    u += 1
                else:
                    out += b"%d" % u
                    out.append(b if 65 <= b <= 90 else b - 32 if 97 <= b <= 122 else 78)
                    u = 0
            rd += l
            rf += l
        elif t == 2:
            out += b"%d^" % u
            for k in range(l):
                b = int(ref[rf + k])
                out.append(b if 65 <= b <= 90 else b - 32 if 97 <= b <= 122 else 78)
            u = 0
            rf += l
        elif t == 1 or t == 4:
            rd += l
        elif t == 3:
            rf += l
    out += b"%d" % u
    return bytes(out)


def n_letters(text: bytes) -> int:
    """the letters of a text, those behind '^' too (with the I lengths: the item's NM)"""
    return sum(1 for b in text if 65 <= b <= 90)


def md_of_record(rec: bytes, chroms) -> bytes:
    """the text of an output record against chroms[refID] (uint8 arrays)"""
    tid, pos, _, ops, codes = nx.record_alignment(rec)
    return md_text(ops, codes, chroms[tid], pos)


def _resize(body: bytes) -> bytes:
    return struct.pack("<I", len(body) - 4) + body[4:]


def cut_first_md(rec: bytes) -> bytes:
    """the record without the first field tagged MD, whatever its type"""
    for a, n, tag, _ in nx.aux_fields(rec):
        if tag == b"MD":
            return _resize(rec[:a] + rec[a + n:])
    return rec


def splice_md(rec: bytes, text: bytes) -> bytes:
    """a lifted record with MD:Z + text + NUL behind its last ZM:C field, behind the NM:i that directly follows that when there is one"""
    f = nx.aux_fields(rec)
    zm = [k for k, (a, n, tag, t) in enumerate(f) if tag == b"ZM" and t == "C"]
    assert len(zm) >= 1
    k = zm[-1]
    if k + 1 < len(f) and f[k + 1][2] == b"NM" and f[k + 1][3] == "i":
        k += 1
    at = f[k][0] + f[k][1]
    return _resize(rec[:at] + b"MDZ" + text + b"\0" + rec[at:])


def strip_md(rec: bytes):
    """-> (the record without its MD:Z fields, their texts)"""
    vals, keep, cur = [], [], 0
    for a, n, tag, t in nx.aux_fields(rec):
        if tag == b"MD" and t == "Z":
            vals.append(rec[a + 3:a + n - 1])
            keep.append(rec[cur:a])
            cur = a + n
    keep.append(rec[cur:])
    return _resize(b"".join(keep)), vals
