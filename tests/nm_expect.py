"""NM:i as samtools calmd counts it, restated from the rule (not from the device code), over an output record's own bytes.

M, = and X compare base by base: with c1 the read's 4-bit code and c2 the reference byte's code in "=ACMGRSVTWYHKDBN" (any other byte: 15)
a pair matches iff c1 == 0, or c1 == c2 and c1 != 15; every other pair adds 1.  I adds its length and advances the read, D adds its length
and advances the reference, N advances the reference, S the read, H and P do nothing.

Together with plo_records_build on the same window this is the yardstick of the NM feature: neither touches the code under test.
TEST INFRASTRUCTURE ONLY."""
import struct

import numpy as np

TABLE = b"=ACMGRSVTWYHKDBN"
CODE_OF = np.full(256, 15, np.uint8)
for _i, _ch in enumerate(TABLE):
    CODE_OF[_ch] = _i

_READ_OPS, _REF_OPS, _CMP_OPS = (0, 1, 4, 7, 8), (0, 2, 3, 7, 8), (0, 7, 8)


def codes_of(seq: bytes, l_seq: int) -> np.ndarray:
    """the 4-bit codes of BAM bases, high nibble first"""
    b = np.frombuffer(bytes(seq), np.uint8)
    c = np.empty(2 * len(b), np.uint8)
    c[0::2] = b >> 4
    c[1::2] = b & 15
    assert l_seq <= len(c)
    return c[:l_seq]


def nm_counts(ops, codes: np.ndarray, ref: np.ndarray, pos: int):
    """-> (NM, bases compared); IndexError when the CIGAR leaves the read or the chromosome"""
    ops = np.asarray(ops, np.uint32)
    t, l = (ops & 15).astype(np.int64), (ops >> 4).astype(np.int64)
    rd_adv, rf_adv = np.where(np.isin(t, _READ_OPS), l, 0), np.where(np.isin(t, _REF_OPS), l, 0)
    if int(rd_adv.sum()) > len(codes) or pos < 0 or pos + int(rf_adv.sum()) > len(ref):
        raise IndexError("the CIGAR leaves the read or the chromosome")
    rd0, rf0 = np.cumsum(rd_adv) - rd_adv, pos + np.cumsum(rf_adv) - rf_adv
    nm = int(l[(t == 1) | (t == 2)].sum())
    m = np.isin(t, _CMP_OPS) & (l > 0)
    lm = l[m]
    total = int(lm.sum())
    if total:
        within = np.arange(total) - np.repeat(np.cumsum(lm) - lm, lm)
        c1 = codes[np.repeat(rd0[m], lm) + within]
        c2 = CODE_OF[np.asarray(ref)[np.repeat(rf0[m], lm) + within]]
        match = (c1 == 0) | ((c1 == c2) & (c1 != 15))
        nm += total - int(match.sum())
    return nm, total


def nm_slow(ops, codes, ref, pos):
    """the same, one base at a time (the hand-made cases are counted both ways)"""
    nm = rd = 0
    rf = pos
    for op in ops:
        t, l = int(op) & 15, int(op) >> 4
        if t in _CMP_OPS:
            for k in range(l):
                c1, c2 = int(codes[rd + k]), int(CODE_OF[ref[rf + k]])
                if not (c1 == 0 or (c1 == c2 and c1 != 15)):
                    nm += 1
            rd += l
            rf += l
        elif t == 1:
            nm += l
            rd += l
        elif t == 2:
            nm += l
            rf += l
        elif t == 3:
            rf += l
        elif t == 4:
            rd += l
    return nm


def aux_fields(rec: bytes):
    """(offset, length, tag, type letter) of the aux fields of a record that starts with its block_size word (well-formed records only)"""
    lq, ncg, lseq = rec[12], struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<I", rec, 20)[0]
    a = 36 + lq + 4 * ncg + (lseq + 1) // 2 + lseq
    out = []
    while a < len(rec):
        t = chr(rec[a + 2])
        if t in "AcC":
            n = 4
        elif t in "sS":
            n = 5
        elif t in "iIf":
            n = 7
        elif t == "d":
            n = 11
        elif t in "ZH":
            n = rec.index(b"\0", a + 3) + 1 - a
        elif t == "B":
            n = 8 + {"c": 1, "C": 1, "s": 2, "S": 2, "i": 4, "I": 4, "f": 4}[chr(rec[a + 3])] * struct.unpack_from("<I", rec, a + 4)[0]
        else:
            raise AssertionError(t)
        out.append((a, n, rec[a:a + 2], t))
        a += n
    assert a == len(rec)
    return out


def record_alignment(rec: bytes):
    """-> (refID, pos, flag, ops, codes) of a record that starts with its block_size word; the CIGAR of a CG:B,I field is honoured"""
    assert struct.unpack_from("<I", rec, 0)[0] == len(rec) - 4
    tid, pos = struct.unpack_from("<ii", rec, 4)
    lq, ncg, flag, lseq = rec[12], struct.unpack_from("<H", rec, 16)[0], struct.unpack_from("<H", rec, 18)[0], struct.unpack_from("<I", rec, 20)[0]
    ops = np.frombuffer(rec, "<u4", ncg, 36 + lq)
    if ncg == 2 and int(ops[0]) == ((lseq << 4) | 4) and (int(ops[1]) & 15) == 3:
        for a, n, tag, t in aux_fields(rec):
            if tag == b"CG" and t == "B" and rec[a + 3:a + 4] == b"I":
                ops = np.frombuffer(rec, "<u4", struct.unpack_from("<I", rec, a + 4)[0], a + 8)
                break
    s = 36 + lq + 4 * ncg
    return tid, pos, flag, ops, codes_of(rec[s:s + (lseq + 1) // 2], lseq)


def nm_of_record(rec: bytes, chroms) -> int:
    """NM of an output record against chroms[refID] (uint8 arrays)"""
    tid, pos, _, ops, codes = record_alignment(rec)
    return nm_counts(ops, codes, chroms[tid], pos)[0]


def splice_nm(rec: bytes, value: int) -> bytes:
    """a host-built lifted record with NM:i (7 bytes) directly behind its ZM:C field, block_size + 7"""
    zm = [(a, n) for a, n, tag, t in aux_fields(rec) if tag == b"ZM" and t == "C"]
    assert len(zm) >= 1
    a, n = zm[-1]  # (a ZM the source record carried twice keeps its second one in front of the new one)
    body = rec[:a + n] + b"NMi" + struct.pack("<I", value) + rec[a + n:]
    return struct.pack("<I", len(body) - 4) + body[4:]


def strip_nm(rec: bytes):
    """-> (the record without its NM:i fields, their values)"""
    vals, keep, cur = [], [], 0
    for a, n, tag, t in aux_fields(rec):
        if tag == b"NM" and t == "i":
            vals.append(struct.unpack_from("<I", rec, a + 3)[0])
            keep.append(rec[cur:a])
            cur = a + n
    keep.append(rec[cur:])
    body = b"".join(keep)
    return struct.pack("<I", len(body) - 4) + body[4:], vals
