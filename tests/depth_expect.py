"""What plo_depth_* must produce, restated from the rule in include/portello_liftover.h ("Depth of the records") in plain Python -- not derived
from the code under test: which records count, a record's real CIGAR, the bases it covers, the layout of the array, the lowest record an
add refuses and the kind it breaks, the depths, the window sums, the runs and the text of the two BED files.  The depths are counted base by
base (an increment per covered base), not through differences and a scan.
TEST INFRASTRUCTURE ONLY."""
import struct

import numpy as np

import index_expect as ix

ERR_OFFSET, ERR_SHORT, ERR_BLOCK, ERR_REFID, ERR_POS, ERR_CIGAR, ERR_AUX, ERR_END = 1, 2, 3, 4, 5, 6, 7, 8
EXCLUDE_DEFAULT = 0x704
SLOT_ALIGN = 64
RUN = np.dtype([("ref_id", "<i4"), ("beg", "<i4"), ("end", "<i4"), ("depth", "<i4")])
COVER, REF = (0, 7, 8), (0, 2, 3, 7, 8)
_AUX_SIZE = {b"A": 1, b"c": 1, b"C": 1, b"s": 2, b"S": 2, b"i": 4, b"I": 4, b"f": 4, b"d": 8}


def slot_off(ref_len):
    """first entry of every slot and, last, the entries of the array"""
    off = [0]
    for n in ref_len:
        off.append(off[-1] + (n + 1 + SLOT_ALIGN - 1) // SLOT_ALIGN * SLOT_ALIGN)
    return off


def aux_field_len(rec, a):
    """length of the aux field at rec[a:], or 0 when it is malformed or leaves the record (SAMv1 4.2.4)"""
    room = len(rec) - a
    if room < 3:
        return 0
    t = rec[a + 2:a + 3]
    if t in _AUX_SIZE:
        n = _AUX_SIZE[t]
    elif t in (b"Z", b"H"):
        z = rec.find(b"\0", a + 3)
        if z < 0:
            return 0
        n = z - (a + 3) + 1
    elif t == b"B":
        if room < 8:
            return 0
        es = _AUX_SIZE.get(rec[a + 3:a + 4], 0)
        if es not in (1, 2, 4):
            return 0
        n = 5 + es * struct.unpack_from("<I", rec, a + 4)[0]
    else:
        return 0
    return 3 + n if 3 + n <= room else 0


def real_cigar(rec):
    """the record's real CIGAR as a list of words, or ERR_AUX.  The in-record CIGAR must lie inside rec."""
    ref, pos, lrn, ncig, flag = ix.fields(rec)
    ops = list(struct.unpack_from("<%dI" % ncig, rec, 36 + lrn))
    l_seq = struct.unpack_from("<I", rec, 20)[0]
    if not (ncig == 2 and ops[0] == ix.op(l_seq, 4) and ops[1] & 15 == 3):
        return ops
    a = 36 + lrn + 8 + (l_seq + 1) // 2 + l_seq
    if a > len(rec):
        return ERR_AUX
    while a < len(rec):
        n = aux_field_len(rec, a)
        if not n:
            return ERR_AUX
        if rec[a:a + 2] == b"CG":
            if rec[a + 2:a + 4] == b"BI":
                return list(struct.unpack_from("<%dI" % struct.unpack_from("<I", rec, a + 4)[0], rec, a + 8))
            return ops
        a += n
    return ops


def counted(rec, exclude=EXCLUDE_DEFAULT):
    ref, pos, _lrn, _ncig, flag = ix.fields(rec)
    return ref >= 0 and pos >= 0 and flag & exclude == 0


def covered(ops, pos, deletions=False):
    """([(beg, end)] of the covering ops in order, the reference end)"""
    out = []
    for o in ops:
        n, c = o >> 4, o & 15
        if n == 0:
            continue
        if c in COVER or (c == 2 and deletions):
            out.append((pos, pos + n))
        if c in REF:
            pos += n
    return out, pos


def first_offender(data, off, ref_len, exclude=EXCLUDE_DEFAULT):
    """(record, kind) of the lowest record an add refuses, or None"""
    n, n_bytes, n_ref = len(off) - 1, len(data), len(ref_len)
    for i in range(n):
        a, b = int(off[i]), int(off[i + 1])
        if (i == 0 and a != 0) or b < a or b > n_bytes or (i == n - 1 and b != n_bytes):
            return i, ERR_OFFSET
        if b - a < 36:
            return i, ERR_SHORT
        rec = data[a:b]
        if struct.unpack_from("<I", rec, 0)[0] + 4 != b - a:
            return i, ERR_BLOCK
        ref, pos, lrn, ncig, flag = ix.fields(rec)
        if not -1 <= ref < n_ref:
            return i, ERR_REFID
        if not -1 <= pos <= ix.POS_MAX:
            return i, ERR_POS
        if 36 + lrn + 4 * ncig > b - a:
            return i, ERR_CIGAR
        ops = real_cigar(rec)
        if ops == ERR_AUX:
            return i, ERR_AUX
        if counted(rec, exclude) and covered(ops, pos)[1] > ref_len[ref]:
            return i, ERR_END
    return None


def depths(records, ref_len, exclude=EXCLUDE_DEFAULT, deletions=False):
    """per chromosome an int64 array of ref_len depths, and the number of counted records; every record must be acceptable"""
    out = [np.zeros(n, np.int64) for n in ref_len]
    n_counted = 0
    for rec in records:
        if not counted(rec, exclude):
            continue
        n_counted += 1
        ref, pos = ix.fields(rec)[:2]
        for a, b in covered(real_cigar(rec), pos, deletions)[0]:
            out[ref][a:b] += 1
    return out, n_counted


def array(dep, ref_len):
    """the finished array: the depths in their slots, zero everywhere else"""
    off = slot_off(ref_len)
    a = np.zeros(off[-1], np.int32)
    for r, d in enumerate(dep):
        a[off[r]:off[r] + len(d)] = d
    return a


def differences(dep, ref_len):
    """the open array: d[b] - d[b - 1] in every slot, the extra entry taking -d[last]"""
    off = slot_off(ref_len)
    a = np.zeros(off[-1], np.int32)
    for r, d in enumerate(dep):
        ext = np.concatenate([[0], d, [0]])
        a[off[r]:off[r] + len(d) + 1] = np.diff(ext)
    return a


def windows(dep, w):
    """(win_first [n_ref + 1], the sums): chromosome r has ceil(ref_len[r] / w) windows, the last one short"""
    first, sums = [0], []
    for d in dep:
        k = (len(d) + w - 1) // w
        first.append(first[-1] + k)
        sums += [int(d[j * w:(j + 1) * w].sum()) for j in range(k)]
    return np.array(first, np.uint64), np.array(sums, np.uint64)


def runs(dep):
    """maximal stretches of equal depth inside a chromosome, zero-depth ones too, ordered by (ref_id, beg)"""
    out = []
    for r, d in enumerate(dep):
        beg = 0
        for b in range(1, len(d) + 1):
            if b == len(d) or d[b] != d[beg]:
                out.append((r, beg, b, int(d[beg])))
                beg = b
    return np.array(out, RUN) if out else np.zeros(0, RUN)


def per_base_text(names, run_arr):
    return "".join("%s\t%d\t%d\t%d\n" % (names[int(r["ref_id"])], r["beg"], r["end"], r["depth"]) for r in run_arr)


def mean_text(total, n):
    """total / n with two decimals, round-half-even on the exact quotient (integer arithmetic: no float enters)"""
    q, rem = divmod(100 * total, n)
    if 2 * rem > n or (2 * rem == n and q & 1):
        q += 1
    return "%d.%02d" % (q // 100, q % 100)


def regions_text(names, ref_len, w, win_first, sums):
    out = []
    for r, n in enumerate(ref_len):
        for j in range(int(win_first[r + 1]) - int(win_first[r])):
            beg, end = j * w, min(n, (j + 1) * w)
            out.append("%s\t%d\t%d\t%s\n" % (names[r], beg, end, mean_text(int(sums[int(win_first[r]) + j]), end - beg)))
    return "".join(out)
