"""What plo_pileup_* must produce, restated from the rule in include/portello_liftover.h ("Allele pileup and candidate sites") in plain Python
-- not derived from the code under test: the slots of an object, the lowest record an add refuses and the kind it breaks, the counts as a
dict {(ref, pos, ch): n}, the array, the sites and the text of <prefix>.sites.tsv.  The checks 1 .. 8 and the real CIGAR are depth's
(depth_expect.py).
TEST INFRASTRUCTURE ONLY."""
import struct

import numpy as np

import depth_expect as dx
import index_expect as ix

A, C, G, T, N, DEL, INS, CLIP = range(8)
CHANNELS = 8
NAMES = ("A", "C", "G", "T", "N", "DEL", "INS", "CLIP")
ERR_SEQ, ERR_LSEQ = 9, 10
EXCLUDE_DEFAULT = 0x704
MASK_DEFAULT = 0x6F
TABLE = b"=ACMGRSVTWYHKDBN"
SITE = np.dtype([("ref_id", "<i4"), ("pos", "<i4"), ("depth", "<i4"), ("ref_base", "u1"), ("pad", "u1", (3,)), ("count", "<i4", (8,))])
assert SITE.itemsize == 48
READ_OPS = (0, 1, 4, 7, 8)  # M I S = X


class Refused(Exception):
    """what plo_pileup_create refuses"""


def slots(ref_len, regions=None):
    """(slot_beg, slot_end, slot_off in bases [n_ref + 1]); regions: [(ref_id, beg, end)] or None"""
    if any(n < 0 for n in ref_len):
        raise Refused("a negative length")
    beg, end = [0] * len(ref_len), list(ref_len)
    if regions:
        beg, end = [0] * len(ref_len), [0] * len(ref_len)
        seen = set()
        for r, b, e in regions:
            if not 0 <= r < len(ref_len):
                raise Refused("ref_id")
            if b < 0 or b > e or e > ref_len[r]:
                raise Refused("bounds")
            if r in seen:
                raise Refused("two regions")
            seen.add(r)
            beg[r], end[r] = b, e
    off = [0]
    for b, e in zip(beg, end):
        off.append(off[-1] + e - b)
    return beg, end, off


def seq_of(rec):
    """the 4-bit codes of the record's l_seq bases"""
    _ref, _pos, lrn, ncig, _flag = ix.fields(rec)
    l_seq = struct.unpack_from("<I", rec, 20)[0]
    at = 36 + lrn + 4 * ncig
    raw = rec[at:at + (l_seq + 1) // 2]
    return [(raw[k >> 1] >> 4) if k % 2 == 0 else (raw[k >> 1] & 15) for k in range(l_seq)]


def pair_matches(c1, ref_byte):
    c2 = TABLE.find(bytes([ref_byte]))
    if c2 < 0:
        c2 = 15
    return c1 == 0 or (c1 == c2 and c1 != 15)


def channel(c1):
    return {1: A, 2: C, 4: G, 8: T}.get(c1, N)


def first_offender(data, off, ref_len, exclude=EXCLUDE_DEFAULT):
    """(record, kind) of the lowest record an add refuses, or None; a record reports the first kind it breaks"""
    n, n_bytes, n_ref = len(off) - 1, len(data), len(ref_len)
    for i in range(n):
        a, b = int(off[i]), int(off[i + 1])
        if (i == 0 and a != 0) or b < a or b > n_bytes or (i == n - 1 and b != n_bytes):
            return i, dx.ERR_OFFSET
        if b - a < 36:
            return i, dx.ERR_SHORT
        rec = data[a:b]
        if struct.unpack_from("<I", rec, 0)[0] + 4 != b - a:
            return i, dx.ERR_BLOCK
        ref, pos, lrn, ncig, _flag = ix.fields(rec)
        if not -1 <= ref < n_ref:
            return i, dx.ERR_REFID
        if not -1 <= pos <= ix.POS_MAX:
            return i, dx.ERR_POS
        if 36 + lrn + 4 * ncig > b - a:
            return i, dx.ERR_CIGAR
        ops = dx.real_cigar(rec)
        if ops == dx.ERR_AUX:
            return i, dx.ERR_AUX
        if dx.counted(rec, exclude) and pos + sum(o >> 4 for o in ops if (o & 15) in dx.REF) > ref_len[ref]:
            return i, dx.ERR_END
        l_seq = struct.unpack_from("<I", rec, 20)[0]
        if 36 + lrn + 4 * ncig + (l_seq + 1) // 2 + l_seq > b - a:
            return i, ERR_SEQ
        if dx.counted(rec, exclude) and sum(o >> 4 for o in dx.real_cigar(rec) if (o & 15) in READ_OPS) != l_seq:
            return i, ERR_LSEQ
    return None


def events(rec, chrom):
    """[(pos, ch)] of one counted, acceptable record against its chromosome's bytes, regions not yet applied"""
    _ref, pos = ix.fields(rec)[:2]
    ops = dx.real_cigar(rec)
    if not any((o >> 4) and (o & 15) in dx.REF for o in ops):
        return []
    seq, out, rf, rd = seq_of(rec), [], pos, 0
    for o in ops:
        n, c = o >> 4, o & 15
        if n == 0:
            continue
        if c in (0, 7, 8):
            for k in range(n):
                if not pair_matches(seq[rd + k], chrom[rf + k]):
                    out.append((rf + k, channel(seq[rd + k])))
            rf += n
            rd += n
        elif c == 2:
            out.append((rf, DEL))
            rf += n
        elif c == 3:
            rf += n
        elif c == 1:
            out.append((max(rf - 1, pos), INS))
            rd += n
        elif c == 4:
            out.append((max(rf - 1, pos), CLIP))
            rd += n
    return out


def counts(records, chroms, regions=None, exclude=EXCLUDE_DEFAULT):
    """({(ref, pos, ch): n} inside the regions, n_counted, n_events); every record must be acceptable"""
    beg, end, _ = slots([len(c) for c in chroms], regions)
    out, n_counted, n_events = {}, 0, 0
    for rec in records:
        if not dx.counted(rec, exclude):
            continue
        n_counted += 1
        ref = ix.fields(rec)[0]
        for pos, ch in events(rec, chroms[ref]):
            if beg[ref] <= pos < end[ref]:
                out[(ref, pos, ch)] = out.get((ref, pos, ch), 0) + 1
                n_events += 1
    return out, n_counted, n_events


def counts_numpy(data, off, chroms, regions=None, exclude=EXCLUDE_DEFAULT):
    """counts() for many long records, a record at a time with numpy (tools/bench_records.py): the same rule, written a second time --
    test_pileup_dev.py holds the two against each other.  data: uint8 array, off: int64 offsets; the records carry their CIGAR in the record.
    -> (keys (ref << 40 | pos << 3 | ch) sorted, their counts, n_counted, n_events, events per channel)"""
    lut = np.full(256, 15, np.int64)
    for k, b in enumerate(TABLE):
        lut[b] = k
    ch_of = np.full(16, N, np.int64)
    ch_of[[1, 2, 4, 8]] = [A, C, G, T]
    beg, end, _ = slots([len(c) for c in chroms], regions)
    chroms = [np.frombuffer(bytes(c), np.uint8) if not isinstance(c, np.ndarray) else c for c in chroms]
    keys, n_counted = [], 0
    for i in range(len(off) - 1):
        p = int(off[i])
        ref, pos = (int(x) for x in data[p + 4:p + 12].view("<i4"))
        lrn, ncig, flag = int(data[p + 12]), int(data[p + 16:p + 18].view("<u2")[0]), int(data[p + 18:p + 20].view("<u2")[0])
        if ref < 0 or pos < 0 or flag & exclude:
            continue
        n_counted += 1
        l_seq = int(data[p + 20:p + 24].view("<u4")[0])
        at = p + 36 + lrn
        ops = data[at:at + 4 * ncig].view("<u4").astype(np.int64)
        ln, code = ops >> 4, ops & 15
        rf_adv, rd_adv = np.where(np.isin(code, (0, 2, 3, 7, 8)), ln, 0), np.where(np.isin(code, READ_OPS), ln, 0)
        if not rf_adv.sum():
            continue
        rf0, rd0 = pos + np.cumsum(rf_adv) - rf_adv, np.cumsum(rd_adv) - rd_adv
        raw = data[at + 4 * ncig:at + 4 * ncig + (l_seq + 1) // 2]
        codes = np.stack([raw >> 4, raw & 15], 1).reshape(-1)[:l_seq].astype(np.int64)
        m = np.isin(code, (0, 7, 8)) & (ln > 0)
        lm = ln[m]
        inside = np.arange(int(lm.sum())) - np.repeat(np.cumsum(lm) - lm, lm)
        rfi, rdi = np.repeat(rf0[m], lm) + inside, np.repeat(rd0[m], lm) + inside
        c1 = codes[rdi]
        c2 = lut[chroms[ref][rfi]]
        mism = (c1 != 0) & ((c1 != c2) | (c1 == 15))
        ev_pos = [rfi[mism]]
        ev_ch = [ch_of[c1[mism]]]
        for t, ch in ((2, DEL), (1, INS), (4, CLIP)):
            sel = (code == t) & (ln > 0)
            ev_pos.append(rf0[sel] if t == 2 else np.maximum(rf0[sel] - 1, pos))
            ev_ch.append(np.full(int(sel.sum()), ch, np.int64))
        ev_pos, ev_ch = np.concatenate(ev_pos), np.concatenate(ev_ch)
        keep = (ev_pos >= beg[ref]) & (ev_pos < end[ref])
        keys.append((ref << 40) | (ev_pos[keep] << 3) | ev_ch[keep])
    allk = np.concatenate(keys) if keys else np.zeros(0, np.int64)
    uk, n = np.unique(allk, return_counts=True)
    return uk, n, n_counted, int(len(allk)), np.bincount(allk & 7, minlength=CHANNELS).tolist()


def array(cnt, ref_len, regions=None):
    """the object's array [n_bases, 8]"""
    beg, _end, off = slots(ref_len, regions)
    a = np.zeros((off[-1], CHANNELS), np.int32)
    for (ref, pos, ch), n in cnt.items():
        a[off[ref] + pos - beg[ref], ch] = n
    return a


def is_site(count, mask=MASK_DEFAULT, min_count=1, depth=None, num=0, den=1):
    sel = [count[ch] for ch in range(CHANNELS) if (mask >> ch) & 1]
    if not sel or max(sel) < min_count:
        return False
    return depth is None or num == 0 or max(sel) * den >= num * depth


def sites(cnt, chroms, regions=None, depth=None, mask=MASK_DEFAULT, min_count=1, num=0, den=1):
    """the sites ordered by (ref_id, pos); depth: per chromosome an array of depths, or None"""
    beg, end, _ = slots([len(c) for c in chroms], regions)
    per = {}
    for (ref, pos, ch), n in cnt.items():
        per.setdefault((ref, pos), [0] * CHANNELS)[ch] = n
    out = []
    for (ref, pos) in sorted(per):
        d = None if depth is None else int(depth[ref][pos])
        if beg[ref] <= pos < end[ref] and is_site(per[(ref, pos)], mask, min_count, d, num, den):
            out.append((ref, pos, -1 if d is None else d, chroms[ref][pos], (0, 0, 0), tuple(per[(ref, pos)])))
    return np.array(out, SITE) if out else np.zeros(0, SITE)


def sites_text(names, site_arr):
    """<prefix>.sites.tsv"""
    lines = ["#chrom\tpos\tend\tref\tdepth\tA\tC\tG\tT\tN\tDEL\tINS\tCLIP\n"]
    for s in site_arr:
        b = int(s["ref_base"])
        lines.append("%s\t%d\t%d\t%s\t%d\t%s\n" % (names[int(s["ref_id"])], s["pos"], s["pos"] + 1, chr(b) if 33 <= b < 127 else "N", s["depth"],
                                                  "\t".join(str(int(x)) for x in s["count"])))
    return "".join(lines)
