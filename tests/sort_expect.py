"""What plo_records_sort_dev and plo_bam_merge_runs must produce, restated from the definition in include/portello_liftover.h in plain
Python -- not derived from the code under test.  Also makes the hand-made records the tests sort: the call looks at the fixed fields only.
TEST INFRASTRUCTURE ONLY."""
import struct

import numpy as np

MIN_RECORD = 36  # block_size + the 32 fixed bytes
ERR_OFFSET, ERR_SHORT, ERR_BLOCK, ERR_REFID, ERR_POS = 1, 2, 3, 4, 5
POS_MAX = (1 << 31) - 2


def make_record(ref, pos, flag=0, name=b"", payload=b"", block_size=None):
    """block_size + fixed fields + name + payload (any bytes): 36 + len(name) + len(payload) bytes"""
    body = struct.pack("<iiBBHHHIiii", ref, pos, len(name), 0, 0, 0, flag, 0, -1, -1, 0) + name + payload
    return struct.pack("<I", len(body) if block_size is None else block_size) + body


def concat(records):
    off = np.zeros(len(records) + 1, np.uint64)
    if records:
        off[1:] = np.cumsum([len(r) for r in records], dtype=np.uint64)
    return b"".join(records), off


def key_of(rec, n_ref):
    ref, pos = struct.unpack_from("<ii", rec, 4)
    (flag,) = struct.unpack_from("<H", rec, 18)
    return ((n_ref if ref < 0 else ref) << 32) | ((pos + 1) << 1) | ((flag >> 4) & 1)


def first_offender(data, off, n_ref):
    """(record, what it breaks) of the lowest record the device check refuses, or None"""
    n, n_bytes = len(off) - 1, len(data)
    for i in range(n):
        a, b = int(off[i]), int(off[i + 1])
        if (i == 0 and a != 0) or b < a or b > n_bytes or (i == n - 1 and b != n_bytes):
            return i, ERR_OFFSET
        if b - a < MIN_RECORD:
            return i, ERR_SHORT
        rec = data[a:b]
        if struct.unpack_from("<I", rec, 0)[0] + 4 != b - a:
            return i, ERR_BLOCK
        ref, pos = struct.unpack_from("<ii", rec, 4)
        if not -1 <= ref < n_ref:
            return i, ERR_REFID
        if not -1 <= pos <= POS_MAX:
            return i, ERR_POS
    return None


def expect(data, off, n_ref):
    """-> dict(perm, key, record_off, bytes, n_mapped) of a buffer every record of which passes the check"""
    n = len(off) - 1
    recs = [data[int(off[i]):int(off[i + 1])] for i in range(n)]
    key = [key_of(r, n_ref) for r in recs]
    perm = sorted(range(n), key=lambda i: (key[i], i))
    out, new_off = concat([recs[i] for i in perm])
    return {"perm": np.array(perm, np.uint32), "key": np.array([key[i] for i in perm], np.uint64), "record_off": new_off, "bytes": out,
            "n_mapped": sum(1 for k in key if (k >> 32) < n_ref)}


def split_records(data):
    """the records of a stream of block_size-prefixed records"""
    out, at = [], 0
    while at < len(data):
        bs = struct.unpack_from("<I", data, at)[0]
        out.append(data[at:at + 4 + bs])
        at += 4 + bs
    assert at == len(data)
    return out


def merged(runs, n_ref):
    """runs: lists of records, each in key order -> the records ordered by (key, run, place in the run)"""
    allr = [(key_of(r, n_ref), ri, k, r) for ri, run in enumerate(runs) for k, r in enumerate(run)]
    return [t[3] for t in sorted(allr, key=lambda t: t[:3])]
