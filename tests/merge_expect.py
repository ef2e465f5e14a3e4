"""What plo_runs_merge_plan_dev / plo_runs_merge_emit_dev must produce, restated from the definition in include/portello_liftover.h in
plain Python -- not derived from the code under test: the records numbered run-major, sorted by (key, g), their offsets, and the greedy
chunk table.  The records and the key come from sort_expect.py.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

import sort_expect as sx

ERR_ORDER = 6  # behind sort_expect's kinds 1 .. 5: a key below the key of the record before it in the same run
MAX_RUNS = 4096


def chunk_table(lengths, chunk_bytes):
    """chunk c begins at record first[c] and holds as many following records as keep its bytes <= chunk_bytes, never fewer than one"""
    first, at, n = [], 0, len(lengths)
    while at < n:
        first.append(at)
        size, at = lengths[at], at + 1
        while at < n and size + lengths[at] <= chunk_bytes:
            size += lengths[at]
            at += 1
    return first + [n]


def first_offender(runs, n_ref):
    """runs: [(data, off)] -> (run, place, kind) of the lowest g the device check refuses and the first kind it breaks, or None"""
    for r, (data, off) in enumerate(runs):
        n, n_bytes = len(off) - 1, len(data)
        prev = None
        for i in range(n):
            a, b = int(off[i]), int(off[i + 1])
            if (i == 0 and a != 0) or b < a or b > n_bytes or (i == n - 1 and b != n_bytes):
                return r, i, sx.ERR_OFFSET
            rec = data[a:b]
            one = sx.first_offender(rec, np.array([0, len(rec)], np.uint64), n_ref)
            if one is not None:
                return r, i, one[1]
            key = sx.key_of(rec, n_ref)
            if prev is not None and key < prev:
                return r, i, ERR_ORDER
            prev = key
    return None


def expect(runs, n_ref, chunk_bytes):
    """runs: [(data, off)], every record of which passes the check -> dict(src, key, record_off, bytes, n_mapped, chunk_first, chunk_off,
    chunks: [(bytes, rebased record_off)])"""
    recs = []
    for data, off in runs:
        recs += [data[int(off[i]):int(off[i + 1])] for i in range(len(off) - 1)]
    key = [sx.key_of(r, n_ref) for r in recs]
    src = sorted(range(len(recs)), key=lambda g: (key[g], g))
    merged = [recs[g] for g in src]
    out, new_off = sx.concat(merged)
    first = chunk_table([len(r) for r in merged], chunk_bytes)
    chunks = [sx.concat(merged[a:b]) for a, b in zip(first[:-1], first[1:])]
    return {"src": np.array(src, np.uint32), "key": np.array([key[g] for g in src], np.uint64), "record_off": new_off, "bytes": out,
            "n_mapped": sum(1 for k in key if (k >> 32) < n_ref), "chunk_first": np.array(first, np.uint32),
            "chunk_off": np.array([int(new_off[f]) for f in first], np.uint64), "chunks": chunks}
