"""tests/emu/emu_finish.cpp: finish_core.hpp (record finishing, SA text) as a stand-alone program with AddressSanitizer and UBSan, built and
run the way emu_deflate_lib.run_asan builds and runs its program.  Every array of a batch lives in a heap block of its exact size there, so
a load or store of the device code that leaves its buffer ends the program.  TEST INFRASTRUCTURE ONLY."""
import os
import struct
import subprocess

import numpy as np

from portello_amd import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
_ASAN = os.path.join(_HERE, "emu", "emu_finish_asan")


def _sources():
    return [os.path.join(_HERE, "emu", f) for f in ("emu_finish.cpp", "emu_finish.hpp", "plo_wave.hpp")] + [
        os.path.join(ROOT, "portello_amd", "csrc", f) for f in ("finish_core.hpp", "lift_core.hpp", "lift_types.hpp")]


def build_asan(force=False):
    srcs = _sources()
    stale = (not os.path.exists(_ASAN)) or any(os.path.getmtime(s) > os.path.getmtime(_ASAN) for s in srcs)
    if force or stale:
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I" + os.path.join(_HERE, "emu"), "-o", _ASAN, srcs[0]])
    return _ASAN


def _shift_of(view: np.ndarray) -> int:
    """how far the view starts into the array it was cut from"""
    base = view.base
    return 0 if base is None else view.ctypes.data - base.ctypes.data


def encode_case(case, threads, names=None) -> bytes:
    """one finish_cases.Case in the program's input format"""
    b, lift = case.batch, case.lift
    one = b.seq.ctypes.data == case.qual.ctypes.data and len(b.seq) == len(case.qual) and len(b.seq) > 0
    shift = _shift_of(b.seq)
    assert 0 <= shift <= 3 and (one or len(case.qual) == 0 or _shift_of(case.qual) == shift)
    enc = [c.encode() if isinstance(c, str) else bytes(c) for c in (names or [])]
    noff = np.zeros(len(enc) + 1, np.uint32)
    noff[1:] = np.cumsum([len(e) for e in enc])
    blob = b"".join(enc)
    n, nr = lift.n_items, b.n_reads
    head = struct.pack("<I", len(threads)) + struct.pack("<%dI" % len(threads), *threads)
    head += struct.pack("<8I4Q", b.seq_fmt, nr, b.n_segs, n, len(enc), shift, 1 if one else 0, 1 if names is not None else 0,
                        len(lift.cigar), len(b.seq), len(case.qual), len(blob))
    t = lambda a, dt: np.ascontiguousarray(a, dtype=dt).tobytes()
    parts = [head, t(b.read_seq_len, np.uint32), t(b.read_seq_off, np.uint64), t(case.flags, np.uint16), t(case.qoff, np.uint64), t(b.seg_read, np.uint32),
             t(b.seq, np.uint8)]
    if not one:
        parts.append(t(case.qual, np.uint8))
    parts += [t(lift.item_seg, np.uint32), t(lift.item_status, np.uint8), t(lift.item_need_flipped, np.uint8), t(lift.item_mapq, np.uint8),
              t(lift.item_chrom_index, np.uint32), t(lift.item_ref_pos, np.int64), t(lift.item_cigar_off, np.uint64), t(lift.item_cigar_len, np.uint32),
              t(lift.cigar, np.uint32), noff.tobytes(), blob]
    return b"".join(parts)


class _Cursor:
    def __init__(self, data):
        self.data, self.at = data, 0

    def take(self, dt, count):
        nb = int(count) * np.dtype(dt).itemsize
        assert self.at + nb <= len(self.data), "the program's output is short"
        a = np.frombuffer(self.data, dt, int(count), self.at).copy()
        self.at += nb
        return a


def decode_results(data: bytes, cases) -> list:
    """per case: ([the finish dict of every thread count], (sa offsets, sa text) or None); cases: (case, threads, names)"""
    cur, out = _Cursor(data), []
    for case, threads, names in cases:
        n, nr = case.lift.n_items, case.batch.n_reads
        runs, sa = [], None
        for k, _ in enumerate(threads):
            res = {"n_fault": int(cur.take(np.uint32, 1)[0])}
            for name, dt in abi.FINISH_ITEM_FIELDS:
                res[name] = cur.take(dt, n)
            for name, dt in abi.FINISH_READ_FIELDS:
                res[name] = cur.take(dt, nr)
            sb, qb = (int(x) for x in cur.take(np.uint64, 2))
            res["rev_seq"], res["rev_qual"] = cur.take(np.uint8, sb), cur.take(np.uint8, qb)
            runs.append(res)
            if names is not None and k == 0:
                off = cur.take(np.uint32, n + 1)
                sa = (off, cur.take(np.uint8, int(off[n])))
        out.append((runs, sa))
    assert cur.at == len(data), "the program wrote more than the cases ask for"
    return out


def run_asan(cases, tmp_dir: str):
    """cases: (finish_cases.Case, thread counts, chromosome names or None) -> (return code, stderr, decode_results(...) or None)"""
    exe = build_asan()
    pin, pout = os.path.join(tmp_dir, "fin_asan_in.bin"), os.path.join(tmp_dir, "fin_asan_out.bin")
    with open(pin, "wb") as fh:
        fh.write(struct.pack("<II", 0x314e4946, len(cases)))
        for case, threads, names in cases:
            fh.write(encode_case(case, threads, names))
    pr = subprocess.run([exe, pin, pout], capture_output=True, text=True, timeout=900)
    if pr.returncode != 0:
        return pr.returncode, pr.stderr, None
    with open(pout, "rb") as fh:
        return 0, pr.stderr, decode_results(fh.read(), cases)
