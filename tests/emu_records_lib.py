"""ctypes binding of tests/emu/libplo_emu_records.so: records_core.hpp (the device code of plo_records_build_dev) executed under the
CPU wave64 emulator.  Built the way emu_lib.build builds the other harness.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

import emu_lib
from portello_amd import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
_LIB = os.path.join(_HERE, "emu", "libplo_emu_records.so")
_ASAN = os.path.join(_HERE, "emu", "emu_records_asan")
_lib = None


def _sources():
    return [os.path.join(_HERE, "emu", "emu_records.cpp"), os.path.join(_HERE, "emu", "plo_wave.hpp")] + [
        os.path.join(ROOT, "portello_amd", "csrc", f) for f in ("records_core.hpp", "finish_core.hpp", "lift_core.hpp", "lift_types.hpp")]


def _stale(target, srcs):
    return (not os.path.exists(target)) or any(os.path.getmtime(s) > os.path.getmtime(target) for s in srcs)


def build(force=False):
    srcs = _sources()
    if force or _stale(_LIB, srcs):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fPIC", "-shared", "-I" + os.path.join(_HERE, "emu"),
                               "-o", _LIB, srcs[0]])
    return _LIB


def build_asan(force=False):
    """the same code as a program with AddressSanitizer and UBSan (CPU only): emu_records_asan IN OUT"""
    srcs = _sources()
    if force or _stale(_ASAN, srcs):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-DEMU_RECORDS_MAIN", "-I" + os.path.join(_HERE, "emu"), "-o", _ASAN, srcs[0]])
    return _ASAN


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(_LIB)
        L.emu_records_build.restype = C.c_int
        L.emu_records_build.argtypes = [C.POINTER(abi.PloBatchIn), C.POINTER(abi.PloBatchOut), C.POINTER(abi.PloFinishOut), C.POINTER(C.c_uint32),
                                        C.POINTER(C.c_uint8), C.POINTER(abi.PloIndexDesc), C.POINTER(abi.PloRecordsIn), C.c_int, C.c_int, C.c_uint,
                                        C.POINTER(abi.PloRecordsOut), C.POINTER(C.c_uint)]
        L.emu_records_free.restype = None
        L.emu_scan64.restype = None
        L.emu_scan64.argtypes = [C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint64), C.c_uint]
        _lib = L
    return _lib


def scan64(values: np.ndarray, order_seed=0) -> np.ndarray:
    v = np.ascontiguousarray(values, dtype=np.uint64)
    out = np.zeros(len(v) + 1, dtype=np.uint64)
    vv = v if len(v) else np.zeros(1, np.uint64)
    lib().emu_scan64(vv.ctypes.data_as(C.POINTER(C.c_uint64)), len(v), out.ctypes.data_as(C.POINTER(C.c_uint64)), order_seed)
    return out


def name_table(names):
    enc = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
    off = np.zeros(len(enc) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(e) for e in enc])
    return off, np.frombuffer(b"".join(enc) or b"\0", dtype=np.uint8).copy()


def records_build(index: abi.IndexData, batch: abi.BatchData, read_flags, raw: np.ndarray, read_rec_off, read_seq_off, read_qual_off, lift: abi.BatchResult,
                  contig_names, ref_names, is_target_region=False, vec=True, nthreads=7, order_seed=0):
    """The whole device route on the host: finish_core.hpp (emu_lib.finish_batch, emu_lib.sa_segments) with the batch's bases and the
    qualities as VIEWS into `raw` (the window's records as they stand), then records_core.hpp.
    -> (status, bytes, record_off, n_lifted, n_unmapped_copies, err counters); status 1 = a bounds check failed, nothing emitted"""
    import dataclasses

    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    vb = dataclasses.replace(batch, seq=raw, read_seq_off=np.ascontiguousarray(read_seq_off, np.uint64), seq_fmt=abi.SEQ_BAM4)
    f = emu_lib.finish_batch(vb, read_flags, raw, read_qual_off, lift)
    sa_off, sa_text, _ = emu_lib.sa_segments(vb, lift, f["item_flag"], f["read_n_lifted"], ref_names)
    st, data, off, nl, nu, err = records_from_finished(index, vb, raw, read_rec_off, lift, f, sa_off, sa_text, contig_names, is_target_region, vec, nthreads, order_seed)
    return st, data, off, nl, nu, err, f, sa_off


def records_from_finished(index, batch, raw, read_rec_off, lift, f, sa_off, sa_text, contig_names, is_target_region=False, vec=True, nthreads=7, order_seed=0,
                          records_bytes=None):
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    ct = {np.dtype(np.uint16): C.c_uint16, np.dtype(np.int64): C.c_int64, np.dtype(np.uint8): C.c_uint8, np.dtype(np.uint64): C.c_uint64,
          np.dtype(np.uint32): C.c_uint32}
    keep = {k: np.ascontiguousarray(v) for k, v in f.items()}
    for k in ("rev_seq", "rev_qual"):
        if not len(keep[k]):
            keep[k] = np.zeros(16, np.uint8)
    fo = abi.PloFinishOut()
    for name, dt in abi.FINISH_ITEM_FIELDS + abi.FINISH_READ_FIELDS:
        a = keep[name] if len(keep[name]) else np.zeros(1, dt)
        keep[name] = a
        setattr(fo, name, a.ctypes.data_as(C.POINTER(ct[np.dtype(dt)])))
    # 16-byte aligned copies of the reversed bases / qualities, as the device buffers are
    def aligned(a):
        buf = np.zeros(len(a) + 32, np.uint8)
        o = (-buf.ctypes.data) & 15
        buf[o:o + len(a)] = a
        return buf, buf[o:o + len(a)]
    ks, vs = aligned(keep["rev_seq"])
    kq, vq = aligned(keep["rev_qual"])
    fo.rev_seq, fo.rev_qual = p(vs, C.c_uint8), p(vq, C.c_uint8)
    fo.rev_seq_bytes, fo.rev_qual_bytes = len(f["rev_seq"]), len(f["rev_qual"])
    fo.n_items, fo.n_reads = lift.n_items, batch.n_reads
    lo, keep_l = abi.out_from_result(lift)
    b = batch.to_desc()
    ixd = index.to_desc()
    so = np.ascontiguousarray(sa_off, np.uint32)
    stx = np.ascontiguousarray(sa_text, np.uint8) if len(sa_text) else np.zeros(1, np.uint8)
    coff, cblob = name_table(contig_names)
    rro = np.ascontiguousarray(read_rec_off, np.uint64)
    if not len(rro):
        rro = np.zeros(1, np.uint64)
    rin = abi.PloRecordsIn(p(raw, C.c_uint8), len(raw) if records_bytes is None else int(records_bytes), p(rro, C.c_uint64), len(contig_names), p(coff, C.c_uint32),
                           p(cblob, C.c_uint8), 1 if is_target_region else 0)
    out = abi.PloRecordsOut()
    err = (C.c_uint * 4)()
    st = lib().emu_records_build(C.byref(b), C.byref(lo), C.byref(fo), p(so, C.c_uint32), p(stx, C.c_uint8), C.byref(ixd), C.byref(rin), 1 if vec else 0,
                                 int(nthreads), int(order_seed), C.byref(out), err)
    data, off = b"", np.zeros(1, np.uint64)
    if st == 0:
        data = C.string_at(out.bytes, out.n_bytes) if out.n_bytes else b""
        off = np.ctypeslib.as_array(out.record_off, shape=(int(out.n_records) + 1,)).copy()
    res = (st, data, off, int(out.n_lifted), int(out.n_unmapped_copies), list(err))
    lib().emu_records_free()
    return res


def run_asan(raw: bytes, read_rec_off, tmp_dir: str):
    """the unmapped copies of forward-strand records without lift items from the sanitizer build: (return code, stderr, bytes, n_records)"""
    exe = build_asan()
    pin, pout = os.path.join(tmp_dir, "asan_in.bin"), os.path.join(tmp_dir, "asan_out.bin")
    with open(pin, "wb") as fh:
        fh.write(struct.pack("<QI", len(raw), len(read_rec_off)) + raw + np.asarray(read_rec_off, dtype="<u8").tobytes())
    pr = subprocess.run([exe, pin, pout], capture_output=True, text=True, timeout=600)
    if pr.returncode != 0:
        return pr.returncode, pr.stderr, b"", 0
    blob = open(pout, "rb").read()
    nb, nrec = struct.unpack_from("<QI", blob, 0)
    return 0, pr.stderr, blob[12:12 + nb], nrec
