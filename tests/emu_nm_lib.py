"""ctypes binding of tests/emu/libplo_emu_nm.so: nm_core.hpp (the device code of plo_nm_dev) and records_core.hpp with NM:i executed
under the CPU wave64 emulator.  Built the way emu_records_lib builds its harness.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

import emu_records_lib as erl
from portello_amd import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
_LIB = os.path.join(_HERE, "emu", "libplo_emu_nm.so")
_ASAN = os.path.join(_HERE, "emu", "emu_nm_asan")
_lib = None
_FLAGS = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas"]


def _sources():
    return [os.path.join(_HERE, "emu", "emu_nm.cpp"), os.path.join(_HERE, "emu", "emu_records.cpp"), os.path.join(_HERE, "emu", "plo_wave.hpp")] + [
        os.path.join(ROOT, "portello_amd", "csrc", f) for f in ("nm_core.hpp", "aln_walk.hpp", "records_core.hpp", "finish_core.hpp", "lift_core.hpp", "lift_types.hpp")] + [
        os.path.join(ROOT, "include", "portello_liftover.h")]


def build(force=False):
    srcs = _sources()
    if force or erl._stale(_LIB, srcs):
        subprocess.check_call(_FLAGS + ["-fPIC", "-shared", "-I" + os.path.join(_HERE, "emu"), "-o", _LIB, srcs[0]])
    return _LIB


def build_asan(force=False):
    """the same code as a program with AddressSanitizer and UBSan (CPU only): emu_nm_asan IN OUT"""
    srcs = _sources()
    if force or erl._stale(_ASAN, srcs):
        subprocess.check_call(_FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-DEMU_NM_MAIN",
                                        "-I" + os.path.join(_HERE, "emu"), "-o", _ASAN, srcs[0]])
    return _ASAN


_u32p, _u64p, _u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(_LIB)
        L.emu_nm_batch.restype = C.c_int
        L.emu_nm_batch.argtypes = [C.POINTER(abi.PloBatchIn), C.POINTER(abi.PloBatchOut), _u64p, _u8p, C.POINTER(abi.PloIndexDesc), C.c_uint, C.c_uint, _u32p, _u64p, _u32p]
        L.emu_nm_one.restype = C.c_int
        L.emu_nm_one.argtypes = [_u32p, C.c_uint32, _u8p, C.c_uint32, C.c_int, _u8p, C.c_int, C.c_int64, C.c_uint, _u32p, _u64p]
        L.emu_nm_records_build.restype = C.c_int
        L.emu_nm_records_build.argtypes = [C.POINTER(abi.PloBatchIn), C.POINTER(abi.PloBatchOut), C.POINTER(abi.PloFinishOut), _u32p, _u8p, C.POINTER(abi.PloIndexDesc),
                                           C.POINTER(abi.PloRecordsIn), _u32p, C.c_int, C.c_int, C.c_uint, C.POINTER(abi.PloRecordsOut)]
        L.emu_records_free.restype = None
        _lib = L
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def nm_batch(index: abi.IndexData, batch: abi.BatchData, lift: abi.BatchResult, item_seq_off, rev_seq, order_seed=0, item_seed=0):
    """nm_core.hpp over a whole batch -> (status, item_nm, n_cmp_bases, err_item)"""
    lo, keep = abi.out_from_result(lift)
    b, ixd = batch.to_desc(), index.to_desc()
    so = np.ascontiguousarray(item_seq_off, np.uint64) if len(item_seq_off) else np.zeros(1, np.uint64)
    rs = np.ascontiguousarray(rev_seq, np.uint8) if len(rev_seq) else np.zeros(16, np.uint8)
    nm = np.full(max(1, lift.n_items), 0xDEADBEEF, np.uint32)
    cmp_, err = C.c_uint64(0), C.c_uint32(0)
    st = lib().emu_nm_batch(C.byref(b), C.byref(lo), _p(so, C.c_uint64), _p(rs, C.c_uint8), C.byref(ixd), int(order_seed), int(item_seed), _p(nm, C.c_uint32),
                            C.byref(cmp_), C.byref(err))
    return st, nm[:lift.n_items], int(cmp_.value), int(err.value)


class Case:
    """one hand-made item: CIGAR ops, the record's 4-bit codes (one per base), the chromosome and the position on it"""

    def __init__(self, name, ops, codes, ref, pos, flip=False, front=0):
        self.name, self.ops, self.codes = name, np.asarray(ops, np.uint32), np.asarray(codes, np.uint8)
        self.ref, self.pos, self.flip, self.front = np.ascontiguousarray(ref, np.uint8), int(pos), bool(flip), int(front)

    @property
    def l_seq(self):
        return len(self.codes)

    def packed(self) -> np.ndarray:
        c = np.concatenate([self.codes, np.zeros(len(self.codes) & 1, np.uint8)])
        return ((c[0::2] << 4) | c[1::2]).astype(np.uint8)


def nm_one(case: Case, order_seed=0):
    """-> (status, NM, bases compared).  The bases lie `front` bytes into their buffer."""
    ops = case.ops if len(case.ops) else np.zeros(1, np.uint32)
    buf = np.zeros(case.front + max(1, (case.l_seq + 1) // 2), np.uint8)
    buf[case.front:case.front + (case.l_seq + 1) // 2] = case.packed()
    seq = buf[case.front:]
    ref = case.ref if len(case.ref) else np.zeros(1, np.uint8)
    nm, cmp_ = C.c_uint32(0xDEADBEEF), C.c_uint64(0)
    st = lib().emu_nm_one(_p(ops, C.c_uint32), len(case.ops), _p(seq, C.c_uint8), case.l_seq, 1 if case.flip else 0, _p(ref, C.c_uint8), len(case.ref), case.pos,
                          int(order_seed), C.byref(nm), C.byref(cmp_))
    return st, int(nm.value), int(cmp_.value)


def run_asan(cases, tmp_dir: str, order_seed=0):
    """every case through the sanitizer build in one process, each array in a heap block of its exact size
    -> (return code, stderr, [(status, NM, bases compared)])"""
    exe = build_asan()
    pin, pout = os.path.join(tmp_dir, "nm_asan_in.bin"), os.path.join(tmp_dir, "nm_asan_out.bin")
    with open(pin, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for c in cases:
            fh.write(struct.pack("<IIIIiqI", len(c.ops), c.l_seq, 1 if c.flip else 0, c.front, len(c.ref), c.pos, order_seed))
            fh.write(c.ops.astype("<u4").tobytes() + c.packed().tobytes() + c.ref.tobytes())
    pr = subprocess.run([exe, pin, pout], capture_output=True, text=True, timeout=600)
    if pr.returncode != 0:
        return pr.returncode, pr.stderr, None
    blob = open(pout, "rb").read()
    assert len(blob) == 16 * len(cases)
    return 0, pr.stderr, [struct.unpack_from("<IIQ", blob, 16 * k) for k in range(len(cases))]


def records_with_nm(index, batch, raw, read_rec_off, lift, f, sa_off, sa_text, contig_names, item_nm, is_target_region=False, vec=True, nthreads=7, order_seed=0):
    """emu_records_lib.records_from_finished with DevRecords::item_nm (None: without) -> (status, bytes, record_off, n_lifted, n_unmapped_copies)"""
    ct = {np.dtype(np.uint16): C.c_uint16, np.dtype(np.int64): C.c_int64, np.dtype(np.uint8): C.c_uint8, np.dtype(np.uint64): C.c_uint64,
          np.dtype(np.uint32): C.c_uint32}
    keep = {k: np.ascontiguousarray(v) for k, v in f.items()}
    fo = abi.PloFinishOut()
    for name, dt in abi.FINISH_ITEM_FIELDS + abi.FINISH_READ_FIELDS:
        a = keep[name] if len(keep[name]) else np.zeros(1, dt)
        keep[name] = a
        setattr(fo, name, a.ctypes.data_as(C.POINTER(ct[np.dtype(dt)])))

    def aligned(a):  # 16-byte aligned copies of the reversed bases / qualities, as the device buffers are
        buf = np.zeros(max(16, len(a)) + 32, np.uint8)
        o = (-buf.ctypes.data) & 15
        buf[o:o + len(a)] = a
        return buf, buf[o:o + max(16, len(a))]
    ks, vs = aligned(keep["rev_seq"])
    kq, vq = aligned(keep["rev_qual"])
    fo.rev_seq, fo.rev_qual = _p(vs, C.c_uint8), _p(vq, C.c_uint8)
    fo.rev_seq_bytes, fo.rev_qual_bytes = len(f["rev_seq"]), len(f["rev_qual"])
    fo.n_items, fo.n_reads = lift.n_items, batch.n_reads
    lo, keep_l = abi.out_from_result(lift)
    b, ixd = batch.to_desc(), index.to_desc()
    so = np.ascontiguousarray(sa_off, np.uint32)
    stx = np.ascontiguousarray(sa_text, np.uint8) if len(sa_text) else np.zeros(1, np.uint8)
    coff, cblob = erl.name_table(contig_names)
    rro = np.ascontiguousarray(read_rec_off, np.uint64) if len(read_rec_off) else np.zeros(1, np.uint64)
    raw = np.ascontiguousarray(raw, np.uint8)
    rin = abi.PloRecordsIn(_p(raw, C.c_uint8), len(raw), _p(rro, C.c_uint64), len(contig_names), _p(coff, C.c_uint32), _p(cblob, C.c_uint8), 1 if is_target_region else 0)
    nmv = None if item_nm is None else np.ascontiguousarray(item_nm, np.uint32)
    out = abi.PloRecordsOut()
    st = lib().emu_nm_records_build(C.byref(b), C.byref(lo), C.byref(fo), _p(so, C.c_uint32), _p(stx, C.c_uint8), C.byref(ixd), C.byref(rin),
                                    None if nmv is None else _p(nmv, C.c_uint32), 1 if vec else 0, int(nthreads), int(order_seed), C.byref(out))
    data, off = b"", np.zeros(1, np.uint64)
    if st == 0:
        data = C.string_at(out.bytes, out.n_bytes) if out.n_bytes else b""
        off = np.ctypeslib.as_array(out.record_off, shape=(int(out.n_records) + 1,)).copy()
    res = (st, data, off, int(out.n_lifted), int(out.n_unmapped_copies))
    lib().emu_records_free()
    return res
