"""ctypes binding of tests/emu/libplo_emu_eqx.so: eqx_core.hpp (the device code of plo_eqx_dev) and records_core.hpp with = / X CIGARs
executed under the CPU wave64 emulator.  Built the way emu_md_lib builds its harness.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

import emu_md_lib as eml
import emu_nm_lib as enl
import emu_records_lib as erl
from portello_amd import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
_LIB = os.path.join(_HERE, "emu", "libplo_emu_eqx.so")
_ASAN = os.path.join(_HERE, "emu", "emu_eqx_asan")
_lib = None
_FLAGS = enl._FLAGS


def _sources():
    return [os.path.join(_HERE, "emu", "emu_eqx.cpp")] + eml._sources() + [os.path.join(ROOT, "portello_amd", "csrc", f) for f in ("eqx_core.hpp", "aln_walk.hpp")]


def build(force=False):
    srcs = _sources()
    if force or erl._stale(_LIB, srcs):
        subprocess.check_call(_FLAGS + ["-fPIC", "-shared", "-I" + os.path.join(_HERE, "emu"), "-o", _LIB, srcs[0]])
    return _LIB


def build_asan(force=False):
    """the same code as a program with AddressSanitizer and UBSan (CPU only): emu_eqx_asan IN OUT"""
    srcs = _sources()
    if force or erl._stale(_ASAN, srcs):
        subprocess.check_call(_FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-DEMU_EQX_MAIN",
                                        "-I" + os.path.join(_HERE, "emu"), "-o", _ASAN, srcs[0]])
    return _ASAN


_u32p, _u64p, _u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
_p = enl._p


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(_LIB)
        L.emu_eqx_batch.restype = C.c_int
        L.emu_eqx_batch.argtypes = [C.POINTER(abi.PloBatchIn), C.POINTER(abi.PloBatchOut), _u64p, _u8p, C.POINTER(abi.PloIndexDesc), C.c_uint, C.c_uint, _u64p, _u64p, _u32p]
        L.emu_eqx_ops.restype = None
        L.emu_eqx_ops.argtypes = [_u32p]
        L.emu_eqx_free.restype = None
        L.emu_eqx_one.restype = C.c_int
        L.emu_eqx_one.argtypes = [_u32p, C.c_uint32, _u8p, C.c_uint32, C.c_int, _u8p, C.c_int, C.c_int64, C.c_uint, _u64p, _u32p, C.c_uint64]
        L.emu_eqx_records_build.restype = C.c_int
        L.emu_eqx_records_build.argtypes = [C.POINTER(abi.PloBatchIn), C.POINTER(abi.PloBatchOut), C.POINTER(abi.PloFinishOut), _u32p, _u8p, C.POINTER(abi.PloIndexDesc),
                                            C.POINTER(abi.PloRecordsIn), _u32p, _u64p, _u8p, _u64p, _u32p, C.c_int, C.c_int, C.c_uint, C.POINTER(abi.PloRecordsOut)]
        L.emu_records_free.restype = None
        _lib = L
    return _lib


def eqx_batch(index: abi.IndexData, batch: abi.BatchData, lift: abi.BatchResult, item_seq_off, rev_seq, order_seed=0, item_seed=0):
    """eqx_core.hpp over a whole batch: count, scan, emit -> (status, item_eqx_off [n + 1], ops, the count pass's op counts, err_item); status
    -2 / -3: the emit stored outside the ops / left one of them unwritten"""
    lo, keep = abi.out_from_result(lift)
    b, ixd = batch.to_desc(), index.to_desc()
    so = np.ascontiguousarray(item_seq_off, np.uint64) if len(item_seq_off) else np.zeros(1, np.uint64)
    rs = np.ascontiguousarray(rev_seq, np.uint8) if len(rev_seq) else np.zeros(16, np.uint8)
    off, ln = np.zeros(lift.n_items + 1, np.uint64), np.zeros(max(1, lift.n_items), np.uint64)
    err = C.c_uint32(0)
    st = lib().emu_eqx_batch(C.byref(b), C.byref(lo), _p(so, C.c_uint64), _p(rs, C.c_uint8), C.byref(ixd), int(order_seed), int(item_seed), _p(off, C.c_uint64),
                             _p(ln, C.c_uint64), C.byref(err))
    ops = np.zeros(max(1, int(off[-1])), np.uint32)
    if st == abi.PLO_OK:
        lib().emu_eqx_ops(_p(ops, C.c_uint32))
    lib().emu_eqx_free()
    return st, off, ops[:int(off[-1])], ln[:lift.n_items], int(err.value)


def eqx_one(case: enl.Case, order_seed=0, cap=1 << 18):
    """-> (status, the count pass's op count, the emitted ops).  The ops lie between 16 canary words on either side."""
    ops = case.ops if len(case.ops) else np.zeros(1, np.uint32)
    buf = np.zeros(case.front + max(1, (case.l_seq + 1) // 2), np.uint8)
    buf[case.front:case.front + (case.l_seq + 1) // 2] = case.packed()
    seq = buf[case.front:]
    ref = case.ref if len(case.ref) else np.zeros(1, np.uint8)
    ln, out = C.c_uint64(0), np.zeros(cap, np.uint32)
    st = lib().emu_eqx_one(_p(ops, C.c_uint32), len(case.ops), _p(seq, C.c_uint8), case.l_seq, 1 if case.flip else 0, _p(ref, C.c_uint8), len(case.ref), case.pos,
                           int(order_seed), C.byref(ln), _p(out, C.c_uint32), cap)
    return st, int(ln.value), out[:int(ln.value)].copy() if st == abi.PLO_OK else np.zeros(0, np.uint32)


def run_asan(cases, tmp_dir: str, order_seed=0):
    """every case through the sanitizer build in one process, each array (the output ops too) in a heap block of its exact size
    -> (return code, stderr, [(status, ops)])"""
    exe = build_asan()
    pin, pout = os.path.join(tmp_dir, "eqx_asan_in.bin"), os.path.join(tmp_dir, "eqx_asan_out.bin")
    with open(pin, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for c in cases:
            fh.write(struct.pack("<IIIIiqI", len(c.ops), c.l_seq, 1 if c.flip else 0, c.front, len(c.ref), c.pos, order_seed))
            fh.write(c.ops.astype("<u4").tobytes() + c.packed().tobytes() + c.ref.tobytes())
    pr = subprocess.run([exe, pin, pout], capture_output=True, text=True, timeout=600)
    if pr.returncode != 0:
        return pr.returncode, pr.stderr, None
    blob, at, res = open(pout, "rb").read(), 0, []
    for _ in cases:
        st, n = struct.unpack_from("<iQ", blob, at)
        res.append((st, np.frombuffer(blob, "<u4", n, at + 12).copy()))
        at += 12 + 4 * n
    assert at == len(blob)
    return 0, pr.stderr, res


def records_with_eqx(index, batch, raw, read_rec_off, lift, f, sa_off, sa_text, contig_names, item_nm, item_md_off, md_text, item_eqx_off, eqx_ops,
                     is_target_region=False, vec=True, nthreads=7, order_seed=0):
    """emu_md_lib.records_with_md with DevRecords::item_eqx_off / eqx_ops as well (each of item_nm, item_md_off and item_eqx_off may be None)
    -> (status, bytes, record_off, n_lifted, n_unmapped_copies)"""
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
    mdo = None if item_md_off is None else np.ascontiguousarray(item_md_off, np.uint64)
    mdt = None if item_md_off is None else np.frombuffer(bytes(md_text) + b"\xa5", np.uint8)  # (exact size but for one byte no record may hold)
    exo = None if item_eqx_off is None else np.ascontiguousarray(item_eqx_off, np.uint64)
    exv = None if item_eqx_off is None else np.concatenate([np.asarray(eqx_ops, np.uint32), np.array([0xA5A5A5A5], np.uint32)])  # (the same, one word)
    out = abi.PloRecordsOut()
    st = lib().emu_eqx_records_build(C.byref(b), C.byref(lo), C.byref(fo), _p(so, C.c_uint32), _p(stx, C.c_uint8), C.byref(ixd), C.byref(rin),
                                     None if nmv is None else _p(nmv, C.c_uint32), None if mdo is None else _p(mdo, C.c_uint64),
                                     None if mdt is None else _p(mdt, C.c_uint8), None if exo is None else _p(exo, C.c_uint64),
                                     None if exv is None else _p(exv, C.c_uint32), 1 if vec else 0, int(nthreads), int(order_seed), C.byref(out))
    data, off = b"", np.zeros(1, np.uint64)
    if st == 0:
        data = C.string_at(out.bytes, out.n_bytes) if out.n_bytes else b""
        off = np.ctypeslib.as_array(out.record_off, shape=(int(out.n_records) + 1,)).copy()
    res = (st, data, off, int(out.n_lifted), int(out.n_unmapped_copies))
    lib().emu_records_free()
    return res
