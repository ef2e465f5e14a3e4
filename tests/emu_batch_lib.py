"""ctypes binding of tests/emu/libplo_emu_batch.so: batch_core.hpp (the device code of plo_batch_build_dev) executed under the CPU wave64
emulator.  Built the way emu_records_lib builds its harness.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

from portello_amd import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
_LIB = os.path.join(_HERE, "emu", "libplo_emu_batch.so")
_ASAN = os.path.join(_HERE, "emu", "emu_batch_asan")
_lib = None

# the arrays of a batch in the order emu_batch_asan writes them: (name, dtype, "r" per read / "s" per segment / "s1" / "ops")
ARRAYS = (("read_is_reverse", np.uint8, "r"), ("read_seq_len", np.uint32, "r"), ("read_seq_off", np.uint64, "r"), ("read_flags", np.uint16, "r"),
          ("read_qual_off", np.uint64, "r"), ("seg_read", np.uint32, "s"), ("seg_contig", np.uint32, "s"), ("seg_pos", np.int64, "s"),
          ("seg_is_fwd_strand", np.uint8, "s"), ("seg_cigar_off", np.uint32, "s1"), ("cigar", np.uint32, "ops"))


def _sources():
    return [os.path.join(_HERE, "emu", "emu_batch.cpp"), os.path.join(_HERE, "emu", "plo_wave.hpp")] + [
        os.path.join(ROOT, "portello_amd", "csrc", f) for f in ("batch_core.hpp", "records_core.hpp", "finish_core.hpp", "lift_core.hpp", "lift_types.hpp")] + [
        os.path.join(ROOT, "include", "portello_liftover.h")]


def _stale(target, srcs):
    return (not os.path.exists(target)) or any(os.path.getmtime(s) > os.path.getmtime(target) for s in srcs)


def build(force=False):
    srcs = _sources()
    if force or _stale(_LIB, srcs):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fPIC", "-shared", "-I" + os.path.join(_HERE, "emu"),
                               "-o", _LIB, srcs[0]])
    return _LIB


def build_asan(force=False):
    """the same code as a program with AddressSanitizer and UBSan (CPU only): emu_batch_asan IN OUT"""
    srcs = _sources()
    if force or _stale(_ASAN, srcs):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-DEMU_BATCH_MAIN", "-I" + os.path.join(_HERE, "emu"), "-o", _ASAN, srcs[0]])
    return _ASAN


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(_LIB)
        L.emu_batch_build.restype = C.c_int
        L.emu_batch_build.argtypes = [C.POINTER(abi.PloBatchBuildIn), C.c_uint, C.POINTER(abi.PloBatchBuildOut), C.POINTER(C.c_int)]
        L.emu_batch_free.restype = None
        _lib = L
    return _lib


def name_table(names):
    enc = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
    off = np.zeros(len(enc) + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(e) for e in enc])
    return off, np.frombuffer(b"".join(enc) or b"\0", dtype=np.uint8).copy()


def counts(n, ns, n_ops):
    return {"r": n, "s": ns, "s1": ns + 1, "ops": n_ops}


def batch_build(raw: np.ndarray, read_rec_off, contig_names, order_seed=0, records_bytes=None):
    """-> (status, arrays by name or None, err_read, err_kind, bounds counters [offset, block, layout, -])"""
    p = lambda a, t: a.ctypes.data_as(C.POINTER(t))
    raw = np.ascontiguousarray(raw, dtype=np.uint8)
    rbuf = raw if len(raw) else np.zeros(1, np.uint8)
    rro = np.ascontiguousarray(read_rec_off, np.uint64)
    n = len(rro)
    if not n:
        rro = np.zeros(1, np.uint64)
    coff, cblob = name_table(contig_names)
    bin_ = abi.PloBatchBuildIn(p(rbuf, C.c_uint8), len(raw) if records_bytes is None else int(records_bytes), p(rro, C.c_uint64), n, len(contig_names),
                               p(coff, C.c_uint32), p(cblob, C.c_uint8))
    out = abi.PloBatchBuildOut()
    bounds = (C.c_int * 4)()
    st = lib().emu_batch_build(C.byref(bin_), int(order_seed), C.byref(out), bounds)
    arrays = None
    if st == abi.PLO_OK:
        b, f = out.batch, out.fin
        ns = int(b.n_segs)
        assert int(b.n_reads) == n and int(b.seq_fmt) == abi.SEQ_BAM4 and int(b.n_items) == 0
        assert int(b.seq_bytes) == int(f.qual_bytes) == int(bin_.records_bytes)
        assert C.cast(b.seq, C.c_void_p).value == C.cast(f.qual, C.c_void_p).value == C.cast(bin_.records, C.c_void_p).value

        def cp(ptr, dt, cnt):
            if not cnt:
                return np.zeros(0, dt)
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(cnt * np.dtype(dt).itemsize,)).view(dt).copy()

        n_ops = int(cp(b.seg_cigar_off, np.uint32, ns + 1)[-1])
        cnt = counts(n, ns, n_ops)
        arrays = {name: cp(getattr(f if name in ("read_flags", "read_qual_off") else b, name), dt, cnt[k]) for name, dt, k in ARRAYS}
    res = (st, arrays, int(out.err_read), int(out.err_kind), list(bounds))
    lib().emu_batch_free()
    return res


def run_asan(raw: bytes, read_rec_off, contig_names, tmp_dir: str):
    """the batch from the sanitizer build, every input in a heap block of its exact size: (return code, stderr, status, arrays or None)"""
    exe = build_asan()
    pin, pout = os.path.join(tmp_dir, "bb_asan_in.bin"), os.path.join(tmp_dir, "bb_asan_out.bin")
    coff, cblob = name_table(contig_names)
    nn = int(coff[-1])
    with open(pin, "wb") as fh:
        fh.write(struct.pack("<QIII", len(raw), len(read_rec_off), len(contig_names), nn) + raw + np.asarray(read_rec_off, dtype="<u8").tobytes() +
                 coff.astype("<u4").tobytes() + cblob[:nn].tobytes())
    pr = subprocess.run([exe, pin, pout], capture_output=True, text=True, timeout=600)
    if pr.returncode != 0:
        return pr.returncode, pr.stderr, None, None
    blob = open(pout, "rb").read()
    st, err_read, err_kind, n, ns, n_ops = struct.unpack_from("<6I", blob, 0)
    arrays = None
    if st == abi.PLO_OK:
        arrays, at, cnt = {}, 24, counts(n, ns, n_ops)
        for name, dt, k in ARRAYS:
            nb = cnt[k] * np.dtype(dt).itemsize
            arrays[name] = np.frombuffer(blob[at:at + nb], dtype=dt).copy()
            at += nb
        assert at == len(blob)
    return 0, pr.stderr, st, arrays
