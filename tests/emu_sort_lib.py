"""ctypes binding of tests/emu/libplo_emu_sort.so: sort_core.hpp (the device code of plo_records_sort_dev) executed under the CPU wave64
emulator.  Built the way emu_records_lib builds its harness.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

import emu_records_lib as erl
from portello_amd import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
_LIB = os.path.join(_HERE, "emu", "libplo_emu_sort.so")
_ASAN = os.path.join(_HERE, "emu", "emu_sort_asan")
_lib = None
_FLAGS = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas"]


def _sources():
    return [os.path.join(_HERE, "emu", "emu_sort.cpp"), os.path.join(_HERE, "emu", "plo_wave.hpp")] + [
        os.path.join(ROOT, "portello_amd", "csrc", f) for f in ("sort_core.hpp", "records_core.hpp", "finish_core.hpp", "lift_core.hpp", "lift_types.hpp")]


def build(force=False):
    srcs = _sources()
    if force or erl._stale(_LIB, srcs):
        subprocess.check_call(_FLAGS + ["-fPIC", "-shared", "-I" + os.path.join(_HERE, "emu"), "-o", _LIB, srcs[0]])
    return _LIB


def build_asan(force=False):
    """the same code as a program with AddressSanitizer and UBSan (CPU only): emu_sort_asan IN OUT"""
    srcs = _sources()
    if force or erl._stale(_ASAN, srcs):
        subprocess.check_call(_FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-DEMU_SORT_MAIN",
                                        "-I" + os.path.join(_HERE, "emu"), "-o", _ASAN, srcs[0]])
    return _ASAN


_u32p, _u64p, _u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(_LIB)
        L.emu_sort.restype = C.c_int
        L.emu_sort.argtypes = [_u8p, C.c_uint64, C.c_uint32, _u64p, C.c_uint32, C.c_uint, _u8p, _u8p, _u64p, _u32p, _u64p, _u32p, _u32p, _u32p]
        L.emu_sort_tile.restype = C.c_uint32
        _lib = L
    return _lib


def tile():
    """SORT_TILE: records per workgroup of the tile sort"""
    return int(lib().emu_sort_tile())


def sort(data: bytes, off, n_ref, expect_bytes: bytes = b"", order_seed=0):
    """-> (status, dict(perm, key, record_off, bytes, n_mapped) or None, err_record, err_kind); status -2 / -3: the copy stored outside the
    output / did not store every byte exactly once.  The records lie in a buffer of their exact size."""
    n = len(off) - 1
    raw = np.frombuffer(data, np.uint8).copy() if len(data) else np.zeros(1, np.uint8)
    exp = np.frombuffer(expect_bytes, np.uint8).copy() if len(expect_bytes) else np.zeros(max(1, len(data)), np.uint8)
    offs = np.ascontiguousarray(off, np.uint64)
    out = np.zeros(max(1, len(data)), np.uint8)
    ooff, perm, key = np.zeros(n + 1, np.uint64), np.zeros(max(1, n), np.uint32), np.zeros(max(1, n), np.uint64)
    nm, er, ek = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    st = lib().emu_sort(_p(raw, C.c_uint8), len(data), n, _p(offs, C.c_uint64), int(n_ref), int(order_seed), _p(exp, C.c_uint8), _p(out, C.c_uint8), _p(ooff, C.c_uint64),
                        _p(perm, C.c_uint32), _p(key, C.c_uint64), C.byref(nm), C.byref(er), C.byref(ek))
    res = None
    if st in (abi.PLO_OK, -2, -3):
        res = {"perm": perm[:n], "key": key[:n], "record_off": ooff, "bytes": out[:len(data)].tobytes(), "n_mapped": int(nm.value)}
    return st, res, int(er.value), int(ek.value)


def run_asan(cases, tmp_dir: str):
    """cases: [(data, off, n_ref, expect_bytes or None, order_seed)] through the sanitizer build in one process, every array in a heap block of
    its exact size -> (return code, stderr, [(status, result dict or None, err_record, err_kind)])"""
    exe = build_asan()
    pin, pout = os.path.join(tmp_dir, "sort_asan_in.bin"), os.path.join(tmp_dir, "sort_asan_out.bin")
    with open(pin, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for data, off, n_ref, exp, seed in cases:
            n = len(off) - 1
            fh.write(struct.pack("<IIIIQ", n, n_ref, seed, 0 if exp is None else 1, len(data)))
            fh.write(np.ascontiguousarray(off, "<u8").tobytes() + data + (b"" if exp is None else exp))
    pr = subprocess.run([exe, pin, pout], capture_output=True, text=True, timeout=600)
    if pr.returncode != 0:
        return pr.returncode, pr.stderr, None
    blob, at, res = open(pout, "rb").read(), 0, []
    for data, off, n_ref, exp, seed in cases:
        n = len(off) - 1
        st, er, ek, nm = struct.unpack_from("<iIII", blob, at)
        at += 16
        r = None
        if st == 0:
            perm = np.frombuffer(blob, "<u4", n, at)
            key = np.frombuffer(blob, "<u8", n, at + 4 * n)
            ooff = np.frombuffer(blob, "<u8", n + 1, at + 12 * n)
            at += 12 * n + 8 * (n + 1)
            r = {"perm": perm, "key": key, "record_off": ooff, "bytes": blob[at:at + len(data)], "n_mapped": nm}
            at += len(data)
        res.append((st, r, er, ek))
    assert at == len(blob)
    return 0, pr.stderr, res
