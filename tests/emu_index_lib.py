"""ctypes binding of tests/emu/libplo_emu_index.so: index_core.hpp (the device code of plo_records_index_dev) executed under the CPU wave64
emulator.  Built the way emu_sort_lib builds its harness.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

import emu_records_lib as erl
import index_expect as ix
from portello_amd import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
_LIB = os.path.join(_HERE, "emu", "libplo_emu_index.so")
_ASAN = os.path.join(_HERE, "emu", "emu_index_asan")
_lib = None
_FLAGS = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas"]


def _sources():
    return [os.path.join(_HERE, "emu", "emu_index.cpp"), os.path.join(_HERE, "emu", "plo_wave.hpp")] + [
        os.path.join(ROOT, "portello_amd", "csrc", f) for f in ("index_core.hpp", "sort_core.hpp", "records_core.hpp", "finish_core.hpp", "lift_core.hpp", "lift_types.hpp")]


def build(force=False):
    srcs = _sources()
    if force or erl._stale(_LIB, srcs):
        subprocess.check_call(_FLAGS + ["-fPIC", "-shared", "-I" + os.path.join(_HERE, "emu"), "-o", _LIB, srcs[0]])
    return _LIB


def build_asan(force=False):
    """the same code as a program with AddressSanitizer and UBSan (CPU only): emu_index_asan IN OUT"""
    srcs = _sources()
    if force or erl._stale(_ASAN, srcs):
        subprocess.check_call(_FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-DEMU_INDEX_MAIN",
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
        L.emu_index.restype = C.c_int
        L.emu_index.argtypes = [_u8p, C.c_uint64, C.c_uint32, _u64p, C.c_uint32, C.c_uint, C.c_uint32, _u8p, _u32p, _u32p, _u32p]
        _lib = L
    return _lib


def index(data: bytes, off, n_ref, order_seed=0, n_waves=4):
    """-> (status, entries (index_expect.ENTRY array) or None, n_placed, err_record, err_kind); status -4: the wave's entry of a record and
    the one-thread rule's differ.  The records lie in a buffer of their exact size."""
    n = len(off) - 1
    raw = np.frombuffer(data, np.uint8).copy() if len(data) else np.zeros(1, np.uint8)
    offs = np.ascontiguousarray(off, np.uint64)
    ent = np.zeros(max(1, n), ix.ENTRY)
    np_, er, ek = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    st = lib().emu_index(_p(raw, C.c_uint8), len(data), n, _p(offs, C.c_uint64), int(n_ref), int(order_seed), int(n_waves), ent.ctypes.data_as(_u8p),
                         C.byref(np_), C.byref(er), C.byref(ek))
    return st, (ent[:n] if st == abi.PLO_OK else None), int(np_.value), int(er.value), int(ek.value)


def run_asan(cases, tmp_dir: str):
    """cases: [(data, off, n_ref, order_seed, n_waves)] through the sanitizer build in one process, every array in a heap block of its exact
    size -> (return code, stderr, [(status, entries or None, n_placed, err_record, err_kind)])"""
    exe = build_asan()
    pin, pout = os.path.join(tmp_dir, "index_asan_in.bin"), os.path.join(tmp_dir, "index_asan_out.bin")
    with open(pin, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for data, off, n_ref, seed, n_waves in cases:
            fh.write(struct.pack("<IIIIQ", len(off) - 1, n_ref, seed, n_waves, len(data)))
            fh.write(np.ascontiguousarray(off, "<u8").tobytes() + data)
    pr = subprocess.run([exe, pin, pout], capture_output=True, text=True, timeout=600)
    if pr.returncode != 0:
        return pr.returncode, pr.stderr, None
    blob, at, res = open(pout, "rb").read(), 0, []
    for data, off, n_ref, seed, n_waves in cases:
        n = len(off) - 1
        st, er, ek, np_ = struct.unpack_from("<iIII", blob, at)
        at += 16
        ent = None
        if st == 0:
            ent = np.frombuffer(blob, ix.ENTRY, n, at)
            at += 24 * n
        res.append((st, ent, np_, er, ek))
    assert at == len(blob)
    return 0, pr.stderr, res
