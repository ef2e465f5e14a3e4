"""ctypes binding of tests/emu/libplo_emu_depth.so: depth_core.hpp (the device code of plo_depth_*) executed under the CPU wave64 emulator,
with PLO_DEPTH_TILE = TILE so that small inputs reach the tile seams of every level of the scan.  Built the way emu_index_lib builds its
harness.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

import depth_expect as dx
import emu_records_lib as erl
from portello_amd import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
_LIB = os.path.join(_HERE, "emu", "libplo_emu_depth.so")
_ASAN = os.path.join(_HERE, "emu", "emu_depth_asan")
_lib = None
TILE = 12
_FLAGS = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-DPLO_DEPTH_TILE=%d" % TILE]


def _sources():
    return [os.path.join(_HERE, "emu", "emu_depth.cpp"), os.path.join(_HERE, "emu", "plo_wave.hpp"), os.path.abspath(__file__)] + [
        os.path.join(ROOT, "portello_amd", "csrc", f) for f in ("depth_core.hpp", "index_core.hpp", "batch_core.hpp", "sort_core.hpp", "records_core.hpp", "finish_core.hpp", "lift_core.hpp", "lift_types.hpp")]


def build(force=False):
    srcs = _sources()
    if force or erl._stale(_LIB, srcs):
        subprocess.check_call(_FLAGS + ["-fPIC", "-shared", "-I" + os.path.join(_HERE, "emu"), "-o", _LIB, srcs[0]])
    return _LIB


def build_asan(force=False):
    """the same code as a program with AddressSanitizer and UBSan (CPU only): emu_depth_asan IN OUT"""
    srcs = _sources()
    if force or erl._stale(_ASAN, srcs):
        subprocess.check_call(_FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-DEMU_DEPTH_MAIN",
                                        "-I" + os.path.join(_HERE, "emu"), "-o", _ASAN, srcs[0]])
    return _ASAN


_u32p, _u64p, _u8p, _i32p = C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_int32)


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(_LIB)
        L.emu_depth_tile.restype = C.c_uint
        L.emu_depth_create.restype = C.c_void_p
        L.emu_depth_create.argtypes = [C.c_uint32, _i32p, C.c_uint32, C.c_int]
        L.emu_depth_destroy.argtypes = [C.c_void_p]
        L.emu_depth_destroy.restype = None
        L.emu_depth_entries.restype = C.c_uint64
        L.emu_depth_entries.argtypes = [C.c_void_p]
        L.emu_depth_slots.argtypes = [C.c_void_p, _u64p]
        L.emu_depth_slots.restype = None
        L.emu_depth_array.argtypes = [C.c_void_p, _i32p]
        L.emu_depth_array.restype = None
        L.emu_depth_reset.argtypes = [C.c_void_p]
        L.emu_depth_add.argtypes = [C.c_void_p, _u8p, C.c_uint64, C.c_uint32, _u64p, C.c_uint, C.c_uint32, _u32p, _u32p, _u32p]
        L.emu_depth_finish.argtypes = [C.c_void_p, C.c_uint]
        L.emu_depth_n_windows.restype = C.c_uint64
        L.emu_depth_n_windows.argtypes = [C.c_void_p, C.c_uint32]
        L.emu_depth_windows.argtypes = [C.c_void_p, C.c_uint32, C.c_uint, C.c_uint32, _u64p, _u64p]
        L.emu_depth_runs.argtypes = [C.c_void_p, C.c_uint, _u64p]
        L.emu_depth_runs_copy.argtypes = [C.c_void_p, _u8p]
        L.emu_depth_runs_copy.restype = None
        assert L.emu_depth_tile() == TILE
        _lib = L
    return _lib


class EmuDepth:
    """a depth object whose kernels are emulated waves; the statuses are the C ABI's (-4: the wave's adds and the one-thread rule's differ)"""

    def __init__(self, ref_len, exclude=dx.EXCLUDE_DEFAULT, deletions=False):
        self.ref_len = list(ref_len)
        rl = np.ascontiguousarray(ref_len, np.int32) if len(ref_len) else np.zeros(1, np.int32)
        self.h = lib().emu_depth_create(len(ref_len), _p(rl, C.c_int32), exclude, int(deletions))

    def close(self):
        if self.h:
            lib().emu_depth_destroy(self.h)
            self.h = None

    def slots(self):
        out = np.zeros(len(self.ref_len) + 1, np.uint64)
        lib().emu_depth_slots(self.h, _p(out, C.c_uint64))
        return out

    def array(self):
        n = lib().emu_depth_entries(self.h)
        out = np.zeros(max(1, n), np.int32)
        lib().emu_depth_array(self.h, _p(out, C.c_int32))
        return out[:n]

    def add(self, data: bytes, off, order_seed=0, n_waves=4):
        """-> (status, n_counted, err_record, err_kind); the records lie in a buffer of their exact size"""
        raw = np.frombuffer(data, np.uint8).copy() if len(data) else np.zeros(1, np.uint8)
        offs = np.ascontiguousarray(off, np.uint64)
        nc, er, ek = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        st = lib().emu_depth_add(self.h, _p(raw, C.c_uint8), len(data), len(off) - 1, _p(offs, C.c_uint64), int(order_seed), int(n_waves), C.byref(nc), C.byref(er), C.byref(ek))
        return st, int(nc.value), int(er.value), int(ek.value)

    def finish(self, order_seed=0):
        return lib().emu_depth_finish(self.h, int(order_seed))

    def reset(self):
        return lib().emu_depth_reset(self.h)

    def windows(self, w, order_seed=0, n_waves=3):
        """-> (status, win_first, sums)"""
        n = lib().emu_depth_n_windows(self.h, w)
        sums, first = np.zeros(max(1, n), np.uint64), np.zeros(len(self.ref_len) + 1, np.uint64)
        st = lib().emu_depth_windows(self.h, w, int(order_seed), int(n_waves), _p(sums, C.c_uint64), _p(first, C.c_uint64))
        return st, first, sums[:n]

    def runs(self, order_seed=0):
        """-> (status, runs (depth_expect.RUN array))"""
        n = C.c_uint64(0)
        st = lib().emu_depth_runs(self.h, int(order_seed), C.byref(n))
        out = np.zeros(max(1, n.value), dx.RUN)
        if st == abi.PLO_OK and n.value:
            lib().emu_depth_runs_copy(self.h, out.ctypes.data_as(_u8p))
        return st, out[:n.value]


def run_asan(cases, tmp_dir: str):
    """cases: [(ref_len, exclude, deletions, w, [(data, off, order_seed, n_waves)])] through the sanitizer build in one process, every array in
    a heap block of its exact size -> (return code, stderr, [dict(adds [(status, err_record, err_kind, n_counted)], diff, depth, win_first,
    sums, runs)])"""
    exe = build_asan()
    pin, pout = os.path.join(tmp_dir, "depth_asan_in.bin"), os.path.join(tmp_dir, "depth_asan_out.bin")
    with open(pin, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for ref_len, exclude, deletions, w, adds in cases:
            fh.write(struct.pack("<IIIII", len(ref_len), exclude, int(deletions), w, len(adds)))
            fh.write(np.ascontiguousarray(ref_len, "<i4").tobytes())
            for data, off, seed, n_waves in adds:
                fh.write(struct.pack("<IIIIQ", len(off) - 1, seed, n_waves, 0, len(data)))
                fh.write(np.ascontiguousarray(off, "<u8").tobytes() + data)
    pr = subprocess.run([exe, pin, pout], capture_output=True, text=True, timeout=600)
    if pr.returncode != 0:
        return pr.returncode, pr.stderr, None
    blob, at, res = open(pout, "rb").read(), 0, []
    for ref_len, exclude, deletions, w, adds in cases:
        r = {"adds": []}
        for _ in adds:
            st, er, ek, nc = struct.unpack_from("<iIII", blob, at)
            at += 16
            r["adds"].append((st, er, ek, nc))
        ne = struct.unpack_from("<Q", blob, at)[0]
        at += 8
        r["diff"] = np.frombuffer(blob, "<i4", ne, at)
        at += 4 * ne
        r["depth"] = np.frombuffer(blob, "<i4", ne, at)
        at += 4 * ne
        nw = struct.unpack_from("<Q", blob, at)[0]
        at += 8
        r["win_first"] = np.frombuffer(blob, "<u8", len(ref_len) + 1, at)
        at += 8 * (len(ref_len) + 1)
        r["sums"] = np.frombuffer(blob, "<u8", nw, at)
        at += 8 * nw
        nr = struct.unpack_from("<Q", blob, at)[0]
        at += 8
        r["runs"] = np.frombuffer(blob, dx.RUN, nr, at)
        at += 16 * nr
        res.append(r)
    assert at == len(blob)
    return 0, pr.stderr, res
