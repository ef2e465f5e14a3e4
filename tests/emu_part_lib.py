"""ctypes binding of tests/emu/libplo_emu_part.so: the device code of plo_part_start_dev and plo_window_cut_part_dev (window_core.hpp)
executed under the CPU wave64 emulator, and the host-only BGZF header walk with own_bytes (plo_bgzf_inflate_part_dev).  Built the way
emu_cut_lib builds its harness.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

from emu_cut_lib import Cut
from portello_amd import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
_LIB = os.path.join(_HERE, "emu", "libplo_emu_part.so")
_ASAN = os.path.join(_HERE, "emu", "emu_part_asan")
_lib = None
_FLAGS = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas"]


def _sources():
    return [os.path.join(_HERE, "emu", "emu_part.cpp"), os.path.join(_HERE, "emu", "plo_wave.hpp")] + [
        os.path.join(ROOT, "portello_amd", "csrc", f) for f in ("window_core.hpp", "bgzf_walk.hpp", "records_core.hpp", "finish_core.hpp", "lift_core.hpp", "lift_types.hpp")] + [
        os.path.join(ROOT, "include", "portello_liftover.h")]


def _stale(target, srcs):
    return (not os.path.exists(target)) or any(os.path.getmtime(s) > os.path.getmtime(target) for s in srcs)


def build(force=False):
    srcs = _sources()
    if force or _stale(_LIB, srcs):
        subprocess.check_call(_FLAGS + ["-fPIC", "-shared", "-I" + os.path.join(_HERE, "emu"), "-o", _LIB, srcs[0]])
    return _LIB


def build_asan(force=False):
    """the same code as a program with AddressSanitizer and UBSan (CPU only): emu_part_asan IN OUT"""
    srcs = _sources()
    if force or _stale(_ASAN, srcs):
        subprocess.check_call(_FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-DEMU_PART_MAIN",
                                        "-I" + os.path.join(_HERE, "emu"), "-o", _ASAN, srcs[0]])
    return _ASAN


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(_LIB)
        L.emu_part_start.restype = C.c_int
        L.emu_part_start.argtypes = [C.POINTER(abi.PloPartStartIn), C.c_ulonglong, C.c_uint, C.c_uint, C.POINTER(abi.PloPartStartOut)]
        L.emu_window_cut_part.restype = C.c_int
        L.emu_window_cut_part.argtypes = [C.POINTER(abi.PloWindowCutPartIn), C.c_ulonglong, C.c_uint, C.c_int, C.POINTER(abi.PloWindowCutOut)]
        L.emu_part_free.restype = None
        L.emu_bgzf_walk_part.restype = C.c_int
        L.emu_bgzf_walk_part.argtypes = [C.c_char_p, C.c_ulonglong, C.c_ulonglong, C.c_ulonglong, C.c_ulonglong] + [C.POINTER(C.c_ulonglong)] * 3 + [C.POINTER(C.c_uint32)]
        _lib = L
    return _lib


def _buf(stream: bytes):
    return np.frombuffer(stream, dtype=np.uint8).copy() if len(stream) else np.zeros(1, np.uint8)


def part_start(stream: bytes, n_ref: int, final: bool, tile: int = 64, order_seed: int = 0, tile_seed: int = 0):
    """-> (kind, first_off or None); tile_seed != 0: the tiles in shuffled order, none left early"""
    buf = _buf(stream)
    pin = abi.PloPartStartIn(buf.ctypes.data_as(abi._u8p), len(stream), n_ref, 1 if final else 0)
    out = abi.PloPartStartOut()
    st = lib().emu_part_start(C.byref(pin), tile, order_seed, tile_seed, C.byref(out))
    assert st == abi.PLO_OK, st
    assert (int(out.first_off) == abi.CUT_NO_ERR) == (int(out.kind) != abi.PART_FOUND)
    return int(out.kind), (int(out.first_off) if int(out.kind) == abi.PART_FOUND else None)


def window_cut_part(stream: bytes, seg_bytes: int, max_records: int, final: bool, own_bytes: int, max_unmapped: int = 0, max_bytes: int = 0,
                    order_seed: int = 0, no_guess: bool = False) -> Cut:
    buf = _buf(stream)
    cin = abi.PloWindowCutPartIn(buf.ctypes.data_as(abi._u8p), len(stream), max_records, max_unmapped, max_bytes, 1 if final else 0, own_bytes)
    out = abi.PloWindowCutOut()
    st = lib().emu_window_cut_part(C.byref(cin), seg_bytes, order_seed, 1 if no_guess else 0, C.byref(out))
    res = Cut(st, err_off=int(out.err_off), n_rewalks=int(out.n_rewalks))
    if st == abi.PLO_OK:
        nr, nu, ub = int(out.n_reads), int(out.n_unmapped), int(out.unmapped_bytes)
        res = Cut(st, nr, [int(out.read_rec_off[i]) for i in range(nr)], nu, bytes(bytearray(out.unmapped[:ub])), [int(out.unmapped_off[i]) for i in range(nu + 1)],
                  int(out.window_bytes), int(out.ended_by), int(out.err_off), int(out.n_rewalks))
    lib().emu_part_free()
    return res


def bgzf_walk_part(buf: bytes, cap: int, file_off: int, range_end: int):
    """-> (return code, consumed, inflated bytes, own_bytes, blocks)"""
    v = [C.c_ulonglong(0) for _ in range(3)]
    nb = C.c_uint32(0)
    rc = lib().emu_bgzf_walk_part(buf, len(buf), cap, file_off, range_end, C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.byref(nb))
    return rc, int(v[0].value), int(v[1].value), int(v[2].value), int(nb.value)


def run_asan(cases, tmp_dir: str):
    """every case through the sanitizer build in one process, each stream in a heap block of its exact size.  A case is
    ("start", stream, n_ref, final, tile, order_seed, tile_seed) or ("cut", stream, seg_bytes, max_records, final, own_bytes, max_unmapped, max_bytes)
    -> (return code, stderr, results: (kind, first_off or None) / Cut)"""
    exe = build_asan()
    pin, pout = os.path.join(tmp_dir, "part_asan_in.bin"), os.path.join(tmp_dir, "part_asan_out.bin")
    with open(pin, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for c in cases:
            if c[0] == "start":
                _, s, n_ref, final, tile, oseed, tseed = c
                fh.write(struct.pack("<IQQIIII", 0, len(s), tile, n_ref, 1 if final else 0, oseed, tseed) + s)
            else:
                _, s, seg, mr, final, own, mu, mb = c
                fh.write(struct.pack("<IQQQQQII", 1, len(s), seg, mu, mb, own, mr, 1 if final else 0) + s)
    pr = subprocess.run([exe, pin, pout], capture_output=True, text=True, timeout=600)
    if pr.returncode != 0:
        return pr.returncode, pr.stderr, None
    blob, at, res = open(pout, "rb").read(), 0, []
    for c in cases:
        if c[0] == "start":
            st, kind, off = struct.unpack_from("<IIQ", blob, at)
            at += 16
            assert st == abi.PLO_OK
            res.append((kind, off if kind == abi.PART_FOUND else None))
        else:
            st, ended, nr, nu, wb, err_off, ub = struct.unpack_from("<4I3Q", blob, at)
            at += 40
            r = Cut(st, err_off=err_off)
            if st == abi.PLO_OK:
                rro = list(struct.unpack_from(f"<{nr}Q", blob, at))
                at += 8 * nr
                r = Cut(st, nr, rro, nu, blob[at:at + ub], None, wb, ended, err_off)
                at += ub
            res.append(r)
    assert at == len(blob)
    return 0, pr.stderr, res
