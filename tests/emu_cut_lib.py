"""ctypes binding of tests/emu/libplo_emu_cut.so: window_core.hpp (the device code of plo_window_cut_dev) executed under the CPU wave64
emulator with segments of any size, and the host-only BGZF header walk of plo_bgzf_inflate_dev.  Built the way emu_batch_lib builds its
harness.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import struct
import subprocess
from dataclasses import dataclass
from typing import Optional

import numpy as np

from portello_amd import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
_LIB = os.path.join(_HERE, "emu", "libplo_emu_cut.so")
_ASAN = os.path.join(_HERE, "emu", "emu_cut_asan")
_lib = None


def _sources():
    return [os.path.join(_HERE, "emu", "emu_cut.cpp"), os.path.join(_HERE, "emu", "plo_wave.hpp")] + [
        os.path.join(ROOT, "portello_amd", "csrc", f) for f in ("window_core.hpp", "bgzf_walk.hpp", "records_core.hpp", "finish_core.hpp", "lift_core.hpp", "lift_types.hpp")] + [
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
    """the same code as a program with AddressSanitizer and UBSan (CPU only): emu_cut_asan IN OUT"""
    srcs = _sources()
    if force or _stale(_ASAN, srcs):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-DEMU_CUT_MAIN", "-I" + os.path.join(_HERE, "emu"), "-o", _ASAN, srcs[0]])
    return _ASAN


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(_LIB)
        L.emu_window_cut.restype = C.c_int
        L.emu_window_cut.argtypes = [C.POINTER(abi.PloWindowCutIn), C.c_ulonglong, C.c_uint, C.c_int, C.POINTER(abi.PloWindowCutOut)]
        L.emu_cut_free.restype = None
        L.emu_bgzf_walk.restype = C.c_int
        L.emu_bgzf_walk.argtypes = [C.c_char_p, C.c_ulonglong, C.c_ulonglong, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong), C.POINTER(C.c_uint32),
                                    C.POINTER(C.c_ulonglong), C.c_uint32]
        _lib = L
    return _lib


@dataclass
class Cut:
    """a window as the host reader or the device call cut it; on a refusal only status and err_off count"""
    status: int
    n_reads: int = 0
    read_rec_off: Optional[list] = None
    n_unmapped: int = 0
    unmapped: bytes = b""
    unmapped_off: Optional[list] = None
    window_bytes: int = 0
    ended_by: int = -1
    err_off: int = abi.CUT_NO_ERR
    n_rewalks: int = 0

    def key(self):
        if self.status != abi.PLO_OK:
            return (self.status, self.err_off)
        return (0, self.n_reads, list(self.read_rec_off), self.n_unmapped, self.unmapped, self.window_bytes, self.ended_by)


def window_cut(stream: bytes, seg_bytes: int, max_records: int, final: bool, max_unmapped: int = 0, max_bytes: int = 0, order_seed: int = 0,
               no_guess: bool = False) -> Cut:
    buf = np.frombuffer(stream, dtype=np.uint8).copy() if len(stream) else np.zeros(1, np.uint8)
    cin = abi.PloWindowCutIn(buf.ctypes.data_as(abi._u8p), len(stream), max_records, max_unmapped, max_bytes, 1 if final else 0)
    out = abi.PloWindowCutOut()
    st = lib().emu_window_cut(C.byref(cin), seg_bytes, order_seed, 1 if no_guess else 0, C.byref(out))
    res = Cut(st, err_off=int(out.err_off), n_rewalks=int(out.n_rewalks))
    if st == abi.PLO_OK:
        nr, nu, ub = int(out.n_reads), int(out.n_unmapped), int(out.unmapped_bytes)
        res = Cut(st, nr, [int(out.read_rec_off[i]) for i in range(nr)], nu, bytes(bytearray(out.unmapped[:ub])), [int(out.unmapped_off[i]) for i in range(nu + 1)],
                  int(out.window_bytes), int(out.ended_by), int(out.err_off), int(out.n_rewalks))
    lib().emu_cut_free()
    return res


def run_asan(stream: bytes, seg_bytes: int, max_records: int, final: bool, tmp_dir: str, max_unmapped: int = 0, max_bytes: int = 0):
    """the cut from the sanitizer build, the stream in a heap block of its exact size: (return code, stderr, Cut or None)"""
    exe = build_asan()
    pin, pout = os.path.join(tmp_dir, "cut_asan_in.bin"), os.path.join(tmp_dir, "cut_asan_out.bin")
    with open(pin, "wb") as fh:
        fh.write(struct.pack("<QQQQII", len(stream), seg_bytes, max_unmapped, max_bytes, max_records, 1 if final else 0) + stream)
    pr = subprocess.run([exe, pin, pout], capture_output=True, text=True, timeout=600)
    if pr.returncode != 0:
        return pr.returncode, pr.stderr, None
    blob = open(pout, "rb").read()
    st, ended, nr, nu = struct.unpack_from("<4I", blob, 0)
    wb, err_off, ub, rew = struct.unpack_from("<4Q", blob, 16)
    res = Cut(st, err_off=err_off, n_rewalks=rew)
    if st == abi.PLO_OK:
        at = 48
        rro = list(struct.unpack_from(f"<{nr}Q", blob, at))
        at += 8 * nr
        uo = list(struct.unpack_from(f"<{nu + 1}Q", blob, at))
        at += 8 * (nu + 1)
        res = Cut(st, nr, rro, nu, blob[at:at + ub], uo, wb, ended if ended < 0x80000000 else ended - (1 << 32), err_off, rew)
        assert at + ub == len(blob)
    return 0, pr.stderr, res


def bgzf_walk(buf: bytes, cap: int):
    """-> (return code 0 ok / 1 not a header / 2 corrupt / 3 too large, consumed, inflated bytes, blocks as (off, coff, clen, uoff, ulen, crc))"""
    consumed, n_bytes, nb = C.c_ulonglong(0), C.c_ulonglong(0), C.c_uint32(0)
    cap_blocks = len(buf) // 28 + 1
    blk = (C.c_ulonglong * (6 * cap_blocks))()
    rc = lib().emu_bgzf_walk(buf, len(buf), cap, C.byref(consumed), C.byref(n_bytes), C.byref(nb), blk, cap_blocks)
    return rc, int(consumed.value), int(n_bytes.value), [tuple(int(blk[6 * i + k]) for k in range(6)) for i in range(nb.value)]
