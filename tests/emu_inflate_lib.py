"""inflate.hpp (the device code of k_bgzf_inflate) on the host: the emulator library's two entry points with a guard behind the output, and
tests/emu/emu_inflate_asan, the same code as a stand-alone AddressSanitizer + UBSan program.  Built the way emu_deflate_lib builds its
harness.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import struct
import subprocess

import emu_lib

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
_ASAN = os.path.join(_HERE, "emu", "emu_inflate_asan")
GUARD = 64
WAVE_SEED = 4711


def _sources():
    return [os.path.join(_HERE, "emu", f) for f in ("emu_inflate.cpp", "emu_inflate.hpp", "plo_wave.hpp")] + [os.path.join(ROOT, "portello_amd", "csrc", "inflate.hpp")]


def _stale(target, srcs):
    return (not os.path.exists(target)) or any(os.path.getmtime(s) > os.path.getmtime(target) for s in srcs)


def build_asan(force=False):
    """the decoder as a program with AddressSanitizer and UBSan (CPU only): emu_inflate_asan IN OUT"""
    srcs = _sources()
    if force or _stale(_ASAN, srcs):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I" + os.path.join(_HERE, "emu"), "-o", _ASAN, srcs[0]])
    return _ASAN


def _lib():
    L = emu_lib.lib()
    if not getattr(L, "_inflate_bound", False):
        L.emu_inflate.restype = C.c_int
        L.emu_inflate.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        L.emu_inflate_wave.restype = C.c_int
        L.emu_inflate_wave.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32), C.c_uint]
        L._inflate_bound = True
    return L


def inflate(comp: bytes, cap: int, wave: bool = False, seed: int = WAVE_SEED):
    """(rc, bytes) of the serial or the 64-lane decode into a buffer of `cap` bytes; the GUARD bytes behind it must come back untouched, and
    so must the rest of the buffer behind the bytes of an accepted stream"""
    buf = (C.c_uint8 * (cap + GUARD))()
    C.memset(buf, 0xA5, cap + GUARD)
    w = C.c_uint32(0)
    L = _lib()
    rc = L.emu_inflate_wave(comp, len(comp), buf, cap, C.byref(w), seed) if wave else L.emu_inflate(comp, len(comp), buf, cap, C.byref(w))
    assert C.string_at(C.addressof(buf) + cap, GUARD) == b"\xa5" * GUARD, "write beyond the output buffer"
    if rc != 0:
        return rc, b""
    assert w.value <= cap
    assert C.string_at(C.addressof(buf) + w.value, cap - w.value) == b"\xa5" * (cap - w.value), "write behind the inflated bytes"
    return 0, C.string_at(buf, w.value)


def run_asan(cases, tmp_dir: str, procs: int = 4):
    """cases: (stream, cap, wave seed or 0) -> (return code, stderr, per case [(rc, bytes) of the serial decode, then of the wave's if asked for])"""
    exe = build_asan()
    parts = min(procs, max(1, len(cases)))  # the cases dealt out to `procs` runs of the program side by side: the emulated wave is slow under ASan
    runs = []
    for p in range(parts):
        pin, pout = os.path.join(tmp_dir, f"inf_asan_in{p}.bin"), os.path.join(tmp_dir, f"inf_asan_out{p}.bin")
        mine = cases[p::parts]
        with open(pin, "wb") as fh:
            fh.write(struct.pack("<I", len(mine)))
            for comp, cap, wave in mine:
                fh.write(struct.pack("<III", len(comp), cap, wave) + comp)
        runs.append((mine, pout, subprocess.Popen([exe, pin, pout], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)))
    res, code, err_text = [None] * len(cases), 0, ""
    for p, (mine, pout, pr) in enumerate(runs):
        err = pr.communicate(timeout=900)[1]
        if pr.returncode != 0:
            code, err_text = code or pr.returncode, err_text + err
            continue
        raw, at = open(pout, "rb").read(), 0
        for k, (comp, cap, wave) in enumerate(mine):
            one = []
            for _ in range(2 if wave else 1):
                rc, n = struct.unpack_from("<iI", raw, at)
                one.append((rc, raw[at + 8:at + 8 + n]))
                at += 8 + n
            res[p + k * parts] = one
        assert at == len(raw)
    return code, err_text, [] if code else res
