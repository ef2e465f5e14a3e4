"""ctypes binding of tests/emu/libplo_emu_pileup.so: pileup_core.hpp (the device code of plo_pileup_*) executed under the CPU wave64 emulator,
with PLO_PILEUP_TILE = TILE so that small inputs reach the tile seams of the sites.  Built the way emu_depth_lib builds its harness.
TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

import emu_records_lib as erl
import pileup_expect as px
from portello_amd import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
_LIB = os.path.join(_HERE, "emu", "libplo_emu_pileup.so")
_ASAN = os.path.join(_HERE, "emu", "emu_pileup_asan")
_lib = None
TILE = 12
_FLAGS = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-DPLO_PILEUP_TILE=%d" % TILE]


def _sources():
    return [os.path.join(_HERE, "emu", "emu_pileup.cpp"), os.path.join(_HERE, "emu", "plo_wave.hpp"), os.path.abspath(__file__)] + [
        os.path.join(ROOT, "portello_amd", "csrc", f) for f in ("pileup_core.hpp", "depth_core.hpp", "aln_walk.hpp", "nm_core.hpp", "index_core.hpp", "batch_core.hpp", "sort_core.hpp",
                                                                "records_core.hpp", "finish_core.hpp", "lift_core.hpp", "lift_types.hpp")]


def build(force=False):
    srcs = _sources()
    if force or erl._stale(_LIB, srcs):
        subprocess.check_call(_FLAGS + ["-fPIC", "-shared", "-I" + os.path.join(_HERE, "emu"), "-o", _LIB, srcs[0]])
    return _LIB


def build_asan(force=False):
    """the same code as a program with AddressSanitizer and UBSan (CPU only): emu_pileup_asan IN OUT"""
    srcs = _sources()
    if force or erl._stale(_ASAN, srcs):
        subprocess.check_call(_FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-DEMU_PILEUP_MAIN",
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
        L.emu_pileup_tile.restype = C.c_uint
        L.emu_pileup_create.restype = C.c_void_p
        L.emu_pileup_create.argtypes = [C.c_uint32, _i32p, _u8p, C.c_uint32, C.c_uint32, _i32p, C.POINTER(C.c_int)]
        L.emu_pileup_destroy.argtypes = [C.c_void_p]
        L.emu_pileup_destroy.restype = None
        L.emu_pileup_bases.restype = C.c_uint64
        L.emu_pileup_bases.argtypes = [C.c_void_p]
        L.emu_pileup_slots.argtypes = [C.c_void_p, _u64p, _i32p, _i32p]
        L.emu_pileup_slots.restype = None
        L.emu_pileup_array.argtypes = [C.c_void_p, _i32p]
        L.emu_pileup_array.restype = None
        L.emu_pileup_reset.argtypes = [C.c_void_p]
        L.emu_pileup_add.argtypes = [C.c_void_p, _u8p, C.c_uint64, C.c_uint32, _u64p, C.c_uint, C.c_uint32, _u32p, _u32p, _u32p, _u64p]
        L.emu_pileup_sites.argtypes = [C.c_void_p, _i32p, C.c_int, C.c_uint32, C.c_int32, C.c_uint32, C.c_uint32, C.c_uint, _u64p]
        L.emu_pileup_sites_copy.argtypes = [C.c_void_p, _u8p]
        L.emu_pileup_sites_copy.restype = None
        assert L.emu_pileup_tile() == TILE
        _lib = L
    return _lib


def _regions(regions):
    rg = np.ascontiguousarray([list(r) for r in regions], np.int32).reshape(-1) if regions else np.zeros(3, np.int32)
    return rg, len(regions) if regions else 0


class CreateRefused(Exception):
    pass


class EmuPileup:
    """a pileup object whose kernels are emulated waves; chroms: the chromosomes' bytes.  The statuses are the C ABI's (-4: the waves' adds
    and the one-thread rule's differ, in the array or in n_events)"""

    def __init__(self, chroms, regions=None, exclude=px.EXCLUDE_DEFAULT, ref_len=None):
        self.chroms = [bytes(c) for c in chroms]
        self.ref_len = [len(c) for c in self.chroms] if ref_len is None else list(ref_len)
        rl = np.ascontiguousarray(self.ref_len, np.int32) if self.ref_len else np.zeros(1, np.int32)
        cat = np.frombuffer(b"".join(self.chroms) or b"\0", np.uint8).copy()
        rg, n_rg = _regions(regions)
        st = C.c_int(0)
        self.h = lib().emu_pileup_create(len(self.ref_len), _p(rl, C.c_int32), _p(cat, C.c_uint8), exclude, n_rg, _p(rg, C.c_int32), C.byref(st))
        if not self.h:
            raise CreateRefused(st.value)

    def close(self):
        if self.h:
            lib().emu_pileup_destroy(self.h)
            self.h = None

    def slots(self):
        """-> (slot_beg, slot_end, slot_off) as lists"""
        n = len(self.ref_len)
        off, beg, end = np.zeros(n + 1, np.uint64), np.zeros(max(1, n), np.int32), np.zeros(max(1, n), np.int32)
        lib().emu_pileup_slots(self.h, _p(off, C.c_uint64), _p(beg, C.c_int32), _p(end, C.c_int32))
        return beg[:n].tolist(), end[:n].tolist(), off.tolist()

    def array(self):
        n = lib().emu_pileup_bases(self.h)
        out = np.zeros((max(1, n), 8), np.int32)
        lib().emu_pileup_array(self.h, _p(out, C.c_int32))
        return out[:n]

    def add(self, data: bytes, off, order_seed=0, n_waves=4):
        """-> (status, n_counted, err_record, err_kind, n_events); the records lie in a buffer of their exact size"""
        raw = np.frombuffer(data, np.uint8).copy() if len(data) else np.zeros(1, np.uint8)
        offs = np.ascontiguousarray(off, np.uint64)
        nc, er, ek, ne = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
        st = lib().emu_pileup_add(self.h, _p(raw, C.c_uint8), len(data), len(off) - 1, _p(offs, C.c_uint64), int(order_seed), int(n_waves), C.byref(nc), C.byref(er), C.byref(ek),
                                  C.byref(ne))
        return st, int(nc.value), int(er.value), int(ek.value), int(ne.value)

    def reset(self):
        return lib().emu_pileup_reset(self.h)

    def sites(self, depth=None, depth_state=1, mask=px.MASK_DEFAULT, min_count=1, num=0, den=1, order_seed=0):
        """depth: per chromosome an array of depths, or None -> (status, sites (pileup_expect.SITE array))"""
        n = C.c_uint64(0)
        dc = None
        if depth is not None:
            dc = np.ascontiguousarray(np.concatenate([np.asarray(d, np.int32) for d in depth] + [np.zeros(1, np.int32)]), np.int32)
        st = lib().emu_pileup_sites(self.h, _p(dc, C.c_int32) if dc is not None else None, int(depth_state), int(mask), int(min_count), int(num), int(den), int(order_seed), C.byref(n))
        out = np.zeros(max(1, n.value), px.SITE)
        if st == abi.PLO_OK and n.value:
            lib().emu_pileup_sites_copy(self.h, out.ctypes.data_as(_u8p))
        return st, out[:n.value]


def run_asan(cases, tmp_dir: str):
    """cases: [dict(chroms, regions, exclude, adds [(data, off, order_seed, n_waves)], depth (per chromosome, or None), mask, min_count, num,
    den, ref_len (None: the chromosomes'))] through the sanitizer build in one process, every array in a heap block of its exact size ->
    (return code, stderr, [dict(create, adds [(status, err_record, err_kind, n_counted, n_events)], array, sites_status, sites)])"""
    exe = build_asan()
    pin, pout = os.path.join(tmp_dir, "pileup_asan_in.bin"), os.path.join(tmp_dir, "pileup_asan_out.bin")
    with open(pin, "wb") as fh:
        fh.write(struct.pack("<I", len(cases)))
        for c in cases:
            chroms = [bytes(x) for x in c["chroms"]]
            ref_len = c.get("ref_len") or [len(x) for x in chroms]
            rg, n_rg = _regions(c.get("regions"))
            depth = c.get("depth")
            fh.write(struct.pack("<IIIIIiIIII", len(ref_len), c.get("exclude", px.EXCLUDE_DEFAULT), n_rg, len(c["adds"]), c.get("mask", px.MASK_DEFAULT), c.get("min_count", 1),
                                 c.get("num", 0), c.get("den", 1), 1 if depth is not None else 0, 0))
            fh.write(np.ascontiguousarray(ref_len, "<i4").tobytes())
            fh.write(rg[:3 * n_rg].astype("<i4").tobytes())
            fh.write(b"".join(chroms))
            if depth is not None:
                fh.write(b"".join(np.asarray(d, "<i4").tobytes() for d in depth))
            for data, off, seed, n_waves in c["adds"]:
                fh.write(struct.pack("<IIIIQ", len(off) - 1, seed, n_waves, 0, len(data)))
                fh.write(np.ascontiguousarray(off, "<u8").tobytes() + data)
    pr = subprocess.run([exe, pin, pout], capture_output=True, text=True, timeout=600)
    if pr.returncode != 0:
        return pr.returncode, pr.stderr, None
    blob, at, res = open(pout, "rb").read(), 0, []
    for c in cases:
        r = {"create": struct.unpack_from("<i", blob, at)[0], "adds": []}
        at += 4
        if r["create"] == abi.PLO_OK:
            for _ in c["adds"]:
                r["adds"].append(struct.unpack_from("<iIIIQ", blob, at))
                at += 24
            nb = struct.unpack_from("<Q", blob, at)[0]
            at += 8
            r["array"] = np.frombuffer(blob, "<i4", nb * 8, at).reshape(-1, 8)
            at += 32 * nb
            r["sites_status"], ns = struct.unpack_from("<iQ", blob, at)
            at += 12
            r["sites"] = np.frombuffer(blob, px.SITE, ns, at)
            at += 48 * ns
        res.append(r)
    assert at == len(blob)
    return 0, pr.stderr, res
