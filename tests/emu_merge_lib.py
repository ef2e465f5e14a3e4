"""ctypes binding of tests/emu/libplo_emu_merge.so: merge_core.hpp (the device code of plo_runs_merge_plan_dev / plo_runs_merge_emit_dev)
executed under the CPU wave64 emulator, the two calls issued as engine.hip issues them.  Built the way emu_sort_lib builds its harness.
The library and the sanitizer program take the same blob of cases (tests/emu/emu_merge.cpp).  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

import emu_records_lib as erl

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
_LIB = os.path.join(_HERE, "emu", "libplo_emu_merge.so")
_ASAN = os.path.join(_HERE, "emu", "emu_merge_asan")
_lib = None
_FLAGS = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas"]

NULL_EMPTY, NO_PLAN, NULL_TABLE = 1, 2, 4  # case flags


def _sources():
    return [os.path.join(_HERE, "emu", "emu_merge.cpp"), os.path.join(_HERE, "emu", "plo_wave.hpp")] + [
        os.path.join(ROOT, "portello_amd", "csrc", f) for f in ("merge_core.hpp", "sort_core.hpp", "records_core.hpp", "finish_core.hpp", "lift_core.hpp", "lift_types.hpp")]


def build(force=False):
    srcs = _sources()
    if force or erl._stale(_LIB, srcs):
        subprocess.check_call(_FLAGS + ["-fPIC", "-shared", "-I" + os.path.join(_HERE, "emu"), "-o", _LIB, srcs[0]])
    return _LIB


def build_asan(force=False):
    """the same code as a program with AddressSanitizer and UBSan (CPU only): emu_merge_asan IN OUT"""
    srcs = _sources()
    if force or erl._stale(_ASAN, srcs):
        subprocess.check_call(_FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-DEMU_MERGE_MAIN",
                                        "-I" + os.path.join(_HERE, "emu"), "-o", _ASAN, srcs[0]])
    return _ASAN


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(_LIB)
        L.emu_merge_blob.restype = C.c_int
        L.emu_merge_blob.argtypes = [C.c_char_p, C.c_uint64, C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_uint64)]
        L.emu_merge_free.argtypes = [C.POINTER(C.c_uint8)]
        L.emu_merge_threads.restype = C.c_uint32
        L.emu_merge_max_runs.restype = C.c_uint32
        _lib = L
    return _lib


def threads():
    """MERGE_THREADS: the block size of the key and rank kernels"""
    return int(lib().emu_merge_threads())


def max_runs():
    return int(lib().emu_merge_max_runs())


def case(runs, n_ref, chunk_bytes, emits=(), expect_bytes=b"", order_seed=0, guard=64, flags=0, n_bytes=None):
    """runs: [(data, off)]; n_bytes: what the descriptors say where that is not len(data)"""
    return {"runs": runs, "n_ref": n_ref, "chunk_bytes": chunk_bytes, "emits": list(emits), "expect": expect_bytes, "seed": order_seed, "guard": guard,
            "flags": flags, "n_bytes": n_bytes}


def _pack(cases):
    out = [struct.pack("<I", len(cases))]
    for c in cases:
        out.append(struct.pack("<IIQIIII", len(c["runs"]), c["n_ref"], c["chunk_bytes"], c["seed"], len(c["emits"]), c["guard"], c["flags"]))
        for k, (data, off) in enumerate(c["runs"]):
            offs = np.ascontiguousarray(off, "<u8")
            nb = len(data) if c["n_bytes"] is None else c["n_bytes"][k]
            out.append(struct.pack("<IIQQ", len(offs) - 1, len(offs), nb, len(data)) + offs.tobytes() + data)
        out.append(np.array(c["emits"], "<u4").tobytes() + struct.pack("<Q", len(c["expect"])) + c["expect"])
    return b"".join(out)


def _unpack(blob, cases):
    """-> per case dict(status, err_run, err_record, err_kind, n_records, n_mapped, n_chunks, n_bytes, [src, key, record_off, chunk_first,
    chunk_off], emits: [dict(status, [check, n_records, first, record_off, bytes])])"""
    at, res = 0, []
    for c in cases:
        st, er, ec, ek, n, nm, nc, _, nb = struct.unpack_from("<iIIIIIIIQ", blob, at)
        at += 40
        r = {"status": st, "err_run": er, "err_record": ec, "err_kind": ek, "n_records": n, "n_mapped": nm, "n_chunks": nc, "n_bytes": nb}
        if st == 0:
            for name, dt, cnt in (("src", "<u4", n), ("key", "<u8", n), ("record_off", "<u8", n + 1), ("chunk_first", "<u4", nc + 1), ("chunk_off", "<u8", nc + 1)):
                r[name] = np.frombuffer(blob, dt, cnt, at)
                at += cnt * np.dtype(dt).itemsize
        r["emits"] = []
        for _ in c["emits"]:
            (est,) = struct.unpack_from("<i", blob, at)
            at += 4
            e = {"status": est}
            if est == 0:
                e["check"], e["n_records"], e["first"], enb = struct.unpack_from("<iIIQ", blob, at)
                at += 20
                e["record_off"] = np.frombuffer(blob, "<u8", e["n_records"] + 1, at)
                at += 8 * (e["n_records"] + 1)
                e["bytes"] = bytes(blob[at:at + enb])
                at += enb
            r["emits"].append(e)
        res.append(r)
    assert at == len(blob)
    return res


def run(cases):
    """the cases through the library, every array in a heap block of its exact size, every chunk's output between `guard` canary bytes"""
    blob = _pack(cases)
    out, n = C.POINTER(C.c_uint8)(), C.c_uint64(0)
    rc = lib().emu_merge_blob(blob, len(blob), C.byref(out), C.byref(n))
    assert rc == 0, rc
    try:
        return _unpack(C.string_at(out, n.value), cases)
    finally:
        lib().emu_merge_free(out)


def run_asan(cases, tmp_dir: str):
    """the cases through the sanitizer build, one child process -> (return code, stderr, results or None)"""
    exe = build_asan()
    pin, pout = os.path.join(tmp_dir, "merge_asan_in.bin"), os.path.join(tmp_dir, "merge_asan_out.bin")
    with open(pin, "wb") as fh:
        fh.write(_pack(cases))
    pr = subprocess.run([exe, pin, pout], capture_output=True, text=True, timeout=600)
    if pr.returncode != 0:
        return pr.returncode, pr.stderr, None
    return 0, pr.stderr, _unpack(open(pout, "rb").read(), cases)
