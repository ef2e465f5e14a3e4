"""ctypes binding of tests/emu/libplo_emu_deflate.so: deflate.hpp (the device code of plo_bgzf_compress_dev) executed under the CPU
wave64 emulator.  Built the way emu_records_lib builds its harness.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
_LIB = os.path.join(_HERE, "emu", "libplo_emu_deflate.so")
_ASAN = os.path.join(_HERE, "emu", "emu_deflate_asan")
_lib = None
BLOCK = 0xff00
GUARD = 32


def _sources():
    return [os.path.join(_HERE, "emu", "emu_deflate.cpp"), os.path.join(_HERE, "emu", "plo_wave.hpp")] + [
        os.path.join(ROOT, "portello_amd", "csrc", f) for f in ("deflate.hpp", "inflate.hpp")]


def _stale(target, srcs):
    return (not os.path.exists(target)) or any(os.path.getmtime(s) > os.path.getmtime(target) for s in srcs)


def build(force=False):
    srcs = _sources()
    if force or _stale(_LIB, srcs):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fPIC", "-shared", "-I" + os.path.join(_HERE, "emu"),
                               "-o", _LIB, srcs[0]])
    return _LIB


def build_asan(force=False):
    """the same code as a program with AddressSanitizer and UBSan (CPU only): emu_deflate_asan IN OUT LEVEL | --jobs JOBS OUT LEVEL"""
    srcs = _sources()
    if force or _stale(_ASAN, srcs):
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-DEMU_DEFLATE_MAIN", "-I" + os.path.join(_HERE, "emu"), "-o", _ASAN, srcs[0]])
    return _ASAN


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(_LIB)
        L.emu_bgzf_deflate.restype = C.c_int
        L.emu_bgzf_deflate.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int, C.c_uint, C.POINTER(C.c_uint32)]
        L.emu_bgzf_slot.restype = C.c_uint32
        L.emu_bgzf_work_bytes.restype = C.c_uint32
        L.emu_def_build_code.restype = C.c_int
        L.emu_def_build_code.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_uint, C.c_void_p, C.c_void_p]
        L.emu_def_put.restype = C.c_int
        L.emu_def_put.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint, C.c_void_p]
        L.emu_def_symbols.restype = None
        L.emu_def_symbols.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib = L
    return _lib


def deflate_block(payload: bytes, level: int, order_seed: int = 0, cap=None):
    """one BGZF block of `payload` (<= 0xff00 bytes) -> (code, block bytes); the 32 guard bytes behind the slot are checked"""
    n = len(payload)
    cap = 18 + 5 + n + 8 if cap is None else cap
    buf = (C.c_uint8 * (cap + GUARD + 8))()
    base = C.addressof(buf)
    base += (-base) & 3
    C.memset(base, 0x5A, cap + GUARD)
    size = C.c_uint32(0)
    rc = lib().emu_bgzf_deflate(payload, n, base, cap, level, order_seed, C.byref(size))
    assert C.string_at(base + cap, GUARD) == b"\x5a" * GUARD, "write behind the output slot"
    if rc != 0:
        assert C.string_at(base, cap) == b"\x5a" * cap, "a refused block was written to"
        return rc, b""
    assert size.value <= cap
    assert C.string_at(base + size.value, cap - size.value) == b"\x5a" * (cap - size.value), "write behind the block"
    return 0, C.string_at(base, size.value)


def compress(data: bytes, level: int, order_seed: int = 0) -> list:
    """`data` cut into 0xff00-byte payloads, the last one short: the list of their BGZF blocks (what plo_bgzf_compress_dev returns, densely packed)"""
    out = []
    for at in range(0, len(data), BLOCK):
        rc, blk = deflate_block(data[at:at + BLOCK], level, order_seed)
        assert rc == 0, rc
        out.append(blk)
    return out


def run_asan(data: bytes, level: int, tmp_dir: str):
    """(return code, stderr, blocks' bytes) of the sanitizer build over `data`"""
    exe = build_asan()
    pin, pout = os.path.join(tmp_dir, "def_asan_in.bin"), os.path.join(tmp_dir, "def_asan_out.bin")
    with open(pin, "wb") as fh:
        fh.write(data)
    pr = subprocess.run([exe, pin, pout, str(level)], capture_output=True, text=True, timeout=900)
    if pr.returncode != 0:
        return pr.returncode, pr.stderr, b""
    return 0, pr.stderr, open(pout, "rb").read()


# ---- direct entries ------------------------------------------------------------------------------------------------------------------------
PUT_GUARD = 4  # words behind cap_words that emu_def_put must leave alone


def build_code(freq, limit: int, order_seed: int = 0):
    """def_build_code over `freq` as a wave -> (lengths, codes as they enter the stream: bit-reversed)"""
    import numpy as np

    n = len(freq)
    f = np.ascontiguousarray(freq, np.uint32)
    ln, code = np.full(n, 0xEE, np.uint8), np.full(n, 0xEEEE, np.uint16)
    rc = lib().emu_def_build_code(f.ctypes.data, n, limit, order_seed, ln.ctypes.data, code.ctypes.data)
    assert rc == 0, rc
    return [int(x) for x in ln], [int(x) for x in code]


def put(calls, cap_words: int, order_seed: int = 0):
    """calls: a list of wave-wide def_put calls, each a list of 64 (value, bits) -> (the cap_words words as bytes, bits written, open word);
    the words behind cap_words are checked"""
    import numpy as np

    v = np.array([[c[0] for c in call] for call in calls], np.uint64).reshape(-1)
    nb = np.array([[c[1] for c in call] for call in calls], np.uint32).reshape(-1)
    assert len(v) == 64 * len(calls)
    out = np.full(cap_words + PUT_GUARD, 0x5A5A5A5A, np.uint32)
    out[:cap_words] = 0
    res = np.zeros(2, np.uint32)
    rc = lib().emu_def_put(v.ctypes.data, nb.ctypes.data, len(calls), out.ctypes.data, cap_words, order_seed, res.ctypes.data)
    assert rc == 0, rc
    assert np.all(out[cap_words:] == 0x5A5A5A5A), "def_put wrote behind cap_words"
    return out[:cap_words].tobytes(), int(res[0]), int(res[1])


def symbols():
    """(lens[256][3], dists[32768][3], extra[59]): def_len_code / def_dist_code over their domains, def_len_extra / def_dist_extra"""
    import numpy as np

    lens, dists, extra = np.zeros((256, 3), np.uint32), np.zeros((32768, 3), np.uint32), np.zeros(59, np.uint32)
    lib().emu_def_symbols(lens.ctypes.data, dists.ctypes.data, extra.ctypes.data)
    return lens, dists, extra


def job_payload(p: bytes) -> bytes:
    import struct

    return struct.pack("<II", 1, len(p)) + p


def job_table(freq, limit: int) -> bytes:
    import struct

    return struct.pack(f"<III{len(freq)}I", 2, len(freq), limit, *freq)


def job_put(calls, cap_words: int) -> bytes:
    import struct

    flat = [c for call in calls for c in call]
    return struct.pack("<III", 3, len(calls), cap_words) + struct.pack(f"<{len(flat)}Q", *[c[0] for c in flat]) + struct.pack(f"<{len(flat)}I", *[c[1] for c in flat])


def run_asan_jobs(jobs: bytes, level: int, tmp_dir: str):
    """(return code, stderr, list of the records' results) of the sanitizer build over a file of job records (emu_deflate.cpp, run_jobs)"""
    import struct

    exe = build_asan()
    pin, pout = os.path.join(tmp_dir, "def_asan_jobs.bin"), os.path.join(tmp_dir, "def_asan_jobs_out.bin")
    with open(pin, "wb") as fh:
        fh.write(jobs)
    pr = subprocess.run([exe, "--jobs", pin, pout, str(level)], capture_output=True, text=True, timeout=900)
    if pr.returncode != 0:
        return pr.returncode, pr.stderr, []
    raw, at, out = open(pout, "rb").read(), 0, []
    while at < len(raw):
        n = struct.unpack_from("<I", raw, at)[0]
        out.append(raw[at + 4:at + 4 + n])
        at += 4 + n
    assert at == len(raw)
    return 0, pr.stderr, out
