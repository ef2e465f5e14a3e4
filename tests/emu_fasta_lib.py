"""ctypes binding of tests/emu/libplo_emu_fasta.so: fasta_core.hpp (the device code and the host's carry of plo_fasta_*) executed under the
CPU wave64 emulator.  Built the way emu_index_lib builds its harness.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C
import os
import struct
import subprocess
from dataclasses import dataclass, field

import numpy as np

import emu_records_lib as erl
import fasta_expect as fx

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
_LIB = os.path.join(_HERE, "emu", "libplo_emu_fasta.so")
_ASAN = os.path.join(_HERE, "emu", "emu_fasta_asan")
_lib = None
_FLAGS = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas"]


def _sources():
    return [os.path.join(_HERE, "emu", "emu_fasta.cpp"), os.path.join(_HERE, "emu", "plo_wave.hpp"), os.path.join(ROOT, "portello_amd", "csrc", "fasta_core.hpp")]


def build(force=False):
    srcs = _sources()
    if force or erl._stale(_LIB, srcs):
        subprocess.check_call(_FLAGS + ["-fPIC", "-shared", "-I" + os.path.join(_HERE, "emu"), "-o", _LIB, srcs[0]])
    return _LIB


def build_asan(force=False):
    """the same code as a program with AddressSanitizer and UBSan (CPU only): emu_fasta_asan IN OUT"""
    srcs = _sources()
    if force or erl._stale(_ASAN, srcs):
        subprocess.check_call(_FLAGS + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-DEMU_FASTA_MAIN",
                                        "-I" + os.path.join(_HERE, "emu"), "-o", _ASAN, srcs[0]])
    return _ASAN


def lib():
    global _lib
    if _lib is None:
        build()
        L = C.CDLL(_LIB)
        L.emu_fasta_tile.restype = C.c_uint32
        L.emu_fasta_many.restype = C.c_longlong
        L.emu_fasta_many.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
        _lib = L
    return _lib


def tile() -> int:
    """FA_TILE of the build"""
    return int(lib().emu_fasta_tile())


@dataclass
class Got:
    status: int = 0
    err_kind: int = 0
    err_offset: int = 0
    err_chrom: int = 0
    err_len: int = 0
    canary_ok: bool = True
    n_bases: int = 0
    text_bytes: int = 0
    ids: list = field(default_factory=list)
    lens: list = field(default_factory=list)
    wants: list = field(default_factory=list)
    chrom_dst: list = field(default_factory=list)
    chrom_len: list = field(default_factory=list)
    alloc: bytes = b""

    def chrom_seq(self):
        return [self.alloc[d:d + n] for d, n in zip(self.chrom_dst, self.chrom_len)]


def parse_blob(blob: bytes) -> Got:
    g = Got()
    g.status, g.err_kind, g.err_offset, g.err_chrom, ok, g.err_len, n_rec, g.n_bases, g.text_bytes = struct.unpack_from("<iiQIIqQQQ", blob, 0)
    g.canary_ok = bool(ok)
    at = struct.calcsize("<iiQIIqQQQ")
    for _ in range(n_rec):
        (ln,) = struct.unpack_from("<I", blob, at)
        at += 4
        g.ids.append(bytes(blob[at:at + ln]))
        at += ln
        length, want = struct.unpack_from("<qi", blob, at)
        at += 12
        g.lens.append(length)
        g.wants.append(want)
    (nc,) = struct.unpack_from("<I", blob, at)
    at += 4
    for _ in range(nc):
        d, n = struct.unpack_from("<qq", blob, at)
        at += 16
        g.chrom_dst.append(d)
        g.chrom_len.append(n)
    (na,) = struct.unpack_from("<Q", blob, at)
    at += 8
    g.alloc = bytes(blob[at:at + na])
    assert at + na == len(blob)
    return g


def _pieces(n, cuts):
    """cuts: None (one piece), or the pieces' lengths"""
    if cuts is None:
        return [n]
    assert sum(cuts) == n, (sum(cuts), n)
    return list(cuts)


def _blob_cap(text, want_lens):
    return 8192 + 2 * len(text) + 600 * (text.count(b">") + len(want_lens or []) + 2) + sum(fx.slot_bytes(x) for x in (want_lens or []))


def _pack(cases) -> bytes:
    out = [struct.pack("<I", len(cases))]
    for c in cases:
        text = c["text"]
        pieces = _pieces(len(text), c.get("cuts"))
        names = c.get("want_names")
        out.append(struct.pack("<QIIIIII", len(text), len(pieces), int(names is not None), len(names or []), c.get("order_seed", 0), c.get("n_waves", 2),
                               int(c.get("vec", True))))
        out.append(np.ascontiguousarray(pieces, "<u8").tobytes() + text)
        for w, ln in zip(names or [], c.get("want_lens") or []):
            w = w if isinstance(w, bytes) else w.encode()
            out.append(struct.pack("<I", len(w)) + w + struct.pack("<q", ln))
    return b"".join(out)


def _unpack(blob: bytes, n: int):
    at, res = 0, []
    for _ in range(n):
        (nb,) = struct.unpack_from("<Q", blob, at)
        at += 8
        res.append(parse_blob(blob[at:at + nb]))
        at += nb
    assert at == len(blob)
    return res


def load_many(cases):
    """cases: [dict(text=, want_names=, want_lens=, cuts=, order_seed=, n_waves=, vec=)] through the emulated loader -> [Got].  The cases of
    one order_seed share their emulator runs (a run's set-up costs more than a small piece does): many small cases cost little more than one."""
    data = _pack(cases)
    cap = 64 + sum(_blob_cap(c["text"], c.get("want_lens")) for c in cases)
    src, out = np.frombuffer(data, np.uint8), np.zeros(cap, np.uint8)
    n = lib().emu_fasta_many(src.ctypes.data, len(data), out.ctypes.data, cap)
    assert n >= 0, n
    return _unpack(out[:n].tobytes(), len(cases))


def load(text: bytes, want_names=None, want_lens=None, cuts=None, order_seed=0, n_waves=2, vec=True) -> Got:
    """the text through the emulated loader, fed in pieces of the lengths `cuts`"""
    return load_many([dict(text=text, want_names=want_names, want_lens=want_lens, cuts=cuts, order_seed=order_seed, n_waves=n_waves, vec=vec)])[0]


def run_asan(cases, tmp_dir: str):
    """the cases of load_many through the sanitizer build in one process -> (return code, stderr, [Got])"""
    exe = build_asan()
    pin, pout = os.path.join(tmp_dir, "fasta_asan_in.bin"), os.path.join(tmp_dir, "fasta_asan_out.bin")
    with open(pin, "wb") as fh:
        fh.write(_pack(cases))
    pr = subprocess.run([exe, pin, pout], capture_output=True, text=True, timeout=600)
    if pr.returncode != 0:
        return pr.returncode, pr.stderr, None
    return 0, pr.stderr, _unpack(open(pout, "rb").read(), len(cases))
