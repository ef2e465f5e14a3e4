"""tests/emu/emu_liftover.cpp: the liftover catalogue through the emulated lane, window and streaming routes as a stand-alone program with
AddressSanitizer and UBSan, built and run the way emu_enumerate_lib builds and runs its program (whose file format it shares).  TEST
INFRASTRUCTURE ONLY."""
import os
import subprocess

import emu_enumerate_lib as el
from portello_amd import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
_ASAN = os.path.join(_HERE, "emu", "emu_liftover_asan")
MODES = ("lanes32", "lanes16", "window64", "stream1")


def build_asan(force=False):
    srcs = [os.path.join(_HERE, "emu", "emu_liftover.cpp")] + el._sources()[1:]
    stale = (not os.path.exists(_ASAN)) or any(os.path.getmtime(s) > os.path.getmtime(_ASAN) for s in srcs)
    if force or stale:
        # (_GLIBCXX_SANITIZE_VECTOR: a read behind a vector's size, inside its capacity, is an error too)
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-D_GLIBCXX_SANITIZE_VECTOR", "-I" + os.path.join(_HERE, "emu"),
                               "-o", _ASAN, srcs[0]])
    return _ASAN


def run_asan(index, cases, tmp_dir, heavy_max_w, name="lift"):
    """cases: (abi.BatchData, stages) pairs -> (exit status, stderr text, per case [(rc, retried items, abi.BatchResult) per mode of MODES;
    the first three for a stage set other than STAGES_ALL])"""
    exe = build_asan()
    src, dst = os.path.join(str(tmp_dir), name + ".in"), os.path.join(str(tmp_dir), name + ".out")
    with open(src, "wb") as fh:
        fh.write(el.encode(index, cases, heavy_max_w))
    p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=900)
    res = None
    if p.returncode == 0:
        with open(dst, "rb") as fh:
            res = el.decode(fh.read(), len(cases), [len(MODES) if st == abi.STAGES_ALL else 3 for _, st in cases])
    return p.returncode, p.stderr, res
