"""Depth of the output records on the device (plo_depth_*, include/portello_liftover.h): DeviceDepth wraps one depth object, and the two
writers turn its results into the files mosdepth leaves -- <prefix>.per-base.bed and <prefix>.regions.bed."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi
from .api import PortelloError


class DeviceDepth:
    """One int32 array for a list of chromosomes (ref_len in the output header's @SQ order) on the device of `engine`.  Open: add() from any
    engine of that device, from several threads at once; then finish() once; then windows() / runs().  finish, windows, runs, reset and
    close must not overlap an add: join the adding threads first."""

    def __init__(self, engine, ref_len, exclude_flags: int = abi.DEPTH_EXCLUDE_DEFAULT, count_deletions: bool = False):
        self.lib = engine.lib
        self.ref_len = [int(n) for n in ref_len]
        rl = np.ascontiguousarray(self.ref_len, np.int32) if self.ref_len else np.zeros(1, np.int32)
        opts = abi.PloDepthOpts(int(exclude_flags), 1 if count_deletions else 0)
        h = C.c_void_p()
        self.handle = None
        self._check(engine, self.lib.plo_depth_create(engine.handle, len(self.ref_len), rl.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(opts), C.byref(h)), "plo_depth_create")
        self.handle = h

    def _check(self, engine, st: int, what: str, out=None):
        if st != abi.PLO_OK:
            msg = self.lib.plo_last_error(engine.handle)
            e = PortelloError(st, f"{what}: {msg.decode() if msg else ''}")
            if out is not None:
                e.err_record, e.err_kind = int(out.err_record), int(out.err_kind)
            raise e

    def info(self) -> abi.PloDepthInfo:
        info = abi.PloDepthInfo()
        st = self.lib.plo_depth_info_get(self.handle, C.byref(info))
        if st != abi.PLO_OK:
            raise PortelloError(st, "plo_depth_info_get")
        return info

    def add(self, engine, bytes_ptr, n_bytes: int, n_records: int, record_off_ptr) -> abi.PloDepthAddOut:
        """The records at the DEVICE address `bytes_ptr` (records_build_dev's or records_sort_dev's bytes / record_off, in any order) on
        `engine`'s stream.  A record the device check refuses raises PortelloError with status PLO_ERR_INVALID_ARG, the lowest such record
        in `err_record` and what it broke in `err_kind`; such a call adds nothing."""
        din = abi.PloDepthIn(C.cast(bytes_ptr, abi._u8p), int(n_bytes), int(n_records), C.cast(record_off_ptr, abi._u64p))
        out = abi.PloDepthAddOut()
        self._check(engine, self.lib.plo_depth_add_dev(engine.handle, self.handle, C.byref(din), C.byref(out)), "plo_depth_add_dev", out)
        return out

    def finish(self, engine) -> float:
        """differences -> depths, in place; -> the HIP-event time in ms"""
        ms = C.c_float(0)
        self._check(engine, self.lib.plo_depth_finish_dev(engine.handle, self.handle, C.byref(ms)), "plo_depth_finish_dev")
        return float(ms.value)

    def windows(self, engine, window: int):
        """-> (win_first [n_ref + 1], sums [n_windows], ms): host copies"""
        out = abi.PloDepthWindowsOut()
        self._check(engine, self.lib.plo_depth_windows_dev(engine.handle, self.handle, int(window), C.byref(out)), "plo_depth_windows_dev")
        n = int(out.n_windows)
        first = np.ctypeslib.as_array(out.win_first, (len(self.ref_len) + 1,)).copy()
        sums = np.ctypeslib.as_array(out.sum, (n,)).copy() if n else np.zeros(0, np.uint64)
        return first, sums, float(out.windows_ms)

    def runs_dev(self, engine) -> abi.PloDepthRunsOut:
        out = abi.PloDepthRunsOut()
        self._check(engine, self.lib.plo_depth_runs_dev(engine.handle, self.handle, C.byref(out)), "plo_depth_runs_dev")
        return out

    def runs(self, engine, with_ms: bool = False):
        """the runs as a host array of abi.DEPTH_RUN_DTYPE (with_ms: and the HIP-event time of the call)"""
        out = self.runs_dev(engine)
        n = int(out.n_runs)
        arr = engine.download(out.run, np.uint8, 16 * n).view(abi.DEPTH_RUN_DTYPE) if n else np.zeros(0, abi.DEPTH_RUN_DTYPE)
        return (arr, float(out.runs_ms)) if with_ms else arr

    def array(self, engine) -> np.ndarray:
        """a host copy of the whole array (tests and small references only)"""
        info = self.info()
        return engine.download(info.array, np.int32, int(info.n_entries))

    def reset(self, engine):
        self._check(engine, self.lib.plo_depth_reset(engine.handle, self.handle), "plo_depth_reset")

    def close(self):
        if getattr(self, "handle", None):
            self.lib.plo_depth_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def format_mean(total: int, n: int) -> str:
    """total / n with two decimals.  The quotient is rounded half to even on its exact value: 100 * total is divided in integers, and a
    remainder of exactly n / 2 rounds to the even neighbour (1 / 8 -> 0.12, 3 / 8 -> 0.38).  No float enters."""
    q, rem = divmod(100 * int(total), int(n))
    if 2 * rem > n or (2 * rem == n and (q & 1)):
        q += 1
    return "%d.%02d" % (q // 100, q % 100)


def write_per_base(path: str, names, runs: np.ndarray):
    """<prefix>.per-base.bed: chrom, beg, end, depth of every run, tab-separated, in the runs' order"""
    with open(path, "w") as fh:
        at, step = 0, 1 << 16
        while at < len(runs):
            part = runs[at:at + step]
            fh.write("".join("%s\t%d\t%d\t%d\n" % (names[r], b, e, d) for r, b, e, d in zip(part["ref_id"].tolist(), part["beg"].tolist(), part["end"].tolist(), part["depth"].tolist())))
            at += step


def write_regions(path: str, names, ref_len, window: int, win_first, sums):
    """<prefix>.regions.bed: chrom, beg, end, mean depth (format_mean) of every window, the last one of a chromosome short"""
    with open(path, "w") as fh:
        for r, n in enumerate(ref_len):
            lo = int(win_first[r])
            s = sums[lo:int(win_first[r + 1])].tolist()
            fh.write("".join("%s\t%d\t%d\t%s\n" % (names[r], j * window, min(n, (j + 1) * window), format_mean(t, min(n, (j + 1) * window) - j * window)) for j, t in enumerate(s)))
