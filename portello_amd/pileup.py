"""Allele pileup of the output records on the device (plo_pileup_*, include/portello_liftover.h): DevicePileup wraps one pileup object --
eight int32 counters per reference base (A C G T N DEL INS CLIP), events only --, and write_sites turns its candidate sites into
<prefix>.sites.tsv."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi
from .api import PortelloError


class DevicePileup:
    """Eight counters per base for a list of chromosomes (ref_len in the output header's @SQ order), or for at most one region
    (ref_id, beg, end) of each, on the device of `engine`: 32 bytes a base.  The reference is the adding engine's index: its chrom_seq must
    have the same chromosomes.  add() from any engine of that device, from several threads at once; sites(), reset() and close() must not
    overlap an add: join the adding threads first.  There is no finish step."""

    def __init__(self, engine, ref_len, regions=None, exclude_flags: int = abi.DEPTH_EXCLUDE_DEFAULT):
        self.lib = engine.lib
        self.engine = engine
        self.ref_len = [int(n) for n in ref_len]
        rl = np.ascontiguousarray(self.ref_len, np.int32) if self.ref_len else np.zeros(1, np.int32)
        regions = [tuple(int(x) for x in r) for r in regions] if regions else []
        rg = (abi.PloPileupRegion * max(1, len(regions)))(*[abi.PloPileupRegion(*r) for r in regions])
        opts = abi.PloPileupOpts(int(exclude_flags), len(regions), C.cast(rg, C.POINTER(abi.PloPileupRegion)))
        h = C.c_void_p()
        self.handle = None
        self._check(engine, self.lib.plo_pileup_create(engine.handle, len(self.ref_len), rl.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(opts), C.byref(h)), "plo_pileup_create")
        self.handle = h

    def _check(self, engine, st: int, what: str, out=None):
        if st != abi.PLO_OK:
            msg = self.lib.plo_last_error(engine.handle)
            e = PortelloError(st, f"{what}: {msg.decode() if msg else ''}")
            if out is not None:
                e.err_record, e.err_kind = int(out.err_record), int(out.err_kind)
            raise e

    def info(self) -> abi.PloPileupInfo:
        info = abi.PloPileupInfo()
        st = self.lib.plo_pileup_info_get(self.handle, C.byref(info))
        if st != abi.PLO_OK:
            raise PortelloError(st, "plo_pileup_info_get")
        return info

    def add_dev(self, engine, bytes_ptr, n_bytes: int, n_records: int, record_off_ptr) -> abi.PloPileupAddOut:
        """The records at the DEVICE address `bytes_ptr` (records_build_dev's or records_sort_dev's bytes / record_off, in any order) on
        `engine`'s stream.  A record the device check refuses raises PortelloError with status PLO_ERR_INVALID_ARG, the lowest such record
        in `err_record` and what it broke in `err_kind`; such a call adds nothing."""
        din = abi.PloDepthIn(C.cast(bytes_ptr, abi._u8p), int(n_bytes), int(n_records), C.cast(record_off_ptr, abi._u64p))
        out = abi.PloPileupAddOut()
        self._check(engine, self.lib.plo_pileup_add_dev(engine.handle, self.handle, C.byref(din), C.byref(out)), "plo_pileup_add_dev", out)
        return out

    def add(self, records, engine=None) -> abi.PloPileupAddOut:
        """records: anything with bytes, n_bytes, n_records and record_off (plo_records_out, plo_sort_out), on the object's engine or `engine`"""
        return self.add_dev(engine or self.engine, records.bytes, records.n_bytes, records.n_records, records.record_off)

    def sites_dev(self, depth=None, channel_mask: int = abi.PILEUP_MASK_DEFAULT, min_count: int = 1, min_frac=(0, 1), engine=None) -> abi.PloPileupSitesOut:
        engine = engine or self.engine
        opts = abi.PloPileupSitesOpts(int(channel_mask), int(min_count), int(min_frac[0]), int(min_frac[1]))
        out = abi.PloPileupSitesOut()
        dh = depth.handle if depth is not None else None
        self._check(engine, self.lib.plo_pileup_sites_dev(engine.handle, self.handle, dh, C.byref(opts), C.byref(out)), "plo_pileup_sites_dev")
        return out

    def sites(self, depth=None, channel_mask: int = abi.PILEUP_MASK_DEFAULT, min_count: int = 1, min_frac=(0, 1), engine=None, with_ms: bool = False):
        """The candidate sites as a host array of abi.PILEUP_SITE_DTYPE, ordered by (ref_id, pos).  With m the largest counter among the
        channels of channel_mask, a base is a site iff m >= min_count and -- with a FINISHED depth.DeviceDepth over the same chromosomes and
        min_frac = (num, den), num != 0 -- m * den >= num * depth.  with_ms: and the HIP-event time of the call."""
        engine = engine or self.engine
        out = self.sites_dev(depth, channel_mask, min_count, min_frac, engine)
        n = int(out.n_sites)
        arr = engine.download(out.site, np.uint8, 48 * n).view(abi.PILEUP_SITE_DTYPE) if n else np.zeros(0, abi.PILEUP_SITE_DTYPE)
        return (arr, float(out.sites_ms)) if with_ms else arr

    def array(self, engine=None) -> np.ndarray:
        """a host copy of the whole array, [n_bases, 8] (tests and small references only)"""
        info = self.info()
        n = int(info.n_bases)
        return (engine or self.engine).download(info.array, np.int32, 8 * n).reshape(-1, 8) if n else np.zeros((0, 8), np.int32)

    def reset(self, engine=None):
        engine = engine or self.engine
        self._check(engine, self.lib.plo_pileup_reset(engine.handle, self.handle), "plo_pileup_reset")

    def close(self):
        if getattr(self, "handle", None):
            self.lib.plo_pileup_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


SITES_HEADER = "#chrom\tpos\tend\tref\tdepth\tA\tC\tG\tT\tN\tDEL\tINS\tCLIP\n"


def write_sites(path: str, ref_names, sites: np.ndarray):
    """<prefix>.sites.tsv: a '#' header line, then chrom, pos, pos + 1, the reference byte (a byte that is no printable ASCII: N), the depth
    (-1 without a depth object) and the eight counters of every site, tab-separated, in the sites' order"""
    with open(path, "w") as fh:
        fh.write(SITES_HEADER)
        at, step = 0, 1 << 16
        while at < len(sites):
            part = sites[at:at + step]
            fh.write("".join("%s\t%d\t%d\t%s\t%d\t%s\n" % (ref_names[r], p, p + 1, chr(b) if 33 <= b < 127 else "N", d, "\t".join(map(str, c)))
                             for r, p, b, d, c in zip(part["ref_id"].tolist(), part["pos"].tolist(), part["ref_base"].tolist(), part["depth"].tolist(), part["count"].tolist())))
            at += step
