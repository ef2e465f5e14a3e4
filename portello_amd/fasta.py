"""The reference FASTA loaded on the device (plo_fasta_* of include/portello_liftover.h, plo_fasta_load_file of include/portello_bam.h):
`load_reference` gives the upper-cased chromosomes in HBM, in the order and with the lengths of the assembly->reference header, ready for
`bam.Phase1.index_data_device`."""
from __future__ import annotations

import ctypes as C
from typing import Iterable, List, Optional, Sequence

import numpy as np

from . import abi, api

_bound = False


def lib():
    global _bound
    L = api.load_library()
    if not _bound:
        vp = C.c_void_p
        L.plo_fasta_create.restype = C.c_int
        L.plo_fasta_create.argtypes = [C.POINTER(abi.PloFastaWant), C.c_uint64, C.c_int, C.POINTER(vp)]
        L.plo_fasta_feed.restype = C.c_int
        L.plo_fasta_feed.argtypes = [vp, vp, C.c_uint64]
        L.plo_fasta_finish.restype = C.c_int
        L.plo_fasta_finish.argtypes = [vp, C.POINTER(abi.PloFastaOut)]
        L.plo_fasta_record.restype = C.c_int
        L.plo_fasta_record.argtypes = [vp, C.c_uint64, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
        L.plo_fasta_adopt.restype = C.c_int
        L.plo_fasta_adopt.argtypes = [vp, C.c_uint32, C.POINTER(vp), C.POINTER(C.c_int64), C.POINTER(vp)]
        L.plo_fasta_download.restype = C.c_int
        L.plo_fasta_download.argtypes = [vp, vp, vp, C.c_size_t]
        L.plo_fasta_destroy.restype = None
        L.plo_fasta_destroy.argtypes = [vp]
        L.plo_fasta_last_error.restype = C.c_char_p
        L.plo_fasta_last_error.argtypes = [vp]
        L.plo_fasta_load_file.restype = C.c_int
        L.plo_fasta_load_file.argtypes = [C.c_char_p, C.POINTER(abi.PloFastaWant), C.c_uint64, C.c_int, C.POINTER(vp), C.POINTER(abi.PloFastaOut)]
        L.plo_bam_last_error.restype = C.c_char_p
        L.plo_bam_last_error.argtypes = []
        _bound = True
    return L


class FastaError(api.PortelloError):
    """a refused load: what plo_fasta_finish reports (kind = abi.FA_ERR_*)"""

    def __init__(self, status, msg, kind=0, offset=0, chrom=0, length=0):
        super().__init__(status, msg)
        self.kind, self.offset, self.chrom, self.length = kind, offset, chrom, length


def _want(ref_names, ref_lens):
    """-> (PloFastaWant or None, what keeps its arrays alive)"""
    if ref_names is None:
        return None, None
    assert ref_lens is not None and len(ref_names) == len(ref_lens)
    names = (C.c_char_p * max(1, len(ref_names)))(*[n.encode() if isinstance(n, str) else bytes(n) for n in ref_names])
    lens = (C.c_int64 * max(1, len(ref_lens)))(*[int(x) for x in ref_lens])
    w = abi.PloFastaWant(len(ref_names), names, C.cast(lens, C.POINTER(C.c_int64)))
    return w, (names, lens)


class DeviceReference:
    """The chromosomes of a loaded reference in device memory.  An api.Index built from `chrom_ptrs` borrows them: this object has to
    outlive it (bam.Phase1.index_data_device keeps it alive inside the IndexData)."""

    def __init__(self, handle, res: abi.PloFastaOut, device: int):
        self.handle, self.device = handle, device
        L = lib()
        n = int(res.n_chroms)
        self.chrom_len: List[int] = [int(res.chrom_len[i]) for i in range(n)]
        self.chrom_ptrs: List[int] = [int(res.chrom_seq[i] or 0) for i in range(n)]
        self.stats = dict(n_records_seen=int(res.n_records_seen), n_bases=int(res.n_bases), text_bytes=int(res.text_bytes), fasta_ms=float(res.fasta_ms))
        self.record_ids, self.record_lens, self.record_want = [], [], []
        cid, ln, wi = C.c_char_p(), C.c_int64(), C.c_int32()
        for i in range(int(res.n_records_seen)):
            assert L.plo_fasta_record(handle, i, C.byref(cid), C.byref(ln), C.byref(wi)) == abi.PLO_OK
            self.record_ids.append(cid.value)
            self.record_lens.append(int(ln.value))
            self.record_want.append(int(wi.value))
        by_want = {w: rid for rid, w in zip(self.record_ids, self.record_want) if w >= 0}
        self.names: List[str] = [by_want[i].decode(errors="replace") for i in range(n)]

    def adopt(self, arrays: Sequence[Optional[np.ndarray]]) -> List[Optional[int]]:
        """host uint8 arrays -> device pointers of copies this object owns (None stays None)"""
        arrs = [None if a is None else np.ascontiguousarray(a, np.uint8) for a in arrays]
        n = len(arrs)
        src = (C.c_void_p * max(1, n))(*[None if a is None else a.ctypes.data for a in arrs])
        lens = (C.c_int64 * max(1, n))(*[0 if a is None else a.size for a in arrs])
        dst = (C.c_void_p * max(1, n))()
        st = lib().plo_fasta_adopt(self.handle, n, src, lens, dst)
        if st != abi.PLO_OK:
            raise api.PortelloError(st, "plo_fasta_adopt: " + lib().plo_fasta_last_error(self.handle).decode(errors="replace"))
        return [None if a is None else int(dst[i]) for i, a in enumerate(arrs)]

    def download(self, c: int) -> np.ndarray:
        """chromosome c back on the host (tests, tools)"""
        return self.download_bytes(self.chrom_ptrs[c], self.chrom_len[c])

    def download_bytes(self, dev_ptr: int, n: int) -> np.ndarray:
        out = np.zeros(max(1, n), np.uint8)
        st = lib().plo_fasta_download(self.handle, out.ctypes.data, dev_ptr, n)
        if st != abi.PLO_OK:
            raise api.PortelloError(st, "plo_fasta_download: " + lib().plo_fasta_last_error(self.handle).decode(errors="replace"))
        return out[:n]

    def close(self):
        if getattr(self, "handle", None):
            h, self.handle = self.handle, None
            lib().plo_fasta_destroy(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _finish(handle, st: int, res: abi.PloFastaOut, device: int, msg: str) -> DeviceReference:
    if st == abi.PLO_OK:
        return DeviceReference(handle, res, device)
    if handle:
        lib().plo_fasta_destroy(handle)
    raise FastaError(st, msg, int(res.err_kind), int(res.err_offset), int(res.err_chrom), int(res.err_len))


def load_reference(path: str, ref_names: Optional[Sequence[str]] = None, ref_lens: Optional[Sequence[int]] = None, device: int = 0,
                   piece_bytes: int = 0) -> DeviceReference:
    """plo_fasta_load_file: the FASTA at `path` on `device`; ref_names / ref_lens = Phase1.ref_names / .ref_lens (None: every record, in
    file order).  piece_bytes: the size of the pieces the file is read in (0: the library's).  Raises FastaError for a refused text."""
    L = lib()
    want, _keep = _want(ref_names, ref_lens)
    h, res = C.c_void_p(), abi.PloFastaOut()
    st = L.plo_fasta_load_file(path.encode(), C.byref(want) if want is not None else None, int(piece_bytes), device, C.byref(h), C.byref(res))
    return _finish(h if h.value else None, st, res, device, "plo_fasta_load_file: " + L.plo_bam_last_error().decode(errors="replace"))


def load_reference_bytes(pieces: Iterable[bytes], ref_names: Optional[Sequence[str]] = None, ref_lens: Optional[Sequence[int]] = None, device: int = 0,
                         text_bytes_hint: int = 0) -> DeviceReference:
    """the same over plo_fasta_create / _feed / _finish: the text as consecutive pieces of any size"""
    L = lib()
    want, _keep = _want(ref_names, ref_lens)
    h = C.c_void_p()
    st = L.plo_fasta_create(C.byref(want) if want is not None else None, int(text_bytes_hint), device, C.byref(h))
    if st != abi.PLO_OK:
        raise api.PortelloError(st, "plo_fasta_create" + (" (no usable HIP device)" if st == abi.PLO_ERR_NO_DEVICE else ": " + L.plo_fasta_last_error(None).decode(errors="replace")))
    for p in pieces:
        buf = np.frombuffer(bytes(p), np.uint8)
        st = L.plo_fasta_feed(h, buf.ctypes.data if buf.size else None, buf.size)
        if st not in (abi.PLO_OK, abi.PLO_ERR_DATA):
            msg = L.plo_fasta_last_error(h).decode(errors="replace")
            L.plo_fasta_destroy(h)
            raise api.PortelloError(st, "plo_fasta_feed: " + msg)
    res = abi.PloFastaOut()
    st = L.plo_fasta_finish(h, C.byref(res))
    return _finish(h, st, res, device, "plo_fasta_finish: " + L.plo_fasta_last_error(h).decode(errors="replace"))
