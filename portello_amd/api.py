"""Host-side mirror of the reference's interface for the liftover path.

The three public functions carry the reference's names and argument meaning
(``liftover_read_alignment`` src/liftover_read_alignment.rs:137-141, ``simplify_alignment_indels``
src/simplify_alignment_indels.rs:119-124, ``left_shift_indels``
lib/rust-vc-utils/src/bam_utils/cigar/shift_indels/left_shift_indels.rs:17-22) and are thin conveniences over the
batch entry point: each call becomes a one-item batch for ``plo_liftover_batch`` with the matching stage mask.
All computation happens in the HIP library (``libportello_liftover.so``); if it is missing or no GPU is usable the
calls raise -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from . import abi
from . import cigar as cg

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PLO_LIB") or os.path.join(_HERE, "libportello_liftover.so")  # (PLO_LIB: timing-experiment builds, tools/)

Backend = Callable[[abi.IndexData, abi.BatchData, int], abi.BatchResult]


class PortelloError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__(f"portello_liftover status {status}: {msg}")
        self.status = status


_lib = None


def load_library(path: Optional[str] = None):
    """Load the C-ABI library (built by ``python -m portello_amd.build`` / ``__graft_entry__.build()``)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise PortelloError(abi.PLO_ERR_NO_DEVICE, f"{path} not built: run `python -m portello_amd.build` (hipcc, gfx950)")
    try:
        # In a process that also uses torch, torch's own HIP runtime must be the one the library binds to: loaded the other
        # way round, two runtimes share the process and the engine's one does not see the device.
        import torch  # noqa: F401
    except ImportError:
        pass
    L = C.CDLL(path)
    vp = C.c_void_p
    if not hasattr(L, "plo_api_version") or L.plo_api_version() != abi.PLO_API_VERSION:
        raise PortelloError(abi.PLO_ERR_INVALID_ARG, f"{path} was built for another PLO_API_VERSION than this binding ({abi.PLO_API_VERSION}): rebuild it")
    L.plo_index_create.restype = C.c_int
    L.plo_index_create.argtypes = [C.POINTER(abi.PloIndexDesc), C.c_int, C.POINTER(vp)]
    L.plo_index_destroy.restype = None
    L.plo_index_destroy.argtypes = [vp]
    L.plo_index_segment_map.restype = C.c_int
    L.plo_index_segment_map.argtypes = [vp, C.c_uint32, C.c_uint32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_uint32)]
    L.plo_ctx_create.restype = C.c_int
    L.plo_ctx_create.argtypes = [vp, vp, C.POINTER(vp)]
    L.plo_ctx_destroy.restype = None
    L.plo_ctx_destroy.argtypes = [vp]
    L.plo_liftover_batch.restype = C.c_int
    L.plo_liftover_batch.argtypes = [vp, C.POINTER(abi.PloBatchIn), C.c_uint32, C.POINTER(abi.PloBatchOut)]
    L.plo_liftover_batch_dev.restype = C.c_int
    L.plo_liftover_batch_dev.argtypes = [vp, C.POINTER(abi.PloBatchIn), C.c_uint32, C.POINTER(abi.PloBatchOut)]
    L.plo_compact_output_dev.restype = C.c_int
    L.plo_compact_output_dev.argtypes = [vp, C.POINTER(abi.PloBatchOut)]
    L.plo_host_alloc.restype = C.c_int
    L.plo_host_alloc.argtypes = [C.c_size_t, C.POINTER(C.c_void_p)]
    L.plo_host_free.restype = None
    L.plo_host_free.argtypes = [C.c_void_p]
    L.plo_sa_segments_dev.restype = C.c_int
    L.plo_sa_segments_dev.argtypes = [vp, C.POINTER(abi.PloSaIn), C.POINTER(abi.PloSaOut)]
    L.plo_finish_batch_dev.restype = C.c_int
    L.plo_finish_batch_dev.argtypes = [vp, C.POINTER(abi.PloBatchIn), C.POINTER(abi.PloFinishIn), C.POINTER(abi.PloFinishOut)]
    L.plo_nm_dev.restype = C.c_int
    L.plo_nm_dev.argtypes = [vp, C.POINTER(abi.PloBatchIn), C.POINTER(abi.PloNmOut)]
    L.plo_md_dev.restype = C.c_int
    L.plo_md_dev.argtypes = [vp, C.POINTER(abi.PloBatchIn), C.POINTER(abi.PloMdOut)]
    L.plo_records_sort_dev.restype = C.c_int
    L.plo_records_sort_dev.argtypes = [vp, C.POINTER(abi.PloSortIn), C.POINTER(abi.PloSortOut)]
    L.plo_runs_merge_plan_dev.restype = C.c_int
    L.plo_runs_merge_plan_dev.argtypes = [vp, C.POINTER(abi.PloMergeIn), C.POINTER(abi.PloMergeOut)]
    L.plo_runs_merge_emit_dev.restype = C.c_int
    L.plo_runs_merge_emit_dev.argtypes = [vp, C.c_uint32, C.POINTER(abi.PloMergeChunkOut)]
    L.plo_records_index_dev.restype = C.c_int
    L.plo_records_index_dev.argtypes = [vp, C.POINTER(abi.PloIndexIn), C.POINTER(abi.PloIndexOut)]
    L.plo_depth_create.restype = C.c_int
    L.plo_depth_create.argtypes = [vp, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(abi.PloDepthOpts), C.POINTER(vp)]
    L.plo_depth_destroy.restype = None
    L.plo_depth_destroy.argtypes = [vp]
    L.plo_depth_info_get.restype = C.c_int
    L.plo_depth_info_get.argtypes = [vp, C.POINTER(abi.PloDepthInfo)]
    L.plo_depth_add_dev.restype = C.c_int
    L.plo_depth_add_dev.argtypes = [vp, vp, C.POINTER(abi.PloDepthIn), C.POINTER(abi.PloDepthAddOut)]
    L.plo_depth_finish_dev.restype = C.c_int
    L.plo_depth_finish_dev.argtypes = [vp, vp, C.POINTER(C.c_float)]
    L.plo_depth_windows_dev.restype = C.c_int
    L.plo_depth_windows_dev.argtypes = [vp, vp, C.c_uint32, C.POINTER(abi.PloDepthWindowsOut)]
    L.plo_depth_runs_dev.restype = C.c_int
    L.plo_depth_runs_dev.argtypes = [vp, vp, C.POINTER(abi.PloDepthRunsOut)]
    L.plo_depth_reset.restype = C.c_int
    L.plo_depth_reset.argtypes = [vp, vp]
    L.plo_pileup_create.restype = C.c_int
    L.plo_pileup_create.argtypes = [vp, C.c_uint32, C.POINTER(C.c_int32), C.POINTER(abi.PloPileupOpts), C.POINTER(vp)]
    L.plo_pileup_destroy.restype = None
    L.plo_pileup_destroy.argtypes = [vp]
    L.plo_pileup_info_get.restype = C.c_int
    L.plo_pileup_info_get.argtypes = [vp, C.POINTER(abi.PloPileupInfo)]
    L.plo_pileup_reset.restype = C.c_int
    L.plo_pileup_reset.argtypes = [vp, vp]
    L.plo_pileup_add_dev.restype = C.c_int
    L.plo_pileup_add_dev.argtypes = [vp, vp, C.POINTER(abi.PloDepthIn), C.POINTER(abi.PloPileupAddOut)]
    L.plo_pileup_sites_dev.restype = C.c_int
    L.plo_pileup_sites_dev.argtypes = [vp, vp, vp, C.POINTER(abi.PloPileupSitesOpts), C.POINTER(abi.PloPileupSitesOut)]
    L.plo_eqx_dev.restype = C.c_int
    L.plo_eqx_dev.argtypes = [vp, C.POINTER(abi.PloBatchIn), C.POINTER(abi.PloEqxOut)]
    L.plo_records_build_dev.restype = C.c_int
    L.plo_records_build_dev.argtypes = [vp, C.POINTER(abi.PloBatchIn), C.POINTER(abi.PloRecordsIn), C.POINTER(abi.PloRecordsOut)]
    L.plo_bgzf_inflate_dev.restype = C.c_int
    L.plo_bgzf_inflate_dev.argtypes = [vp, C.POINTER(abi.PloBgzfInflateIn), C.POINTER(abi.PloBgzfInflateOut)]
    L.plo_window_cut_dev.restype = C.c_int
    L.plo_window_cut_dev.argtypes = [vp, C.POINTER(abi.PloWindowCutIn), C.POINTER(abi.PloWindowCutOut)]
    L.plo_bgzf_inflate_part_dev.restype = C.c_int
    L.plo_bgzf_inflate_part_dev.argtypes = [vp, C.POINTER(abi.PloBgzfInflatePartIn), C.POINTER(abi.PloBgzfInflatePartOut)]
    L.plo_window_cut_part_dev.restype = C.c_int
    L.plo_window_cut_part_dev.argtypes = [vp, C.POINTER(abi.PloWindowCutPartIn), C.POINTER(abi.PloWindowCutOut)]
    L.plo_part_start_dev.restype = C.c_int
    L.plo_part_start_dev.argtypes = [vp, C.POINTER(abi.PloPartStartIn), C.POINTER(abi.PloPartStartOut)]
    L.plo_internal_window_cut_seg.restype = C.c_int
    L.plo_internal_window_cut_seg.argtypes = [vp, C.POINTER(abi.PloWindowCutIn), C.POINTER(abi.PloWindowCutOut), C.c_uint64]
    L.plo_batch_build_dev.restype = C.c_int
    L.plo_batch_build_dev.argtypes = [vp, C.POINTER(abi.PloBatchBuildIn), C.POINTER(abi.PloBatchBuildOut)]
    L.plo_bgzf_compress_dev.restype = C.c_int
    L.plo_bgzf_compress_dev.argtypes = [vp, vp, C.c_uint64, C.c_int, C.POINTER(abi.PloBgzfOut)]
    L.plo_ctx_sync.restype = C.c_int
    L.plo_ctx_sync.argtypes = [vp]
    L.plo_ctx_download.restype = C.c_int
    L.plo_ctx_download.argtypes = [vp, vp, vp, C.c_size_t]
    L.plo_gather_unique_id.restype = C.c_int
    L.plo_gather_unique_id.argtypes = [C.POINTER(C.c_uint8)]
    L.plo_gather_create.restype = C.c_int
    L.plo_gather_create.argtypes = [C.POINTER(C.c_uint8), C.c_int, C.c_int, C.c_int, C.POINTER(vp)]
    L.plo_gather_destroy.restype = None
    L.plo_gather_destroy.argtypes = [vp]
    L.plo_gather_records.restype = C.c_int
    L.plo_gather_records.argtypes = [vp, vp, C.POINTER(abi.PloBatchOut), C.c_int, C.POINTER(abi.PloBatchOut)]
    L.plo_gather_wait.restype = C.c_int
    L.plo_gather_wait.argtypes = [vp]
    L.plo_gather_last_error.restype = C.c_char_p
    L.plo_gather_last_error.argtypes = [vp]
    L.plo_ctx_stream.restype = vp
    L.plo_ctx_stream.argtypes = [vp]
    L.plo_ctx_device.restype = C.c_int
    L.plo_ctx_device.argtypes = [vp]
    L.plo_ctx_set_stats.restype = C.c_int
    L.plo_ctx_set_stats.argtypes = [vp, C.c_int]
    L.plo_ctx_set_phase_events.restype = C.c_int
    L.plo_ctx_set_phase_events.argtypes = [vp, C.c_int]
    L.plo_api_version.restype = C.c_uint32
    L.plo_ctx_timing.restype = C.c_int
    L.plo_ctx_timing.argtypes = [vp, C.POINTER(abi.PloTiming)]
    L.plo_last_error.restype = C.c_char_p
    L.plo_last_error.argtypes = [vp]
    L.plo_version.restype = C.c_char_p
    L.plo_version.argtypes = []
    _lib = L
    return L


class Index:
    """Device-resident contig->reference index (plo_index).  Immutable; shareable between engines."""

    def __init__(self, data: abi.IndexData, device: int = 0):
        self.lib = load_library()
        self.data = data
        self._desc = data.to_desc()
        h = C.c_void_p()
        st = self.lib.plo_index_create(C.byref(self._desc), device, C.byref(h))
        if st != abi.PLO_OK:
            raise PortelloError(st, "plo_index_create failed" + (" (no usable HIP device)" if st == abi.PLO_ERR_NO_DEVICE else ""))
        self.handle = h
        self.device = device

    def segment_map(self, global_seg: int) -> Tuple[np.ndarray, np.ndarray]:
        n = C.c_uint32(0)
        self.lib.plo_index_segment_map(self.handle, global_seg, 0, None, None, C.byref(n))
        keys = np.zeros(max(1, n.value), dtype=np.int64)
        vals = np.zeros(max(1, n.value), dtype=np.int64)
        st = self.lib.plo_index_segment_map(self.handle, global_seg, n.value, keys.ctypes.data_as(C.POINTER(C.c_int64)),
                                            vals.ctypes.data_as(C.POINTER(C.c_int64)), C.byref(n))
        if st != abi.PLO_OK:
            raise PortelloError(st, "plo_index_segment_map")
        return keys[: n.value], vals[: n.value]

    def close(self):
        if getattr(self, "handle", None):
            self.lib.plo_index_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Engine:
    """One worker context (plo_ctx): the per-thread home the reference gives BamReaderWorkerThreadData
    (src/worker_thread_data.rs:8-18)."""

    def __init__(self, index: Index, stream: Optional[int] = None):
        """stream: a hipStream_t handle to run on, or None / 0 for a private (non-blocking) stream of the context.  torch's
        *default* stream is the NULL handle, i.e. 0: a context created with `torch.cuda.current_stream().cuda_stream` while the
        default stream is current gets a private stream and is NOT ordered behind torch work -- synchronise before handing it
        tensors torch has just written (devbatch.run_and_download does), or run under a `torch.cuda.Stream` of your own."""
        self.lib = index.lib
        self.index = index
        h = C.c_void_p()
        st = self.lib.plo_ctx_create(index.handle, C.c_void_p(stream) if stream else None, C.byref(h))
        if st != abi.PLO_OK:
            raise PortelloError(st, "plo_ctx_create failed")
        self.handle = h

    def set_stats(self, on: bool = True):
        """plo_ctx_set_stats: the light-item kernel counts timing().algo_bytes / lane_utilisation from the next call on (its production
        instantiation is compiled without the counters)"""
        self._check(self.lib.plo_ctx_set_stats(self.handle, 1 if on else 0), "plo_ctx_set_stats")
        return self

    def set_phase_events(self, on: bool = True):
        """plo_ctx_set_phase_events: off = the one-round-trip calls record no HIP events between their phases (two ~6 us bubbles fewer per
        call on the stream); timing() then carries counts but no times for such calls"""
        self._check(self.lib.plo_ctx_set_phase_events(self.handle, 1 if on else 0), "plo_ctx_set_phase_events")
        return self

    def _check(self, st: int, what: str):
        if st != abi.PLO_OK:
            msg = self.lib.plo_last_error(self.handle)
            raise PortelloError(st, f"{what}: {msg.decode() if msg else ''}")

    def liftover_batch(self, batch: abi.BatchData, stages: int = abi.STAGES_ALL) -> abi.BatchResult:
        """Host arrays in, host arrays out (plo_liftover_batch)."""
        b = batch.to_desc()
        out = abi.PloBatchOut()
        self._check(self.lib.plo_liftover_batch(self.handle, C.byref(b), stages, C.byref(out)), "plo_liftover_batch")
        return abi.result_from_out(out)

    def liftover_batch_host(self, desc: abi.PloBatchIn, stages: int = abi.STAGES_ALL) -> abi.PloBatchOut:
        """plo_liftover_batch on a descriptor of host arrays (e.g. a BAM window's batch); the returned arrays are pinned host
        memory owned by the context, valid until its next call."""
        out = abi.PloBatchOut()
        self._check(self.lib.plo_liftover_batch(self.handle, C.byref(desc), stages, C.byref(out)), "plo_liftover_batch")
        return out

    def liftover_batch_dev(self, desc: abi.PloBatchIn, stages: int = abi.STAGES_ALL) -> abi.PloBatchOut:
        """Device pointers in, device pointers out (plo_liftover_batch_dev); asynchronous on the engine's stream."""
        out = abi.PloBatchOut()
        self._check(self.lib.plo_liftover_batch_dev(self.handle, C.byref(desc), stages, C.byref(out)), "plo_liftover_batch_dev")
        return out

    def finish_batch_dev(self, desc: abi.PloBatchIn, fin: abi.PloFinishIn) -> abi.PloFinishOut:
        """Record finishing for the last liftover_batch_dev result (plo_finish_batch_dev); device pointers."""
        out = abi.PloFinishOut()
        self._check(self.lib.plo_finish_batch_dev(self.handle, C.byref(desc), C.byref(fin), C.byref(out)), "plo_finish_batch_dev")
        return out

    def compact_output_dev(self, out: abi.PloBatchOut) -> abi.PloBatchOut:
        """Pack the output CIGARs of the last liftover_batch_dev result densely (plo_compact_output_dev); updates `out`."""
        self._check(self.lib.plo_compact_output_dev(self.handle, C.byref(out)), "plo_compact_output_dev")
        return out

    def sa_segments_dev(self, sa_in: abi.PloSaIn) -> abi.PloSaOut:
        """SA-tag segments of the last liftover + finish result (plo_sa_segments_dev); device pointers."""
        out = abi.PloSaOut()
        self._check(self.lib.plo_sa_segments_dev(self.handle, C.byref(sa_in), C.byref(out)), "plo_sa_segments_dev")
        return out

    def nm_dev(self, desc: abi.PloBatchIn) -> abi.PloNmOut:
        """NM:i of every lifted item of the batch this context has just lifted, compacted and finished (plo_nm_dev): calmd's edit distance of
        the output record against the index's chromosomes; device pointers out.  While the result stands (until the next lift call),
        records_build_dev writes NM:i into every lifted record.  A CIGAR that leaves its chromosome or its read raises PortelloError with
        status PLO_ERR_RANGE and the lowest such item in `err_item`."""
        out = abi.PloNmOut()
        st = self.lib.plo_nm_dev(self.handle, C.byref(desc), C.byref(out))
        if st != abi.PLO_OK:
            msg = self.lib.plo_last_error(self.handle)
            e = PortelloError(st, f"plo_nm_dev: {msg.decode() if msg else ''}")
            e.err_item = int(out.err_item)
            raise e
        return out

    def md_dev(self, desc: abi.PloBatchIn) -> abi.PloMdOut:
        """MD:Z of every lifted item of the batch this context has just lifted, compacted and finished (plo_md_dev): calmd's text of the
        output record against the index's chromosomes, the items' values side by side with their offsets; device pointers out.  While the
        result stands (until the next lift call), records_build_dev writes MD:Z into every lifted record and cuts the source's MD.
        Independent of nm_dev.  A CIGAR that leaves its chromosome or its read raises PortelloError with status PLO_ERR_RANGE and the
        lowest such item in `err_item`."""
        out = abi.PloMdOut()
        st = self.lib.plo_md_dev(self.handle, C.byref(desc), C.byref(out))
        if st != abi.PLO_OK:
            msg = self.lib.plo_last_error(self.handle)
            e = PortelloError(st, f"plo_md_dev: {msg.decode() if msg else ''}")
            e.err_item = int(out.err_item)
            raise e
        return out

    def eqx_dev(self, desc: abi.PloBatchIn) -> abi.PloEqxOut:
        """The = / X CIGAR of every lifted item of the batch this context has just lifted, compacted and finished (plo_eqx_dev): every M, =
        or X op of the output CIGAR replaced by its maximal runs of matching (=) and mismatching (X) pairs against the index's chromosomes,
        every other op as it stands; the items' ops side by side with their offsets, device pointers out.  While the result stands (until
        the next lift call), records_build_dev writes these CIGARs in place of the lift's.  Independent of nm_dev and md_dev.  A CIGAR that
        leaves its chromosome or its read raises PortelloError with status PLO_ERR_RANGE and the lowest such item in `err_item`."""
        out = abi.PloEqxOut()
        st = self.lib.plo_eqx_dev(self.handle, C.byref(desc), C.byref(out))
        if st != abi.PLO_OK:
            msg = self.lib.plo_last_error(self.handle)
            e = PortelloError(st, f"plo_eqx_dev: {msg.decode() if msg else ''}")
            e.err_item = int(out.err_item)
            raise e
        return out

    def records_build_dev(self, desc: abi.PloBatchIn, rin: abi.PloRecordsIn) -> abi.PloRecordsOut:
        """The window's output BAM records assembled on the device from the last liftover + finish + SA results
        (plo_records_build_dev); device pointers in and out."""
        out = abi.PloRecordsOut()
        self._check(self.lib.plo_records_build_dev(self.handle, C.byref(desc), C.byref(rin), C.byref(out)), "plo_records_build_dev")
        return out

    def records_sort_dev(self, bytes_ptr, n_bytes: int, n_records: int, record_off_ptr, n_ref: int) -> abi.PloSortOut:
        """The records at the DEVICE address `bytes_ptr` (plo_records_out::bytes / record_off, or any such buffer) copied in coordinate
        order into a buffer of the context's own (plo_records_sort_dev): by (reference in header order, position, forward before reverse;
        refID -1 last), ties in input order.  Device pointers out, valid until the engine's next records_sort_dev; the input stays
        unchanged.  A record the device check refuses raises PortelloError with status PLO_ERR_INVALID_ARG and the lowest such record in
        `err_record`."""
        sin = abi.PloSortIn(C.cast(bytes_ptr, abi._u8p), int(n_bytes), int(n_records), C.cast(record_off_ptr, abi._u64p), int(n_ref))
        out = abi.PloSortOut()
        st = self.lib.plo_records_sort_dev(self.handle, C.byref(sin), C.byref(out))
        if st != abi.PLO_OK:
            msg = self.lib.plo_last_error(self.handle)
            e = PortelloError(st, f"plo_records_sort_dev: {msg.decode() if msg else ''}")
            e.err_record = int(out.err_record)
            raise e
        return out

    def records_index_dev(self, bytes_ptr, n_bytes: int, n_records: int, record_off_ptr, n_ref: int) -> abi.PloIndexOut:
        """What a BAM index needs of every record of the coordinate-sorted buffer at the DEVICE address `bytes_ptr` (records_sort_dev's
        bytes / record_off): plo_records_index_dev, a plo_index_entry of 24 bytes a record, on the device, valid until the engine's next
        records_index_dev; the input stays unchanged.  A record the device check refuses (what records_sort_dev refuses, a CIGAR that
        leaves its record, an end behind 2^29, a record in front of the one before it) raises PortelloError with status
        PLO_ERR_INVALID_ARG, the lowest such record in `err_record` and what it broke in `err_kind`."""
        iin = abi.PloIndexIn(C.cast(bytes_ptr, abi._u8p), int(n_bytes), int(n_records), C.cast(record_off_ptr, abi._u64p), int(n_ref))
        out = abi.PloIndexOut()
        st = self.lib.plo_records_index_dev(self.handle, C.byref(iin), C.byref(out))
        if st != abi.PLO_OK:
            msg = self.lib.plo_last_error(self.handle)
            e = PortelloError(st, f"plo_records_index_dev: {msg.decode() if msg else ''}")
            e.err_record, e.err_kind = int(out.err_record), int(out.err_kind)
            raise e
        return out

    def runs_merge_plan_dev(self, runs, n_ref: int, chunk_bytes: int) -> abi.PloMergeOut:
        """The merged order of coordinate-sorted record buffers that each lie in a DEVICE allocation of their own (plo_runs_merge_plan_dev).
        runs: a sequence of (bytes_ptr, n_bytes, n_records, record_off_ptr), record_off counted from the run's own bytes; a run without
        records may carry 0 for both pointers.  The order is records_sort_dev's over the runs' concatenation: by (key, run, place in the
        run).  Out: device src / key / record_off of the merged stream and the chunk table as HOST arrays (chunk c holds the merged
        records [chunk_first[c], chunk_first[c + 1]): as many as keep its bytes <= chunk_bytes, never fewer than one), all valid until the
        engine's next runs_merge_plan_dev.  No record byte is moved: runs_merge_emit_dev copies a chunk, and the runs must stay valid and
        unchanged until the last emit.  A record the device check refuses raises PortelloError with status PLO_ERR_INVALID_ARG and
        `err_run`, `err_record` (its place in that run) and `err_kind` (1 .. 5 as records_sort_dev, 6: a key below the one before it)."""
        runs = list(runs)
        arr = (abi.PloMergeRun * max(1, len(runs)))()
        for k, (b, nb, n, off) in enumerate(runs):
            arr[k] = abi.PloMergeRun(C.cast(b, abi._u8p), int(nb), int(n), C.cast(off, abi._u64p))
        min_ = abi.PloMergeIn(arr, len(runs), int(n_ref), int(chunk_bytes))
        out = abi.PloMergeOut()
        st = self.lib.plo_runs_merge_plan_dev(self.handle, C.byref(min_), C.byref(out))
        if st != abi.PLO_OK:
            msg = self.lib.plo_last_error(self.handle)
            e = PortelloError(st, f"plo_runs_merge_plan_dev: {msg.decode() if msg else ''}")
            e.err_run, e.err_record, e.err_kind = int(out.err_run), int(out.err_record), int(out.err_kind)
            raise e
        return out

    def runs_merge_emit_dev(self, chunk: int) -> abi.PloMergeChunkOut:
        """Chunk `chunk` of the engine's current plan copied, in merged order, into a buffer of the context's own (plo_runs_merge_emit_dev):
        device bytes and record_off rebased to the chunk -- what records_index_dev and bgzf_compress_dev take --, valid until the engine's
        next runs_merge_emit_dev.  PLO_ERR_INVALID_ARG without a plan or for chunk >= n_chunks."""
        out = abi.PloMergeChunkOut()
        self._check(self.lib.plo_runs_merge_emit_dev(self.handle, int(chunk), C.byref(out)), "plo_runs_merge_emit_dev")
        return out

    def batch_build_dev(self, bin_: abi.PloBatchBuildIn) -> abi.PloBatchBuildOut:
        """The window's plo_batch_in / plo_finish_in built on the device from its uploaded records (plo_batch_build_dev); device pointers in
        and out, the arrays valid until the engine's next batch_build_dev.  A PLO_ERR_DATA failure carries `err_read` (the lowest failing
        read) and `err_kind` (abi.BB_ERR_*) on the exception."""
        out = abi.PloBatchBuildOut()
        st = self.lib.plo_batch_build_dev(self.handle, C.byref(bin_), C.byref(out))
        if st != abi.PLO_OK:
            msg = self.lib.plo_last_error(self.handle)
            e = PortelloError(st, f"plo_batch_build_dev: {msg.decode() if msg else ''}")
            e.err_read, e.err_kind = int(out.err_read), int(out.err_kind)
            raise e
        return out

    def bgzf_inflate_dev(self, bgzf, bgzf_bytes: int, dst, dst_cap: int) -> abi.PloBgzfInflateOut:
        """The whole BGZF blocks at the HOST address `bgzf` inflated and CRC-checked on the device, their bytes left packed at the DEVICE
        address `dst` (plo_bgzf_inflate_dev); blocks that no longer fit into dst_cap and a trailing partial block are not consumed."""
        out = abi.PloBgzfInflateOut()
        bin_ = abi.PloBgzfInflateIn(C.cast(C.c_void_p(int(bgzf)), abi._u8p), int(bgzf_bytes), C.cast(C.c_void_p(int(dst)), abi._u8p), int(dst_cap))
        self._check(self.lib.plo_bgzf_inflate_dev(self.handle, C.byref(bin_), C.byref(out)), "plo_bgzf_inflate_dev")
        return out

    def window_cut_dev(self, stream, stream_bytes: int, max_records: int, final: bool, max_unmapped: int = 0, max_bytes: int = 0,
                       seg_bytes: int = 0) -> abi.PloWindowCutOut:
        """The window plo_bam_read_window would cut from the inflated BAM stream at the DEVICE address `stream` (plo_window_cut_dev); device
        pointers out, valid until the engine's next window_cut_dev.  A refused record raises with `err_off` on the exception.  seg_bytes:
        tests only, segments of another size than abi.CUT_SEG_BYTES."""
        out = abi.PloWindowCutOut()
        cin = abi.PloWindowCutIn(C.cast(C.c_void_p(int(stream)), abi._u8p), int(stream_bytes), int(max_records), int(max_unmapped), int(max_bytes), 1 if final else 0)
        if seg_bytes:
            st = self.lib.plo_internal_window_cut_seg(self.handle, C.byref(cin), C.byref(out), int(seg_bytes))
        else:
            st = self.lib.plo_window_cut_dev(self.handle, C.byref(cin), C.byref(out))
        if st != abi.PLO_OK:
            msg = self.lib.plo_last_error(self.handle)
            e = PortelloError(st, f"plo_window_cut_dev: {msg.decode() if msg else ''}")
            e.err_off = int(out.err_off)
            raise e
        return out

    def bgzf_inflate_part_dev(self, bgzf, bgzf_bytes: int, dst, dst_cap: int, bgzf_file_off: int, range_end: int = abi.NO_RANGE_END) -> abi.PloBgzfInflatePartOut:
        """bgzf_inflate_dev for a part of a file (plo_bgzf_inflate_part_dev): `bgzf` lies at bgzf_file_off of the file and the part ends at
        range_end; own_bytes of the result is where, inside dst, the first block of the next part's stretch starts (n_bytes: nowhere)."""
        out = abi.PloBgzfInflatePartOut()
        bin_ = abi.PloBgzfInflatePartIn(C.cast(C.c_void_p(int(bgzf)), abi._u8p), int(bgzf_bytes), C.cast(C.c_void_p(int(dst)), abi._u8p), int(dst_cap),
                                        int(bgzf_file_off), int(range_end))
        self._check(self.lib.plo_bgzf_inflate_part_dev(self.handle, C.byref(bin_), C.byref(out)), "plo_bgzf_inflate_part_dev")
        return out

    def window_cut_part_dev(self, stream, stream_bytes: int, max_records: int, final: bool, own_bytes: int, max_unmapped: int = 0,
                            max_bytes: int = 0) -> abi.PloWindowCutOut:
        """window_cut_dev with the host's range test (plo_window_cut_part_dev): a record at or behind own_bytes ends the window in front of it
        with abi.CUT_PART_END, whatever stands there."""
        out = abi.PloWindowCutOut()
        cin = abi.PloWindowCutPartIn(C.cast(C.c_void_p(int(stream)), abi._u8p), int(stream_bytes), int(max_records), int(max_unmapped), int(max_bytes),
                                     1 if final else 0, int(own_bytes))
        st = self.lib.plo_window_cut_part_dev(self.handle, C.byref(cin), C.byref(out))
        if st != abi.PLO_OK:
            msg = self.lib.plo_last_error(self.handle)
            e = PortelloError(st, f"plo_window_cut_part_dev: {msg.decode() if msg else ''}")
            e.err_off = int(out.err_off)
            raise e
        return out

    def part_start_dev(self, stream, stream_bytes: int, n_ref: int, final: bool) -> abi.PloPartStartOut:
        """Where the first record of a part starts in the inflated bytes at the DEVICE address `stream`, which begin with the part's first
        BGZF block (plo_part_start_dev): kind abi.PART_FOUND with first_off, PART_NEED_MORE (ask again with more bytes) or PART_NONE."""
        out = abi.PloPartStartOut()
        pin = abi.PloPartStartIn(C.cast(C.c_void_p(int(stream)), abi._u8p), int(stream_bytes), int(n_ref), 1 if final else 0)
        self._check(self.lib.plo_part_start_dev(self.handle, C.byref(pin), C.byref(out)), "plo_part_start_dev")
        return out

    def bgzf_compress_dev(self, dev_bytes, n_bytes: int, level: int) -> abi.PloBgzfOut:
        """`n_bytes` at the device pointer `dev_bytes` (typically a plo_records_out's bytes) as finished BGZF blocks of 0xff00-byte payloads
        (plo_bgzf_compress_dev): level 0 stored, level 1 the device's deflate.  Device pointers out; the preceding records_build_dev
        output stays valid."""
        out = abi.PloBgzfOut()
        addr = dev_bytes if isinstance(dev_bytes, int) or dev_bytes is None else C.cast(dev_bytes, C.c_void_p).value
        self._check(self.lib.plo_bgzf_compress_dev(self.handle, C.c_void_p(addr), int(n_bytes), int(level), C.byref(out)), "plo_bgzf_compress_dev")
        return out

    def download(self, dev_ptr, dtype, count: int) -> np.ndarray:
        """copy `count` elements of `dtype` from a device pointer (e.g. a plo_batch_out array) to a numpy array"""
        out = np.zeros(max(1, count), dtype=dtype)
        addr = C.cast(dev_ptr, C.c_void_p).value if not isinstance(dev_ptr, int) else dev_ptr
        if count:
            self._check(self.lib.plo_ctx_download(self.handle, out.ctypes.data_as(C.c_void_p), C.c_void_p(addr),
                                                  count * out.itemsize), "plo_ctx_download")
        return out[:count]

    def sync(self):
        self._check(self.lib.plo_ctx_sync(self.handle), "plo_ctx_sync")

    def timing(self) -> abi.PloTiming:
        t = abi.PloTiming()
        t.struct_size = C.sizeof(abi.PloTiming)
        self._check(self.lib.plo_ctx_timing(self.handle, C.byref(t)), "plo_ctx_timing")
        return t

    def close(self):
        if getattr(self, "handle", None):
            self.lib.plo_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def hip_backend(device: int = 0) -> Backend:
    """Backend that builds a throw-away index + engine per call (unit-level calls and tests)."""

    def run(index: abi.IndexData, batch: abi.BatchData, stages: int) -> abi.BatchResult:
        ix = Index(index, device)
        try:
            eng = Engine(ix)
            try:
                return eng.liftover_batch(batch, stages)
            finally:
                eng.close()
        finally:
            ix.close()

    return run


# ----------------------------------------------------------------------------------------------------------------
# one-item cases: the reference's function signatures expressed as batch inputs
# ----------------------------------------------------------------------------------------------------------------

class CaseSet:
    """Accumulates independent single-call cases into one batch (one contig + one read per case)."""

    def __init__(self):
        self.contig_len: List[int] = []
        self.seg_chrom: List[int] = []
        self.seg_pos: List[int] = []
        self.seg_cigar: List[np.ndarray] = []
        self.chrom_seq: List[np.ndarray] = []
        self.rev_seq: List[Optional[np.ndarray]] = []
        self.read_seq: List[np.ndarray] = []
        self.read_pos: List[int] = []
        self.read_cigar: List[np.ndarray] = []

    def _add(self, map_pos, map_cigar, chrom_seq, rev_seq, contig_len, read_pos, read_cigar, read_seq):
        self.contig_len.append(int(contig_len))
        self.seg_chrom.append(len(self.chrom_seq))
        self.seg_pos.append(int(map_pos))
        self.seg_cigar.append(np.asarray(map_cigar, dtype=np.uint32))
        self.chrom_seq.append(np.frombuffer(bytes(chrom_seq), dtype=np.uint8))
        self.rev_seq.append(None if rev_seq is None else np.frombuffer(bytes(rev_seq), dtype=np.uint8))
        self.read_pos.append(int(read_pos))
        self.read_cigar.append(np.asarray(read_cigar, dtype=np.uint32))
        self.read_seq.append(np.frombuffer(bytes(read_seq), dtype=np.uint8))
        return len(self.contig_len) - 1

    def add_liftover(self, map_pos: int, map_cigar, start: int, cigar) -> int:
        cigar = np.asarray(cigar, dtype=np.uint32)
        n = cg.read_len(cigar)
        return self._add(map_pos, map_cigar, b"N", None, 1 << 30, start, cigar, b"N" * n)

    def add_simplify(self, ref_pos: int, cigar, ref_seq: bytes, read_seq: bytes) -> int:
        return self._add(0, np.zeros(0, np.uint32), ref_seq, None, 1 << 30, ref_pos, cigar, read_seq)

    def add_left_shift(self, ref_pos: int, cigar, ref_seq: bytes, read_seq: bytes) -> int:
        return self._add(0, np.zeros(0, np.uint32), b"N", ref_seq, len(ref_seq), ref_pos, cigar, read_seq)

    def build(self) -> Tuple[abi.IndexData, abi.BatchData]:
        n = len(self.contig_len)
        seg_cigar_off = np.zeros(n + 1, dtype=np.uint32)
        seg_cigar_off[1:] = np.cumsum([len(c) for c in self.seg_cigar])
        index = abi.IndexData(
            contig_len=np.array(self.contig_len, dtype=np.int64), contig_seg_off=np.arange(n + 1, dtype=np.uint32),
            seg_chrom_index=np.array(self.seg_chrom, dtype=np.uint32), seg_pos=np.array(self.seg_pos, dtype=np.int64),
            seg_is_fwd_strand=np.ones(n, dtype=np.uint8), seg_mapq=np.full(n, 60, dtype=np.uint8),
            seg_seq_order_start=np.zeros(n, dtype=np.int64), seg_seq_order_end=np.array(self.contig_len, dtype=np.int64),
            seg_cigar_off=seg_cigar_off,
            seg_cigar=np.concatenate(self.seg_cigar) if n else np.zeros(0, np.uint32),
            chrom_seq=self.chrom_seq, rev_contig_seq=self.rev_seq)
        seq_len = np.array([len(s) for s in self.read_seq], dtype=np.uint32)
        seq_off = np.zeros(n, dtype=np.uint64)
        if n:
            seq_off[1:] = np.cumsum(seq_len[:-1])
        rc_off = np.zeros(n + 1, dtype=np.uint32)
        rc_off[1:] = np.cumsum([len(c) for c in self.read_cigar])
        batch = abi.BatchData(
            read_is_reverse=np.zeros(n, dtype=np.uint8), read_seq_len=seq_len, read_seq_off=seq_off,
            seq=np.concatenate(self.read_seq) if n else np.zeros(0, np.uint8), seq_fmt=abi.SEQ_ASCII,
            seg_read=np.arange(n, dtype=np.uint32), seg_contig=np.arange(n, dtype=np.uint32),
            seg_pos=np.array(self.read_pos, dtype=np.int64), seg_is_fwd_strand=np.ones(n, dtype=np.uint8),
            seg_cigar_off=rc_off, cigar=np.concatenate(self.read_cigar) if n else np.zeros(0, np.uint32),
            item_seg=np.arange(n, dtype=np.uint32), item_cseg=np.zeros(n, dtype=np.uint32))
        return index, batch

    def run(self, stages: int, backend: Optional[Backend] = None):
        """-> list of None | (pos, cigar) per case, in insertion order"""
        backend = backend or hip_backend()
        index, batch = self.build()
        res = backend(index, batch, stages)
        assert res.n_items == len(self.contig_len)
        out = [None] * res.n_items
        for i in range(res.n_items):
            k = int(res.item_seg[i])
            st = int(res.item_status[i])
            if st == abi.ITEM_LIFTED:
                out[k] = (int(res.item_ref_pos[i]), res.item_cigar(i).copy())
            elif st == abi.ITEM_NO_LIFTOVER:
                out[k] = None
            else:
                raise PortelloError(abi.PLO_ERR_INTERNAL, f"case {k}: item status {st} (the reference would panic)")
        return out


def liftover_read_alignment(ref1_to_ref2_map: Tuple[int, Sequence[int]], ref1_cigar_segment_start_pos: int,
                            ref1_cigar: Sequence[int], backend: Optional[Backend] = None):
    """liftover_read_alignment(&ReadToRefTreeMap, i64, &[Cigar]) -> Option<(i64, Vec<Cigar>)>
    (src/liftover_read_alignment.rs:137-141).  The map is given by what it is built from: ``(ref_pos, cigar)`` of
    the contig segment alignment, i.e. the arguments of get_read_segment_to_ref_pos_tree_map."""
    cs = CaseSet()
    cs.add_liftover(ref1_to_ref2_map[0], ref1_to_ref2_map[1], ref1_cigar_segment_start_pos, ref1_cigar)
    return cs.run(abi.STAGE_LIFTOVER, backend)[0]


def simplify_alignment_indels(ref_pos: int, cigar: Sequence[int], ref_seq: bytes, read_seq: bytes,
                              backend: Optional[Backend] = None):
    """simplify_alignment_indels(i64, &[Cigar], &[u8], &[u8]) -> (i64, Vec<Cigar>) (src/simplify_alignment_indels.rs:119-124)"""
    cs = CaseSet()
    cs.add_simplify(ref_pos, cigar, ref_seq, read_seq)
    return cs.run(abi.STAGE_SIMPLIFY, backend)[0]


def left_shift_indels(ref_pos: int, cigar: Sequence[int], ref_seq: bytes, read_seq: bytes, backend: Optional[Backend] = None):
    """left_shift_indels(i64, &[Cigar], &[u8], &[u8]) -> (i64, Vec<Cigar>)
    (lib/rust-vc-utils/src/bam_utils/cigar/shift_indels/left_shift_indels.rs:17-22)"""
    cs = CaseSet()
    cs.add_left_shift(ref_pos, cigar, ref_seq, read_seq)
    return cs.run(abi.STAGE_LSHIFT, backend)[0]


def assemble_sa_values(seg_off: np.ndarray, text: np.ndarray, item_read: np.ndarray) -> list:
    """SA:Z value of every item from the per-item segments (src/read_alignment_scanner.rs:352-364): the segments of the
    read's other items, in item order; None where the record gets no SA tag.  Items of a read are consecutive."""
    n = len(item_read)
    t = text.tobytes()
    segs = [t[int(seg_off[i]):int(seg_off[i + 1])] for i in range(n)]
    out = [None] * n
    i0 = 0
    while i0 < n:
        i1 = i0
        while i1 < n and item_read[i1] == item_read[i0]:
            i1 += 1
        for i in range(i0, i1):
            if segs[i]:
                v = b"".join(segs[j] for j in range(i0, i1) if j != i)
                out[i] = v if v else None
        i0 = i1
    return out


class PinnedArray:
    """numpy view of page-locked host memory from plo_host_alloc (released on close / garbage collection)"""

    def __init__(self, like: np.ndarray):
        like = np.ascontiguousarray(like)
        self.lib = load_library()
        self.ptr = C.c_void_p()
        rc = self.lib.plo_host_alloc(max(16, like.nbytes), C.byref(self.ptr))
        if rc != abi.PLO_OK:
            raise PortelloError(rc, "plo_host_alloc failed")
        buf = (C.c_uint8 * max(16, like.nbytes)).from_address(self.ptr.value)
        self.array = np.frombuffer(buf, dtype=like.dtype, count=like.size).reshape(like.shape)
        self.array[...] = like

    def close(self):
        if getattr(self, "ptr", None) is not None and self.ptr.value:
            self.array = None
            self.lib.plo_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
