"""Device-resident batches: builds a ``plo_batch_in`` whose arrays are torch tensors already in HBM (the form the
bench times: inputs resident on the GPU when the timed region starts), and downloads ``plo_batch_out`` arrays."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import abi


def _p(t: torch.Tensor, ctype):
    return C.cast(C.c_void_p(t.data_ptr()), C.POINTER(ctype))


@dataclass
class DeviceBatch:
    read_is_reverse: torch.Tensor  # uint8
    read_seq_len: torch.Tensor     # int32 (bit pattern of uint32)
    read_seq_off: torch.Tensor     # int64 (bit pattern of uint64)
    seq: torch.Tensor              # uint8
    seq_fmt: int
    seg_read: torch.Tensor         # int32
    seg_contig: torch.Tensor       # int32
    seg_pos: torch.Tensor          # int64
    seg_is_fwd_strand: torch.Tensor  # uint8
    seg_cigar_off: torch.Tensor    # int32 [n_segs+1]
    cigar: torch.Tensor            # int32 (bit pattern of uint32)

    @property
    def n_reads(self) -> int:
        return int(self.read_seq_len.numel())

    @property
    def n_segs(self) -> int:
        return int(self.seg_read.numel())

    @classmethod
    def from_workload(cls, w, read_lo: int = 0, read_hi: Optional[int] = None) -> "DeviceBatch":
        """Slice reads [read_lo, read_hi) of a synth.Workload living on the GPU (offsets re-based)."""
        dev = w.device
        assert dev.type == "cuda"
        hi = w.n_reads if read_hi is None else read_hi
        lo = read_lo
        seg_lo = int(torch.searchsorted(w.seg_read, torch.tensor(lo, device=dev)).item())
        seg_hi = int(torch.searchsorted(w.seg_read, torch.tensor(hi, device=dev)).item())
        co = w.seg_cigar_off_r[seg_lo: seg_hi + 1]
        c0 = int(co[0].item()) if co.numel() else 0
        c1 = int(co[-1].item()) if co.numel() else 0
        so = w.read_seq_off[lo:hi]
        sl = w.read_seq_len[lo:hi]
        if hi > lo:
            b0 = int(so[0].item())
            last = int(sl[-1].item())
            b1 = int(so[-1].item()) + ((last + 1) // 2 if w.cfg.seq_fmt == abi.SEQ_BAM4 else last)
        else:
            b0 = b1 = 0
        return cls(
            read_is_reverse=w.read_is_reverse[lo:hi].contiguous(), read_seq_len=sl.to(torch.int32).contiguous(),
            read_seq_off=(so - b0).to(torch.int64).contiguous(), seq=w.seq[b0:b1].contiguous(), seq_fmt=w.cfg.seq_fmt,
            seg_read=(w.seg_read[seg_lo:seg_hi] - lo).to(torch.int32).contiguous(),
            seg_contig=w.seg_contig[seg_lo:seg_hi].to(torch.int32).contiguous(),
            seg_pos=w.seg_pos_r[seg_lo:seg_hi].to(torch.int64).contiguous(),
            seg_is_fwd_strand=w.seg_is_fwd_r[seg_lo:seg_hi].contiguous(),
            seg_cigar_off=(co - c0).to(torch.int32).contiguous(), cigar=w.cigar[c0:c1].to(torch.int32).contiguous())

    @classmethod
    def from_batch_data(cls, b: abi.BatchData, device="cuda") -> "DeviceBatch":
        """upload of a host-side batch (numpy arrays) as it is"""
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt) if a.dtype.itemsize == np.dtype(dt).itemsize else
                                           np.ascontiguousarray(a).astype(dt)).to(device)
        return cls(read_is_reverse=t(b.read_is_reverse, np.uint8), read_seq_len=t(b.read_seq_len, np.int32), read_seq_off=t(b.read_seq_off, np.int64),
                   seq=t(b.seq if len(b.seq) else np.zeros(1, np.uint8), np.uint8), seq_fmt=b.seq_fmt, seg_read=t(b.seg_read, np.int32),
                   seg_contig=t(b.seg_contig, np.int32), seg_pos=t(b.seg_pos, np.int64), seg_is_fwd_strand=t(b.seg_is_fwd_strand, np.uint8),
                   seg_cigar_off=t(b.seg_cigar_off, np.int32), cigar=t(b.cigar if len(b.cigar) else np.zeros(1, np.uint32), np.int32))

    @classmethod
    def from_read_ranges(cls, w, ranges) -> "DeviceBatch":
        """The reads of several ranges [lo, hi) of a workload as ONE batch (a rank's windows, portello_amd/shard.py):
        the slices are concatenated, offsets re-based.  Read r of range k becomes read (reads of ranges < k) + r - lo."""
        parts = [cls.from_workload(w, lo, hi) for lo, hi in ranges if hi > lo]
        if not parts:
            return cls.from_workload(w, 0, 0)
        if len(parts) == 1:
            return parts[0]
        rb = cb = sb = 0
        seg_read, coff, soff = [], [], []
        for p_ in parts:
            seg_read.append(p_.seg_read + rb)
            coff.append(p_.seg_cigar_off[:-1] + cb)
            soff.append(p_.read_seq_off + sb)
            rb += p_.n_reads
            cb += int(p_.cigar.numel())
            sb += int(p_.seq.numel())
        coff.append(torch.tensor([cb], dtype=torch.int32, device=parts[0].cigar.device))
        cat = lambda name: torch.cat([getattr(p_, name) for p_ in parts]).contiguous()
        return cls(read_is_reverse=cat("read_is_reverse"), read_seq_len=cat("read_seq_len"), read_seq_off=torch.cat(soff).contiguous(),
                   seq=cat("seq"), seq_fmt=parts[0].seq_fmt, seg_read=torch.cat(seg_read).to(torch.int32).contiguous(),
                   seg_contig=cat("seg_contig"), seg_pos=cat("seg_pos"), seg_is_fwd_strand=cat("seg_is_fwd_strand"),
                   seg_cigar_off=torch.cat(coff).to(torch.int32).contiguous(), cigar=cat("cigar"))

    def desc(self) -> abi.PloBatchIn:
        b = abi.PloBatchIn()
        b.n_reads = self.n_reads
        b.read_is_reverse = _p(self.read_is_reverse, C.c_uint8)
        b.read_seq_len = _p(self.read_seq_len, C.c_uint32)
        b.read_seq_off = _p(self.read_seq_off, C.c_uint64)
        b.seq = _p(self.seq, C.c_uint8)
        b.seq_bytes = self.seq.numel()
        b.seq_fmt = self.seq_fmt
        b.n_segs = self.n_segs
        b.seg_read = _p(self.seg_read, C.c_uint32)
        b.seg_contig = _p(self.seg_contig, C.c_uint32)
        b.seg_pos = _p(self.seg_pos, C.c_int64)
        b.seg_is_fwd_strand = _p(self.seg_is_fwd_strand, C.c_uint8)
        b.seg_cigar_off = _p(self.seg_cigar_off, C.c_uint32)
        b.cigar = _p(self.cigar, C.c_uint32)
        b.n_items = 0
        b.item_seg = C.cast(None, C.POINTER(C.c_uint32))
        b.item_cseg = C.cast(None, C.POINTER(C.c_uint32))
        return b


def download(eng, out: abi.PloBatchOut) -> abi.BatchResult:
    n, nc = int(out.n_items), int(out.n_cigar)
    return abi.BatchResult(
        item_seg=eng.download(out.item_seg, np.uint32, n), item_cseg=eng.download(out.item_cseg, np.uint32, n),
        item_status=eng.download(out.item_status, np.uint8, n), item_need_flipped=eng.download(out.item_need_flipped, np.uint8, n),
        item_mapq=eng.download(out.item_mapq, np.uint8, n), item_chrom_index=eng.download(out.item_chrom_index, np.uint32, n),
        item_ref_pos=eng.download(out.item_ref_pos, np.int64, n), item_cigar_off=eng.download(out.item_cigar_off, np.uint64, n),
        item_cigar_len=eng.download(out.item_cigar_len, np.uint32, n), cigar=eng.download(out.cigar, np.uint32, nc))


def run_and_download(eng, db: DeviceBatch, stages: int = abi.STAGES_ALL) -> abi.BatchResult:
    torch.cuda.synchronize()
    out = eng.liftover_batch_dev(db.desc(), stages)
    return download(eng, out)


def finish_inputs(w, db: DeviceBatch, seed: int = 1):
    """Synthetic record flags + base qualities for the record-finishing stage (device tensors + the plo_finish_in)."""
    dev = db.seq.device
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    lens = db.read_seq_len.to(torch.int64)
    qoff = torch.cumsum(lens, 0) - lens
    total = int(lens.sum().item())
    qual = torch.randint(0, 94, (max(1, total),), generator=g, device=dev, dtype=torch.uint8)
    flags = (db.read_is_reverse.to(torch.int16) * 0x10) | (torch.randint(0, 2, (db.n_reads,), generator=g, device=dev).to(torch.int16) * 0x400)
    fin = abi.PloFinishIn(_p(flags, C.c_uint16), _p(qual, C.c_uint8), _p(qoff, C.c_uint64), total)
    return fin, dict(flags=flags, qual=qual, qoff=qoff)


def download_finish(eng, fo: abi.PloFinishOut, n_items: int, n_reads: int) -> dict:
    res = {name: eng.download(getattr(fo, name), dt, n_items) for name, dt in abi.FINISH_ITEM_FIELDS}
    res.update({name: eng.download(getattr(fo, name), dt, n_reads) for name, dt in abi.FINISH_READ_FIELDS})
    res["rev_seq"] = eng.download(fo.rev_seq, np.uint8, int(fo.rev_seq_bytes))
    res["rev_qual"] = eng.download(fo.rev_qual, np.uint8, int(fo.rev_qual_bytes))
    return res


def sa_inputs(names, dev):
    """chromosome labels as device arrays + the plo_sa_in"""
    enc = [n.encode() if isinstance(n, str) else bytes(n) for n in names]
    off = np.zeros(len(enc) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(e) for e in enc])
    blob = np.frombuffer(b"".join(enc) or b"\0", dtype=np.uint8).copy()
    t_off = torch.from_numpy(off).to(dev)
    t_blob = torch.from_numpy(blob).to(dev)
    return abi.PloSaIn(len(enc), _p(t_off, C.c_uint32), _p(t_blob, C.c_uint8)), dict(off=t_off, blob=t_blob)


def download_sa(eng, so: abi.PloSaOut):
    off = eng.download(so.item_sa_off, np.uint32, int(so.n_items) + 1)
    text = eng.download(so.sa_text, np.uint8, int(so.sa_bytes))
    return off, text


# ---- a BAM window's batch on the device, finished there, results back on the host (pipeline.run_bam_to_bam, device_finish) --------

def _host_view(ptr, dtype, count: int) -> np.ndarray:
    if not count:
        return np.zeros(0, dtype)
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(count * np.dtype(dtype).itemsize,)).view(dtype)


@dataclass
class UploadedWindow:
    """device copies of a window's plo_batch_in (dense bases) and plo_finish_in; keeps the tensors alive"""
    batch: DeviceBatch
    flags: torch.Tensor
    qual: torch.Tensor
    qual_off: torch.Tensor
    qual_bytes: int

    def finish_in(self) -> abi.PloFinishIn:
        return abi.PloFinishIn(_p(self.flags, C.c_uint16), _p(self.qual, C.c_uint8), _p(self.qual_off, C.c_uint64), self.qual_bytes)


def upload_window(desc: abi.PloBatchIn, fin: abi.PloFinishIn, dev) -> UploadedWindow:
    """copies the host arrays of a window's batch descriptor (bam.Window.batch_desc(with_finish=True)) to the device, on torch's
    current stream"""
    n, ns = int(desc.n_reads), int(desc.n_segs)

    def up(ptr, dtype, count, as_dtype=None):
        a = _host_view(ptr, dtype, count)
        if as_dtype is not None:
            a = a.view(as_dtype)
        t = torch.from_numpy(a) if count else torch.zeros(0, dtype=torch.from_numpy(np.zeros(1, as_dtype or dtype)).dtype)
        return t.to(dev, non_blocking=True) if count else torch.zeros(1, dtype=t.dtype, device=dev)[:0]

    coff = _host_view(desc.seg_cigar_off, np.uint32, ns + 1)
    n_ops = int(coff[-1]) if ns else 0
    b = DeviceBatch(read_is_reverse=up(desc.read_is_reverse, np.uint8, n), read_seq_len=up(desc.read_seq_len, np.uint32, n, np.int32),
                    read_seq_off=up(desc.read_seq_off, np.uint64, n, np.int64), seq=up(desc.seq, np.uint8, int(desc.seq_bytes)),
                    seq_fmt=int(desc.seq_fmt), seg_read=up(desc.seg_read, np.uint32, ns, np.int32), seg_contig=up(desc.seg_contig, np.uint32, ns, np.int32),
                    seg_pos=up(desc.seg_pos, np.int64, ns), seg_is_fwd_strand=up(desc.seg_is_fwd_strand, np.uint8, ns),
                    seg_cigar_off=up(desc.seg_cigar_off, np.uint32, ns + 1, np.int32), cigar=up(desc.cigar, np.uint32, n_ops, np.int32))
    return UploadedWindow(b, up(fin.read_flags, np.uint16, n, np.int16), up(fin.qual, np.uint8, int(fin.qual_bytes)),
                          up(fin.read_qual_off, np.uint64, n, np.int64), int(fin.qual_bytes))


class PinnedArena:
    """A worker's page-locked landing area for the results of one window at a time (round 5): every array of a HostResults is a slice of ONE
    pinned block that is reused from window to window, filled by asynchronous copies on the worker's stream and waited for once.  (Round 4
    downloaded each of the ~25 arrays into a fresh numpy array with a stream synchronisation of its own: page faults on 90 MB of new
    memory per 7 500-read window and staged copies into pageable memory.  Measured per 60 k reads: lift stage 0.317 -> 0.302 s, record
    assembly -- which reads these arrays -- 0.163 -> 0.102 s; EXPERIMENTS.md 5.15.)"""

    def __init__(self, nbytes: int = 64 << 20):
        self.buf = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        self.used = 0
        self.retired = []  # blocks outgrown while a window's arrays still point into them

    def reset(self):
        self.used = 0
        self.retired = []

    def take(self, nbytes: int) -> torch.Tensor:
        at = (self.used + 63) & ~63
        if at + nbytes > self.buf.numel():
            self.retired.append(self.buf)
            self.buf = torch.empty(max(at + nbytes, self.buf.numel() * 3 // 2), dtype=torch.uint8, pin_memory=True)
            at = 0
        self.used = at + nbytes
        return self.buf[at:at + nbytes]


class HostResults:
    """host copies of a context's device results for one batch -- plo_batch_out (compacted), plo_finish_out, plo_sa_out -- as the
    structs plo_records_build_finished takes (the numpy arrays behind the pointers live as long as this object; with an `arena`: until the
    arena's next reset)"""

    def __init__(self, eng, out: abi.PloBatchOut, fo: abi.PloFinishOut, so: Optional[abi.PloSaOut], n_reads: int, arena: Optional[PinnedArena] = None, dev=None):
        self._keep = []
        pending = []

        def dl(ptr, dtype, count, ctype):
            if arena is None or not count:
                a = eng.download(ptr, dtype, count)
            else:
                from .gather import device_view

                nb = count * np.dtype(dtype).itemsize
                dst = arena.take(nb)
                dst.copy_(device_view(ptr, nb, torch.uint8, dev), non_blocking=True)  # (torch's current stream = the engine's)
                pending.append(dst)
                a = dst.numpy().view(dtype)
            self._keep.append(a)
            return abi._ptr(a, ctype)

        n, nc = int(out.n_items), int(out.n_cigar)
        self.lift = abi.PloBatchOut()
        self.lift.n_items = n
        self.lift.n_cigar = nc
        for name, dt, ct, cnt in (("item_seg", np.uint32, C.c_uint32, n), ("item_cseg", np.uint32, C.c_uint32, n), ("item_status", np.uint8, C.c_uint8, n),
                                  ("item_need_flipped", np.uint8, C.c_uint8, n), ("item_mapq", np.uint8, C.c_uint8, n),
                                  ("item_chrom_index", np.uint32, C.c_uint32, n), ("item_ref_pos", np.int64, C.c_int64, n),
                                  ("item_cigar_off", np.uint64, C.c_uint64, n), ("item_cigar_len", np.uint32, C.c_uint32, n), ("cigar", np.uint32, C.c_uint32, nc)):
            setattr(self.lift, name, dl(getattr(out, name), dt, cnt, ct))
        ctypes_of = {np.uint16: C.c_uint16, np.int64: C.c_int64, np.uint8: C.c_uint8, np.uint64: C.c_uint64, np.uint32: C.c_uint32}
        self.fin = abi.PloFinishOut()
        for name, dt in abi.FINISH_ITEM_FIELDS:
            setattr(self.fin, name, dl(getattr(fo, name), dt, n, ctypes_of[dt]))
        for name, dt in abi.FINISH_READ_FIELDS:
            setattr(self.fin, name, dl(getattr(fo, name), dt, n_reads, ctypes_of[dt]))
        self.fin.rev_seq_bytes, self.fin.rev_qual_bytes = int(fo.rev_seq_bytes), int(fo.rev_qual_bytes)
        self.fin.rev_seq = dl(fo.rev_seq, np.uint8, int(fo.rev_seq_bytes), C.c_uint8)
        self.fin.rev_qual = dl(fo.rev_qual, np.uint8, int(fo.rev_qual_bytes), C.c_uint8)
        self.fin.finish_ms, self.fin.revcomp_ms = fo.finish_ms, fo.revcomp_ms
        self.fin.n_items, self.fin.n_reads = n, n_reads
        self.sa = None
        if so is not None:
            self.sa = abi.PloSaOut()
            self.sa.n_items = int(so.n_items)
            self.sa.item_sa_off = dl(so.item_sa_off, np.uint32, int(so.n_items) + 1, C.c_uint32)
            self.sa.sa_text = dl(so.sa_text, np.uint8, int(so.sa_bytes), C.c_uint8)
            self.sa.sa_bytes = int(so.sa_bytes)
            self.sa.sa_ms = so.sa_ms
        if pending:
            torch.cuda.current_stream().synchronize()  # one wait for all the copies


# ---- a BAM window's records on the device as they stand, the output records assembled there (pipeline.run_bam_to_bam, device_records) ----

@dataclass
class UploadedRawWindow:
    """the window's stretch of the BAM stream in HBM, ONE upload: the batch's bases, the finishing's qualities and the source records of
    plo_records_build_dev are views into `raw`; keeps the tensors alive"""
    raw: torch.Tensor
    raw_bytes: int
    batch: DeviceBatch
    flags: torch.Tensor
    qual_off: torch.Tensor
    rec_off: torch.Tensor

    def finish_in(self) -> abi.PloFinishIn:
        return abi.PloFinishIn(_p(self.flags, C.c_uint16), _p(self.raw, C.c_uint8), _p(self.qual_off, C.c_uint64), self.raw_bytes)

    def records_in(self, labels, is_target_region: bool = False) -> abi.PloRecordsIn:
        """labels: contig_labels(...) of the read->contig BAM's @SQ names"""
        n, t_off, t_blob = labels
        return abi.PloRecordsIn(_p(self.raw, C.c_uint8), self.raw_bytes, _p(self.rec_off, C.c_uint64), n, _p(t_off, C.c_uint32), _p(t_blob, C.c_uint8),
                                1 if is_target_region else 0)


def upload_raw_window(desc: abi.PloBatchIn, fin: abi.PloFinishIn, raw: abi.PloWindowRaw, dev) -> UploadedRawWindow:
    """copies what bam.Window.batch_raw() describes to the device on torch's current stream: the records once, the segment arrays, the
    per-read offsets into the records (bases, qualities, block_size words)"""
    n, ns, nb = int(desc.n_reads), int(desc.n_segs), int(raw.raw_bytes)

    def up(ptr, dtype, count, as_dtype=None):
        if not count:
            return torch.zeros(1, dtype=torch.from_numpy(np.zeros(1, as_dtype or dtype)).dtype, device=dev)[:0]
        a = _host_view(ptr, dtype, count)
        return torch.from_numpy(a.view(as_dtype) if as_dtype is not None else a).to(dev, non_blocking=True)

    t_raw = up(raw.raw, np.uint8, nb) if nb else torch.zeros(16, dtype=torch.uint8, device=dev)
    coff = _host_view(desc.seg_cigar_off, np.uint32, ns + 1)
    n_ops = int(coff[-1]) if ns else 0
    b = DeviceBatch(read_is_reverse=up(desc.read_is_reverse, np.uint8, n), read_seq_len=up(desc.read_seq_len, np.uint32, n, np.int32),
                    read_seq_off=up(desc.read_seq_off, np.uint64, n, np.int64), seq=t_raw[:nb], seq_fmt=int(desc.seq_fmt),
                    seg_read=up(desc.seg_read, np.uint32, ns, np.int32), seg_contig=up(desc.seg_contig, np.uint32, ns, np.int32),
                    seg_pos=up(desc.seg_pos, np.int64, ns), seg_is_fwd_strand=up(desc.seg_is_fwd_strand, np.uint8, ns),
                    seg_cigar_off=up(desc.seg_cigar_off, np.uint32, ns + 1, np.int32), cigar=up(desc.cigar, np.uint32, n_ops, np.int32))
    return UploadedRawWindow(t_raw, nb, b, up(fin.read_flags, np.uint16, n, np.int16), up(fin.read_qual_off, np.uint64, n, np.int64),
                             up(raw.read_rec_off, np.uint64, n, np.int64))


@dataclass
class UploadedRecords:
    """the window's stretch of the BAM stream and read_rec_off in HBM and nothing else (device_batch): the batch is built there
    (api.Engine.batch_build_dev) and handed on by DeviceBuiltWindow; keeps the tensors alive"""
    raw: torch.Tensor
    raw_bytes: int
    rec_off: torch.Tensor
    n_reads: int

    def build_in(self, labels) -> abi.PloBatchBuildIn:
        """labels: contig_labels(...) of the read->contig BAM's @SQ names"""
        n, t_off, t_blob = labels
        return abi.PloBatchBuildIn(_p(self.raw, C.c_uint8), self.raw_bytes, _p(self.rec_off, C.c_uint64), self.n_reads, n, _p(t_off, C.c_uint32), _p(t_blob, C.c_uint8))


def upload_records(raw: abi.PloWindowRaw, dev) -> UploadedRecords:
    """copies what bam.Window.raw() describes to the device on torch's current stream: the records once and their offsets"""
    n, nb = int(raw.n_reads), int(raw.raw_bytes)
    t_raw = torch.from_numpy(_host_view(raw.raw, np.uint8, nb)).to(dev, non_blocking=True) if nb else torch.zeros(16, dtype=torch.uint8, device=dev)
    t_off = (torch.from_numpy(_host_view(raw.read_rec_off, np.uint64, n).view(np.int64)).to(dev, non_blocking=True) if n
             else torch.zeros(1, dtype=torch.int64, device=dev)[:0])
    return UploadedRecords(t_raw, nb, t_off, n)


class DeviceBuiltWindow:
    """what UploadedRawWindow hands on, from a batch built on the device: the plo_batch_in / plo_finish_in of a plo_batch_build_out (arrays
    owned by the engine's context until its next batch_build_dev) and the plo_records_in over the same uploaded records"""

    def __init__(self, up: UploadedRecords, bo: abi.PloBatchBuildOut):
        self.up, self.bo = up, bo
        self.batch_ms = float(bo.batch_ms)

    def desc(self) -> abi.PloBatchIn:
        return self.bo.batch

    def finish_in(self) -> abi.PloFinishIn:
        return self.bo.fin

    def records_in(self, labels, is_target_region: bool = False) -> abi.PloRecordsIn:
        n, t_off, t_blob = labels
        return abi.PloRecordsIn(_p(self.up.raw, C.c_uint8), self.up.raw_bytes, _p(self.up.rec_off, C.c_uint64), n, _p(t_off, C.c_uint32), _p(t_blob, C.c_uint8),
                                1 if is_target_region else 0)


def contig_labels(names, dev):
    """the PS:Z labels (the @SQ names of the read->contig BAM) as device arrays, as sa_inputs carries the reference's: (n, offsets, blob)"""
    sa, keep = sa_inputs(names, dev)
    return int(sa.n_chroms), keep["off"], keep["blob"]


class PinnedPool:
    """page-locked blocks for the record bytes of the windows in flight between a lift worker and the writers: a window's block goes back
    when its bytes are written (DeviceRecords.release), so a handful of blocks serve the whole run"""

    def __init__(self):
        import threading

        self.free = []
        self.lock = threading.Lock()

    def take(self, nbytes: int) -> torch.Tensor:
        with self.lock:
            for k, t in enumerate(self.free):
                if t.numel() >= nbytes:
                    return self.free.pop(k)
            if self.free:  # outgrown: drop the smallest
                self.free.sort(key=lambda t: t.numel())
                self.free.pop(0)
        return torch.empty(max(nbytes + nbytes // 4, 1 << 20), dtype=torch.uint8, pin_memory=True)

    def give(self, t: torch.Tensor):
        with self.lock:
            self.free.append(t)


def _entries_room(nb: int, index_out, n_records: int):
    """where the plo_index_entry values of a plo_index_out stand behind the `nb` bytes of a window in its page-locked block, and the size
    of that block: (at, nbytes).  One block from the pool serves both, so an index costs no page-locked allocation of its own.  The
    index must count the window's `n_records`: the writer sees offsets only and cannot tell that an entry is missing"""
    if index_out is None:
        return nb, nb
    if int(index_out.n_records) != n_records:
        raise ValueError("the index holds %d entries for a window of %d records" % (int(index_out.n_records), n_records))
    at = (nb + 7) & ~7
    return at, at + int(index_out.n_records) * 24


def _entries_down(index_out, dev, block, at: int):
    """the plo_index_entry values of a plo_index_out on their way into `block` at byte `at` (_entries_room; the caller waits for the
    stream) -> a numpy array of abi.INDEX_ENTRY_DTYPE over the block, good until the block is released, or None without an index"""
    from .gather import device_view

    if index_out is None:
        return None
    n = int(index_out.n_records)
    if n:
        block[at:at + n * 24].copy_(device_view(index_out.entry, n * 24, torch.uint8, dev), non_blocking=True)
    return block.numpy()[at:at + n * 24].view(abi.INDEX_ENTRY_DTYPE)


class DeviceRecords:
    """host copy of a plo_records_out: what the writer takes (`bytes`, `n_bytes`) and the counts, as bam.PloRecordBuf has them"""

    def __init__(self, ro: abi.PloRecordsOut, pool: Optional[PinnedPool] = None, dev=None, with_offsets: bool = False,
                 sorted_out: Optional[abi.PloSortOut] = None, index_out: Optional[abi.PloIndexOut] = None):
        """sorted_out: the plo_sort_out of api.Engine.records_sort_dev on `ro` -- its buffer (the same records in coordinate order) and
        offsets are taken instead of ro's.  index_out: the plo_index_out of api.Engine.records_index_dev on the sorted buffer -- its
        entries come down with the bytes, behind them in the same page-locked block (`index_entries`, what bam.BamWriter.index_add takes;
        good until release())"""
        from .gather import device_view

        self.n_bytes, self.n_records = int(ro.n_bytes), int(ro.n_records)
        self.n_lifted, self.n_unmapped_copies = int(ro.n_lifted), int(ro.n_unmapped_copies)
        self.records_ms = float(ro.records_ms)
        self._pool = pool
        import time

        at, nb = _entries_room(max(16, self.n_bytes), index_out, self.n_records)
        t0 = time.perf_counter()
        self._block = pool.take(nb) if pool is not None else torch.empty(nb, dtype=torch.uint8, pin_memory=True)
        t1 = time.perf_counter()
        self.record_off = None
        src = sorted_out if sorted_out is not None else ro
        if self.n_bytes:
            self._block[:self.n_bytes].copy_(device_view(src.bytes, self.n_bytes, torch.uint8, dev), non_blocking=True)  # ONE copy, on the current stream
        if with_offsets:
            off = torch.empty((self.n_records + 1) * 8, dtype=torch.uint8, pin_memory=True)
            off.copy_(device_view(src.record_off, (self.n_records + 1) * 8, torch.uint8, dev), non_blocking=True)
            self.record_off = off.numpy().view(np.uint64)
        self.index_entries = _entries_down(index_out, dev, self._block, at)
        torch.cuda.current_stream().synchronize()
        self.block_s, self.copy_s = t1 - t0, time.perf_counter() - t1  # the page-locked block (a fresh one is an allocation) / the copy
        self.bytes = self._block.data_ptr()

    def data(self) -> bytes:
        return self._block[:self.n_bytes].numpy().tobytes()

    def release(self):
        if self._pool is not None and self._block is not None:
            self._pool.give(self._block)
        self._block = None


class DeviceBlocks:
    """the records of a plo_records_out compressed on the device (api.Engine.bgzf_compress_dev) and brought down as finished BGZF blocks:
    what bam.BamWriter.write_blocks takes (`bytes`, `n_bytes`), the counts of the records as DeviceRecords has them, `n_in` = the record
    bytes the blocks hold.  The record bytes themselves never leave the device."""
    is_blocks = True

    def __init__(self, eng, ro: abi.PloRecordsOut, level: int, pool: Optional[PinnedPool] = None, dev=None, sorted_out: Optional[abi.PloSortOut] = None,
                 index_out: Optional[abi.PloIndexOut] = None):
        """sorted_out, index_out: as for DeviceRecords -- the sorted buffer is compressed instead of ro's, the entries come down with the
        blocks"""
        from .gather import device_view
        import time

        self.n_records, self.n_lifted, self.n_unmapped_copies = int(ro.n_records), int(ro.n_lifted), int(ro.n_unmapped_copies)
        self.records_ms = float(ro.records_ms)
        bo = eng.bgzf_compress_dev((sorted_out if sorted_out is not None else ro).bytes, int(ro.n_bytes), level)
        self.n_in, self.n_bytes, self.n_blocks, self.bgzf_ms = int(bo.n_in), int(bo.n_bytes), int(bo.n_blocks), float(bo.bgzf_ms)
        self._pool = pool
        at, nb = _entries_room(max(16, self.n_bytes), index_out, self.n_records)
        t0 = time.perf_counter()
        self._block = pool.take(nb) if pool is not None else torch.empty(nb, dtype=torch.uint8, pin_memory=True)
        t1 = time.perf_counter()
        if self.n_bytes:
            self._block[:self.n_bytes].copy_(device_view(bo.blocks, self.n_bytes, torch.uint8, dev), non_blocking=True)
        self.index_entries = _entries_down(index_out, dev, self._block, at)
        torch.cuda.current_stream().synchronize()
        self.block_s, self.copy_s = t1 - t0, time.perf_counter() - t1
        self.bytes = self._block.data_ptr()

    def data(self) -> bytes:
        return self._block[:self.n_bytes].numpy().tobytes()

    def release(self):
        if self._pool is not None and self._block is not None:
            self._pool.give(self._block)
        self._block = None


class RetainedWindow:
    """one window's coordinate-sorted records kept on the device in allocations of its own: a device-to-device copy of the plo_sort_out
    of api.Engine.records_sort_dev, which the context overwrites at its next sort.  What api.Engine.runs_merge_plan_dev takes as a run
    (`run()`); the copy is made on the current stream and waited for, so another thread's context may read it.  `free()` gives the
    memory back."""

    def __init__(self, so: abi.PloSortOut, dev=None):
        from .gather import device_view

        self.n_bytes, self.n_records = int(so.n_bytes), int(so.n_records)
        self.raw = torch.empty(max(16, self.n_bytes), dtype=torch.uint8, device=dev)
        self.off = torch.empty((self.n_records + 1) * 8, dtype=torch.uint8, device=dev)
        if self.n_bytes:
            self.raw[:self.n_bytes].copy_(device_view(so.bytes, self.n_bytes, torch.uint8, dev), non_blocking=True)
        self.off.copy_(device_view(so.record_off, (self.n_records + 1) * 8, torch.uint8, dev), non_blocking=True)
        torch.cuda.current_stream().synchronize()

    def run(self):
        """(bytes, n_bytes, n_records, record_off) as device addresses"""
        return self.raw.data_ptr(), self.n_bytes, self.n_records, self.off.data_ptr()

    def free(self):
        self.raw = self.off = None


class MergedChunk:
    """a chunk of a merge plan (api.Engine.runs_merge_emit_dev) in the shape DeviceRecords and DeviceBlocks take for `ro`: bytes, n_bytes,
    n_records, record_off; the counts of the lift are the windows' own and stay with them (0 here).  Good until the engine's next emit."""
    n_lifted = n_unmapped_copies = 0
    records_ms = 0.0

    def __init__(self, co: abi.PloMergeChunkOut, chunk: int):
        self.chunk, self.bytes, self.n_bytes, self.n_records, self.record_off = chunk, co.bytes, int(co.n_bytes), int(co.n_records), co.record_off
        self.first_record, self.emit_ms = int(co.first_record), float(co.emit_ms)


def merged_chunks(eng, plan: abi.PloMergeOut):
    """the chunks of `plan` (api.Engine.runs_merge_plan_dev on `eng`), emitted one after the other in merged order: every MergedChunk is good
    until the next one is asked for, so the consumer indexes, compresses or downloads it before it goes on"""
    for c in range(int(plan.n_chunks)):
        yield MergedChunk(eng.runs_merge_emit_dev(c), c)


class RetainedCounts:
    """what the pipeline counts of a window whose records stay on the device for the merger: the fields of DeviceRecords without a byte"""
    bytes = None

    def __init__(self, ro: abi.PloRecordsOut):
        self.n_bytes, self.n_records = int(ro.n_bytes), int(ro.n_records)
        self.n_lifted, self.n_unmapped_copies, self.records_ms = int(ro.n_lifted), int(ro.n_unmapped_copies), float(ro.records_ms)
