"""ctypes mirror of ``include/portello_liftover.h`` plus numpy containers that build the descriptors.

Nothing in here computes anything: it only lays arrays out the way the C ABI wants them.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

PLO_OK = 0
PLO_ERR_INVALID_ARG = 1
PLO_ERR_NO_DEVICE = 2
PLO_ERR_HIP = 3
PLO_ERR_OUT_OF_MEMORY = 4
PLO_ERR_RANGE = 5
PLO_ERR_INTERNAL = 6
PLO_ERR_IO = 7
PLO_ERR_DATA = 8

ITEM_LIFTED = 0
ITEM_NO_LIFTOVER = 1
ITEM_LEN_MISMATCH = 2
ITEM_PANIC = 3
ITEM_NEED_BASES = 4  # sparse bases only: a comparison reached bases the batch does not carry (and no seq_full was given)

SEQ_BAM4 = 0
SEQ_ASCII = 1
SEQ_BAM4_SPARSE = 2

MEM_HOST = 0
MEM_DEVICE = 1

STAGE_STRAND = 1 << 0
STAGE_LSHIFT = 1 << 1
STAGE_LIFTOVER = 1 << 2
STAGE_LENCHECK = 1 << 3
STAGE_SIMPLIFY = 1 << 4
STAGES_ALL = 0x1F

NONE_VAL = -(2**63)  # INT64_MIN: Option::None for block-map values

_u8p = C.POINTER(C.c_uint8)
_u32p = C.POINTER(C.c_uint32)
_u64p = C.POINTER(C.c_uint64)
_i64p = C.POINTER(C.c_int64)
_pp = C.POINTER(C.c_void_p)


class PloIndexDesc(C.Structure):
    _fields_ = [
        ("n_contigs", C.c_uint32),
        ("contig_len", _i64p),
        ("contig_seg_off", _u32p),
        ("n_segments", C.c_uint32),
        ("seg_chrom_index", _u32p),
        ("seg_pos", _i64p),
        ("seg_is_fwd_strand", _u8p),
        ("seg_mapq", _u8p),
        ("seg_seq_order_start", _i64p),
        ("seg_seq_order_end", _i64p),
        ("seg_cigar_off", _u32p),
        ("seg_cigar", _u32p),
        ("n_chroms", C.c_uint32),
        ("chrom_len", _i64p),
        ("chrom_seq", _pp),
        ("rev_contig_seq", _pp),
        ("seq_mem", C.c_int32),
    ]


# plo_fasta_* (the reference FASTA loaded on the device)
FA_ERR_NONE, FA_ERR_BAD_BYTE, FA_ERR_NO_HEADER, FA_ERR_MISSING, FA_ERR_LENGTH, FA_ERR_DUPLICATE = 0, 1, 2, 3, 4, 5


class PloFastaWant(C.Structure):
    _fields_ = [("n", C.c_uint32), ("names", C.POINTER(C.c_char_p)), ("lens", _i64p)]


class PloFastaOut(C.Structure):
    _fields_ = [
        ("n_chroms", C.c_uint32),
        ("chrom_len", _i64p),
        ("chrom_seq", _pp),
        ("n_records_seen", C.c_uint64),
        ("n_bases", C.c_uint64),
        ("text_bytes", C.c_uint64),
        ("fasta_ms", C.c_float),
        ("err_kind", C.c_int32),
        ("err_offset", C.c_uint64),
        ("err_chrom", C.c_uint32),
        ("err_len", C.c_int64),
    ]


class PloBatchIn(C.Structure):
    _fields_ = [
        ("n_reads", C.c_uint32),
        ("read_is_reverse", _u8p),
        ("read_seq_len", _u32p),
        ("read_seq_off", _u64p),
        ("seq", _u8p),
        ("seq_bytes", C.c_uint64),
        ("seq_fmt", C.c_int32),
        ("n_segs", C.c_uint32),
        ("seg_read", _u32p),
        ("seg_contig", _u32p),
        ("seg_pos", _i64p),
        ("seg_is_fwd_strand", _u8p),
        ("seg_cigar_off", _u32p),
        ("cigar", _u32p),
        ("n_items", C.c_uint32),
        ("item_seg", _u32p),
        ("item_cseg", _u32p),
        ("seq_full", _u8p),
        ("read_seq_full_off", _u64p),
    ]


class PloBatchOut(C.Structure):
    _fields_ = [
        ("n_items", C.c_uint32),
        ("item_seg", _u32p),
        ("item_cseg", _u32p),
        ("item_status", _u8p),
        ("item_need_flipped", _u8p),
        ("item_mapq", _u8p),
        ("item_chrom_index", _u32p),
        ("item_ref_pos", _i64p),
        ("item_cigar_off", _u64p),
        ("item_cigar_len", _u32p),
        ("cigar", _u32p),
        ("n_cigar", C.c_uint64),
    ]


PLO_API_VERSION = 20  # include/portello_liftover.h


class PloTiming(C.Structure):
    _fields_ = [
        ("struct_size", C.c_uint32),
        ("total_ms", C.c_float),
        ("enumerate_ms", C.c_float),
        ("lift_ms", C.c_float),
        ("big_ms", C.c_float),
        ("n_items", C.c_uint32),
        ("n_big_items", C.c_uint32),
        ("n_in_ops", C.c_uint64),
        ("n_out_ops", C.c_uint64),
        ("algo_bytes", C.c_uint64),
        ("lanes_ms", C.c_float),
        ("retry_ms", C.c_float),
        ("n_lane_items", C.c_uint32),
        ("n_retry_items", C.c_uint32),
        ("mid_ms", C.c_float),
        ("n_mid_items", C.c_uint32),
        ("n_miss_items", C.c_uint32),
        ("miss_ms", C.c_float),
        ("tile_cap", C.c_uint32),
        ("tile_window", C.c_uint32),
        ("heavy_lanes_ms", C.c_float),
        ("n_heavy_lane_items", C.c_uint32),
        ("lane_utilisation", C.c_float),
        ("heavy_kernel", C.c_uint32),
        ("host_syncs", C.c_uint32),
    ]


_u16p = C.POINTER(C.c_uint16)
NO_FLIP = 2**64 - 1


class PloFinishIn(C.Structure):
    _fields_ = [("read_flags", _u16p), ("qual", _u8p), ("read_qual_off", _u64p), ("qual_bytes", C.c_uint64)]


class PloFinishOut(C.Structure):
    _fields_ = [
        ("item_flag", _u16p), ("item_bin", _u16p), ("item_ref_end", _i64p), ("item_is_primary", _u8p),
        ("item_seq_off", _u64p), ("item_qual_off", _u64p),
        ("read_n_lifted", _u32p), ("read_primary_item", _u32p), ("read_unmapped_flag", _u16p),
        ("read_seq_off", _u64p), ("read_qual_off", _u64p),
        ("rev_seq", _u8p), ("rev_qual", _u8p), ("rev_seq_bytes", C.c_uint64), ("rev_qual_bytes", C.c_uint64),
        ("finish_ms", C.c_float), ("revcomp_ms", C.c_float),
        ("n_items", C.c_uint32), ("n_reads", C.c_uint32),
    ]


class PloSaIn(C.Structure):
    _fields_ = [("n_chroms", C.c_uint32), ("chrom_name_off", _u32p), ("chrom_names", _u8p)]


class PloSaOut(C.Structure):
    _fields_ = [("n_items", C.c_uint32), ("item_sa_off", _u32p), ("sa_text", _u8p), ("sa_bytes", C.c_uint64), ("sa_ms", C.c_float)]


class PloRecordsIn(C.Structure):
    _fields_ = [("records", _u8p), ("records_bytes", C.c_uint64), ("read_rec_off", _u64p), ("n_contigs", C.c_uint32),
                ("contig_name_off", _u32p), ("contig_names", _u8p), ("is_target_region", C.c_int32)]


class PloRecordsOut(C.Structure):
    _fields_ = [("bytes", _u8p), ("n_bytes", C.c_uint64), ("n_records", C.c_uint32), ("record_off", _u64p), ("n_lifted", C.c_uint32),
                ("n_unmapped_copies", C.c_uint32), ("records_ms", C.c_float)]


class PloNmOut(C.Structure):
    _fields_ = [("n_items", C.c_uint32), ("item_nm", _u32p), ("n_cmp_bases", C.c_uint64), ("err_item", C.c_uint32), ("nm_ms", C.c_float)]


class PloMdOut(C.Structure):
    _fields_ = [("n_items", C.c_uint32), ("item_md_off", _u64p), ("md_text", _u8p), ("md_bytes", C.c_uint64), ("err_item", C.c_uint32), ("md_ms", C.c_float)]


class PloSortIn(C.Structure):
    _fields_ = [("bytes", _u8p), ("n_bytes", C.c_uint64), ("n_records", C.c_uint32), ("record_off", _u64p), ("n_ref", C.c_uint32)]


class PloSortOut(C.Structure):
    _fields_ = [("bytes", _u8p), ("n_bytes", C.c_uint64), ("n_records", C.c_uint32), ("record_off", _u64p), ("perm", _u32p), ("key", _u64p),
                ("n_mapped", C.c_uint32), ("err_record", C.c_uint32), ("sort_ms", C.c_float)]


PLO_MERGE_MAX_RUNS = 4096


class PloMergeRun(C.Structure):
    _fields_ = [("bytes", _u8p), ("n_bytes", C.c_uint64), ("n_records", C.c_uint32), ("record_off", _u64p)]


class PloMergeIn(C.Structure):
    _fields_ = [("runs", C.POINTER(PloMergeRun)), ("n_runs", C.c_uint32), ("n_ref", C.c_uint32), ("chunk_bytes", C.c_uint64)]


class PloMergeOut(C.Structure):
    """chunk_first / chunk_off are HOST arrays of n_chunks + 1 values, the rest device pointers"""
    _fields_ = [("n_records", C.c_uint32), ("n_mapped", C.c_uint32), ("n_bytes", C.c_uint64), ("src", _u32p), ("key", _u64p), ("record_off", _u64p),
                ("n_chunks", C.c_uint32), ("chunk_first", _u32p), ("chunk_off", _u64p), ("err_run", C.c_uint32), ("err_record", C.c_uint32),
                ("err_kind", C.c_uint32), ("plan_ms", C.c_float)]


class PloMergeChunkOut(C.Structure):
    _fields_ = [("bytes", _u8p), ("n_bytes", C.c_uint64), ("n_records", C.c_uint32), ("first_record", C.c_uint32), ("record_off", _u64p),
                ("emit_ms", C.c_float)]


class PloIndexEntry(C.Structure):
    """24 bytes: off, ref_id, beg, end, flags (bit 0: FLAG & 4; bits 16..31: reg2bin(beg, end))"""
    _fields_ = [("off", C.c_uint64), ("ref_id", C.c_int32), ("beg", C.c_int32), ("end", C.c_int32), ("flags", C.c_uint32)]


INDEX_ENTRY_DTYPE = np.dtype([("off", "<u8"), ("ref_id", "<i4"), ("beg", "<i4"), ("end", "<i4"), ("flags", "<u4")])  # plo_index_entry as a numpy record


class PloIndexIn(C.Structure):
    _fields_ = [("bytes", _u8p), ("n_bytes", C.c_uint64), ("n_records", C.c_uint32), ("record_off", _u64p), ("n_ref", C.c_uint32)]


class PloIndexOut(C.Structure):
    _fields_ = [("entry", C.POINTER(PloIndexEntry)), ("n_records", C.c_uint32), ("n_placed", C.c_uint32), ("err_record", C.c_uint32), ("err_kind", C.c_uint32),
                ("index_ms", C.c_float)]


DEPTH_EXCLUDE_DEFAULT = 0x704  # PLO_DEPTH_EXCLUDE_DEFAULT: unmapped, secondary, QC-fail, duplicate


class PloDepthOpts(C.Structure):
    _fields_ = [("exclude_flags", C.c_uint32), ("count_deletions", C.c_int32)]


class PloDepthInfo(C.Structure):
    """array: device; slot_off: HOST [n_ref + 1]"""
    _fields_ = [("array", C.POINTER(C.c_int32)), ("n_entries", C.c_uint64), ("slot_off", _u64p), ("bytes_allocated", C.c_uint64), ("n_ref", C.c_uint32),
                ("exclude_flags", C.c_uint32), ("count_deletions", C.c_int32), ("finished", C.c_int32)]


class PloDepthIn(C.Structure):
    _fields_ = [("bytes", _u8p), ("n_bytes", C.c_uint64), ("n_records", C.c_uint32), ("record_off", _u64p)]


class PloDepthAddOut(C.Structure):
    _fields_ = [("n_records", C.c_uint32), ("n_counted", C.c_uint32), ("err_record", C.c_uint32), ("err_kind", C.c_uint32), ("add_ms", C.c_float)]


class PloDepthWindowsOut(C.Structure):
    """sum / win_first are HOST arrays of n_windows and n_ref + 1 values"""
    _fields_ = [("sum", _u64p), ("win_first", _u64p), ("n_windows", C.c_uint64), ("windows_ms", C.c_float)]


class PloDepthRun(C.Structure):
    """16 bytes: ref_id, [beg, end), depth"""
    _fields_ = [("ref_id", C.c_int32), ("beg", C.c_int32), ("end", C.c_int32), ("depth", C.c_int32)]


DEPTH_RUN_DTYPE = np.dtype([("ref_id", "<i4"), ("beg", "<i4"), ("end", "<i4"), ("depth", "<i4")])  # plo_depth_run as a numpy record


class PloDepthRunsOut(C.Structure):
    _fields_ = [("run", C.POINTER(PloDepthRun)), ("n_runs", C.c_uint64), ("runs_ms", C.c_float)]


PILEUP_CHANNELS = 8  # PLO_PILEUP_CHANNELS
PILEUP_CHANNEL_NAMES = ("A", "C", "G", "T", "N", "DEL", "INS", "CLIP")
PILEUP_MASK_DEFAULT = 0x6F  # PLO_PILEUP_MASK_DEFAULT: A C G T DEL INS


class PloPileupRegion(C.Structure):
    _fields_ = [("ref_id", C.c_int32), ("beg", C.c_int32), ("end", C.c_int32)]


class PloPileupOpts(C.Structure):
    _fields_ = [("exclude_flags", C.c_uint32), ("n_regions", C.c_uint32), ("regions", C.POINTER(PloPileupRegion))]


class PloPileupInfo(C.Structure):
    """array: device [n_bases * 8]; slot_off [n_ref + 1] (in bases), slot_beg and slot_end [n_ref]: HOST"""
    _fields_ = [("array", C.POINTER(C.c_int32)), ("n_bases", C.c_uint64), ("slot_off", _u64p), ("slot_beg", C.POINTER(C.c_int32)), ("slot_end", C.POINTER(C.c_int32)),
                ("bytes_allocated", C.c_uint64), ("n_ref", C.c_uint32), ("exclude_flags", C.c_uint32)]


class PloPileupAddOut(C.Structure):
    _fields_ = [("n_records", C.c_uint32), ("n_counted", C.c_uint32), ("err_record", C.c_uint32), ("err_kind", C.c_uint32), ("n_events", C.c_uint64), ("add_ms", C.c_float)]


class PloPileupSitesOpts(C.Structure):
    _fields_ = [("channel_mask", C.c_uint32), ("min_count", C.c_int32), ("frac_num", C.c_uint32), ("frac_den", C.c_uint32)]


class PloPileupSite(C.Structure):
    """48 bytes: ref_id, pos, depth (-1 without a depth object), ref_base, the eight counters"""
    _fields_ = [("ref_id", C.c_int32), ("pos", C.c_int32), ("depth", C.c_int32), ("ref_base", C.c_uint8), ("pad", C.c_uint8 * 3), ("count", C.c_int32 * 8)]


PILEUP_SITE_DTYPE = np.dtype([("ref_id", "<i4"), ("pos", "<i4"), ("depth", "<i4"), ("ref_base", "u1"), ("pad", "u1", (3,)), ("count", "<i4", (8,))])  # plo_pileup_site


class PloPileupSitesOut(C.Structure):
    _fields_ = [("site", C.POINTER(PloPileupSite)), ("n_sites", C.c_uint64), ("sites_ms", C.c_float)]


class PloEqxOut(C.Structure):
    _fields_ = [("n_items", C.c_uint32), ("item_eqx_off", _u64p), ("eqx_ops", _u32p), ("n_ops", C.c_uint64), ("err_item", C.c_uint32), ("eqx_ms", C.c_float)]


class PloBgzfOut(C.Structure):
    _fields_ = [("blocks", _u8p), ("n_bytes", C.c_uint64), ("n_blocks", C.c_uint32), ("block_off", _u64p), ("n_in", C.c_uint64), ("bgzf_ms", C.c_float)]


# plo_bb_err: what plo_batch_build_dev found in the lowest failing read
BB_ERR_NONE = 0
BB_ERR_SA_NOT_Z = 1
BB_ERR_FIELD_COUNT = 2
BB_ERR_MALFORMED = 3
BB_ERR_UNALIGNED = 4
BB_ERR_READ_SIZE = 5
BB_ERR_UNKNOWN_CONTIG = 6
BB_ERR_EMPTY_SEGMENT = 7
BB_NO_READ = 0xFFFFFFFF


class PloBatchBuildIn(C.Structure):
    _fields_ = [("records", _u8p), ("records_bytes", C.c_uint64), ("read_rec_off", _u64p), ("n_reads", C.c_uint32), ("n_contigs", C.c_uint32),
                ("contig_name_off", _u32p), ("contig_names", _u8p)]


class PloBatchBuildOut(C.Structure):
    _fields_ = [("batch", PloBatchIn), ("fin", PloFinishIn), ("err_read", C.c_uint32), ("err_kind", C.c_uint32), ("batch_ms", C.c_float)]


# plo_cut_end: why a window of plo_window_cut_dev ended
CUT_MAX_RECORDS = 0
CUT_MAX_UNMAPPED = 1
CUT_MAX_BYTES = 2
CUT_END_OF_BYTES = 3
CUT_EOF = 4
CUT_PART_END = 5  # plo_window_cut_part_dev: the next record starts at or behind own_bytes
CUT_SEG_BYTES = 32768
CUT_NO_ERR = 0xFFFFFFFFFFFFFFFF


class PloBgzfInflateIn(C.Structure):
    _fields_ = [("bgzf", _u8p), ("bgzf_bytes", C.c_uint64), ("dst", _u8p), ("dst_cap", C.c_uint64)]


class PloBgzfInflateOut(C.Structure):
    _fields_ = [("n_blocks", C.c_uint32), ("bgzf_consumed", C.c_uint64), ("n_bytes", C.c_uint64), ("inflate_ms", C.c_float)]


class PloWindowCutIn(C.Structure):
    _fields_ = [("stream", _u8p), ("stream_bytes", C.c_uint64), ("max_records", C.c_uint32), ("max_unmapped", C.c_uint64), ("max_bytes", C.c_uint64),
                ("final", C.c_int32)]


class PloWindowCutOut(C.Structure):
    _fields_ = [("n_reads", C.c_uint32), ("read_rec_off", _u64p), ("n_unmapped", C.c_uint32), ("unmapped_off", _u64p), ("unmapped", _u8p),
                ("unmapped_bytes", C.c_uint64), ("window_bytes", C.c_uint64), ("ended_by", C.c_int32), ("err_off", C.c_uint64), ("cut_ms", C.c_float),
                ("n_rewalks", C.c_uint32)]


# API 11: one part of a file on the device
PART_FOUND = 0
PART_NEED_MORE = 1
PART_NONE = 2
NO_RANGE_END = 0xFFFFFFFFFFFFFFFF


class PloBgzfInflatePartIn(C.Structure):
    _fields_ = [("bgzf", _u8p), ("bgzf_bytes", C.c_uint64), ("dst", _u8p), ("dst_cap", C.c_uint64), ("bgzf_file_off", C.c_uint64), ("range_end", C.c_uint64)]


class PloBgzfInflatePartOut(C.Structure):
    _fields_ = [("n_blocks", C.c_uint32), ("bgzf_consumed", C.c_uint64), ("n_bytes", C.c_uint64), ("inflate_ms", C.c_float), ("own_bytes", C.c_uint64)]


class PloWindowCutPartIn(C.Structure):
    _fields_ = [("stream", _u8p), ("stream_bytes", C.c_uint64), ("max_records", C.c_uint32), ("max_unmapped", C.c_uint64), ("max_bytes", C.c_uint64),
                ("final", C.c_int32), ("own_bytes", C.c_uint64)]


class PloPartStartIn(C.Structure):
    _fields_ = [("stream", _u8p), ("stream_bytes", C.c_uint64), ("n_ref", C.c_uint32), ("final", C.c_int32)]


class PloPartStartOut(C.Structure):
    _fields_ = [("kind", C.c_int32), ("first_off", C.c_uint64), ("start_ms", C.c_float)]


class PloWindowRaw(C.Structure):  # include/portello_bam.h
    _fields_ = [("raw", _u8p), ("raw_bytes", C.c_uint64), ("n_reads", C.c_uint32), ("read_rec_off", _u64p)]


FINISH_ITEM_FIELDS = [("item_flag", np.uint16), ("item_bin", np.uint16), ("item_ref_end", np.int64), ("item_is_primary", np.uint8),
                      ("item_seq_off", np.uint64), ("item_qual_off", np.uint64)]
FINISH_READ_FIELDS = [("read_n_lifted", np.uint32), ("read_primary_item", np.uint32), ("read_unmapped_flag", np.uint16),
                      ("read_seq_off", np.uint64), ("read_qual_off", np.uint64)]


def _np(a, dtype) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=dtype))


def _ptr(a: Optional[np.ndarray], ctype):
    if a is None:
        return C.cast(None, C.POINTER(ctype))
    return a.ctypes.data_as(C.POINTER(ctype))


@dataclass
class IndexData:
    """Host-side picture of AllContigMappingInfo + reference (src/contig_alignment_scanner/mod.rs:25-47,76)."""

    contig_len: np.ndarray
    contig_seg_off: np.ndarray
    seg_chrom_index: np.ndarray
    seg_pos: np.ndarray
    seg_is_fwd_strand: np.ndarray
    seg_mapq: np.ndarray
    seg_seq_order_start: np.ndarray
    seg_seq_order_end: np.ndarray
    seg_cigar_off: np.ndarray
    seg_cigar: np.ndarray
    chrom_seq: List[np.ndarray]  # uint8 arrays (host) -- or ints (device pointers) when seq_mem == MEM_DEVICE
    rev_contig_seq: List[Optional[np.ndarray]]
    chrom_len: Optional[np.ndarray] = None
    seq_mem: int = MEM_HOST
    _keep: list = field(default_factory=list, repr=False)

    def __post_init__(self):
        self.contig_len = _np(self.contig_len, np.int64)
        self.contig_seg_off = _np(self.contig_seg_off, np.uint32)
        self.seg_chrom_index = _np(self.seg_chrom_index, np.uint32)
        self.seg_pos = _np(self.seg_pos, np.int64)
        self.seg_is_fwd_strand = _np(self.seg_is_fwd_strand, np.uint8)
        self.seg_mapq = _np(self.seg_mapq, np.uint8)
        self.seg_seq_order_start = _np(self.seg_seq_order_start, np.int64)
        self.seg_seq_order_end = _np(self.seg_seq_order_end, np.int64)
        self.seg_cigar_off = _np(self.seg_cigar_off, np.uint32)
        self.seg_cigar = _np(self.seg_cigar, np.uint32)
        if self.seq_mem == MEM_HOST:
            self.chrom_seq = [_np(s, np.uint8) for s in self.chrom_seq]
            self.rev_contig_seq = [None if s is None else _np(s, np.uint8) for s in self.rev_contig_seq]
            if self.chrom_len is None:
                self.chrom_len = np.array([len(s) for s in self.chrom_seq], dtype=np.int64)
        self.chrom_len = _np(self.chrom_len, np.int64)

    @property
    def n_contigs(self) -> int:
        return len(self.contig_len)

    @property
    def n_segments(self) -> int:
        return len(self.seg_pos)

    def to_desc(self) -> PloIndexDesc:
        d = PloIndexDesc()
        d.n_contigs = self.n_contigs
        d.contig_len = _ptr(self.contig_len, C.c_int64)
        d.contig_seg_off = _ptr(self.contig_seg_off, C.c_uint32)
        d.n_segments = self.n_segments
        d.seg_chrom_index = _ptr(self.seg_chrom_index, C.c_uint32)
        d.seg_pos = _ptr(self.seg_pos, C.c_int64)
        d.seg_is_fwd_strand = _ptr(self.seg_is_fwd_strand, C.c_uint8)
        d.seg_mapq = _ptr(self.seg_mapq, C.c_uint8)
        d.seg_seq_order_start = _ptr(self.seg_seq_order_start, C.c_int64)
        d.seg_seq_order_end = _ptr(self.seg_seq_order_end, C.c_int64)
        d.seg_cigar_off = _ptr(self.seg_cigar_off, C.c_uint32)
        d.seg_cigar = _ptr(self.seg_cigar, C.c_uint32)
        d.n_chroms = len(self.chrom_seq)
        d.chrom_len = _ptr(self.chrom_len, C.c_int64)

        def addr(s):
            if s is None:
                return None
            return int(s) if self.seq_mem == MEM_DEVICE else s.ctypes.data

        chrom_ptrs = (C.c_void_p * max(1, len(self.chrom_seq)))(*[addr(s) for s in self.chrom_seq])
        rev_ptrs = (C.c_void_p * max(1, self.n_contigs))(*[addr(s) for s in self.rev_contig_seq])
        self._keep = [chrom_ptrs, rev_ptrs] + [k for k in self._keep if not isinstance(k, C.Array)]  # (owners of device sequences stay)
        d.chrom_seq = C.cast(chrom_ptrs, _pp)
        d.rev_contig_seq = C.cast(rev_ptrs, _pp)
        d.seq_mem = self.seq_mem
        return d


@dataclass
class BatchData:
    """Host-side picture of one window of primary reads with their split segments."""

    read_is_reverse: np.ndarray
    read_seq_len: np.ndarray
    read_seq_off: np.ndarray
    seq: np.ndarray
    seq_fmt: int
    seg_read: np.ndarray
    seg_contig: np.ndarray
    seg_pos: np.ndarray
    seg_is_fwd_strand: np.ndarray
    seg_cigar_off: np.ndarray
    cigar: np.ndarray
    item_seg: Optional[np.ndarray] = None
    item_cseg: Optional[np.ndarray] = None
    # seq_fmt SEQ_BAM4_SPARSE: the reads' complete BAM4 bases (host), looked up when a comparison runs past the granules sent
    seq_full: Optional[np.ndarray] = None
    read_seq_full_off: Optional[np.ndarray] = None

    def __post_init__(self):
        self.read_is_reverse = _np(self.read_is_reverse, np.uint8)
        self.read_seq_len = _np(self.read_seq_len, np.uint32)
        self.read_seq_off = _np(self.read_seq_off, np.uint64)
        self.seq = _np(self.seq, np.uint8)
        self.seg_read = _np(self.seg_read, np.uint32)
        self.seg_contig = _np(self.seg_contig, np.uint32)
        self.seg_pos = _np(self.seg_pos, np.int64)
        self.seg_is_fwd_strand = _np(self.seg_is_fwd_strand, np.uint8)
        self.seg_cigar_off = _np(self.seg_cigar_off, np.uint32)
        self.cigar = _np(self.cigar, np.uint32)
        if self.item_seg is not None:
            self.item_seg = _np(self.item_seg, np.uint32)
            self.item_cseg = _np(self.item_cseg, np.uint32)
        if self.seq_full is not None:
            self.seq_full = _np(self.seq_full, np.uint8)
            self.read_seq_full_off = _np(self.read_seq_full_off, np.uint64)

    @property
    def n_reads(self) -> int:
        return len(self.read_seq_len)

    @property
    def n_segs(self) -> int:
        return len(self.seg_read)

    def to_desc(self) -> PloBatchIn:
        b = PloBatchIn()
        b.n_reads = self.n_reads
        b.read_is_reverse = _ptr(self.read_is_reverse, C.c_uint8)
        b.read_seq_len = _ptr(self.read_seq_len, C.c_uint32)
        b.read_seq_off = _ptr(self.read_seq_off, C.c_uint64)
        b.seq = _ptr(self.seq, C.c_uint8)
        b.seq_bytes = self.seq.nbytes
        b.seq_fmt = self.seq_fmt
        b.n_segs = self.n_segs
        b.seg_read = _ptr(self.seg_read, C.c_uint32)
        b.seg_contig = _ptr(self.seg_contig, C.c_uint32)
        b.seg_pos = _ptr(self.seg_pos, C.c_int64)
        b.seg_is_fwd_strand = _ptr(self.seg_is_fwd_strand, C.c_uint8)
        b.seg_cigar_off = _ptr(self.seg_cigar_off, C.c_uint32)
        b.cigar = _ptr(self.cigar, C.c_uint32)
        if self.item_seg is not None:
            b.n_items = len(self.item_seg)
            b.item_seg = _ptr(self.item_seg, C.c_uint32)
            b.item_cseg = _ptr(self.item_cseg, C.c_uint32)
        else:
            b.n_items = 0
            b.item_seg = _ptr(None, C.c_uint32)
            b.item_cseg = _ptr(None, C.c_uint32)
        b.seq_full = _ptr(self.seq_full, C.c_uint8)
        b.read_seq_full_off = _ptr(self.read_seq_full_off, C.c_uint64)
        return b


@dataclass
class BatchResult:
    """Host copy of a plo_batch_out."""

    item_seg: np.ndarray
    item_cseg: np.ndarray
    item_status: np.ndarray
    item_need_flipped: np.ndarray
    item_mapq: np.ndarray
    item_chrom_index: np.ndarray
    item_ref_pos: np.ndarray
    item_cigar_off: np.ndarray
    item_cigar_len: np.ndarray
    cigar: np.ndarray

    @property
    def n_items(self) -> int:
        return len(self.item_seg)

    def item_cigar(self, i: int) -> np.ndarray:
        o = int(self.item_cigar_off[i])
        return self.cigar[o : o + int(self.item_cigar_len[i])]

    def canonical(self):
        """Order-independent, layout-independent view used by the parity tests: per item
        (seg, cseg, status, flip, mapq, chrom, pos, cigar-bytes)."""
        rows = []
        for i in range(self.n_items):
            rows.append(
                (
                    int(self.item_seg[i]),
                    int(self.item_cseg[i]),
                    int(self.item_status[i]),
                    int(self.item_need_flipped[i]),
                    int(self.item_mapq[i]),
                    int(self.item_chrom_index[i]),
                    int(self.item_ref_pos[i]),
                    self.item_cigar(i).tobytes(),
                )
            )
        return rows


def result_from_out(out: PloBatchOut) -> BatchResult:
    """Copy a host-resident plo_batch_out into numpy arrays."""
    n = int(out.n_items)
    nc = int(out.n_cigar)

    def cp(p, dtype, count):
        if count == 0:
            return np.zeros(0, dtype=dtype)
        return np.ctypeslib.as_array(p, shape=(count,)).astype(dtype, copy=True)

    return BatchResult(
        item_seg=cp(out.item_seg, np.uint32, n),
        item_cseg=cp(out.item_cseg, np.uint32, n),
        item_status=cp(out.item_status, np.uint8, n),
        item_need_flipped=cp(out.item_need_flipped, np.uint8, n),
        item_mapq=cp(out.item_mapq, np.uint8, n),
        item_chrom_index=cp(out.item_chrom_index, np.uint32, n),
        item_ref_pos=cp(out.item_ref_pos, np.int64, n),
        item_cigar_off=cp(out.item_cigar_off, np.uint64, n),
        item_cigar_len=cp(out.item_cigar_len, np.uint32, n),
        cigar=cp(out.cigar, np.uint32, nc),
    )


def out_from_result(res: BatchResult):
    """a plo_batch_out whose pointers view the numpy arrays of a BatchResult; returns (struct, keep-alive list)"""
    o = PloBatchOut()
    keep = []

    def put(name, dt, ct):
        a = np.ascontiguousarray(getattr(res, name), dtype=dt)
        if a.size == 0:
            a = np.zeros(1, dtype=dt)
        keep.append(a)
        setattr(o, name, a.ctypes.data_as(C.POINTER(ct)))

    o.n_items = res.n_items
    put("item_seg", np.uint32, C.c_uint32)
    put("item_cseg", np.uint32, C.c_uint32)
    put("item_status", np.uint8, C.c_uint8)
    put("item_need_flipped", np.uint8, C.c_uint8)
    put("item_mapq", np.uint8, C.c_uint8)
    put("item_chrom_index", np.uint32, C.c_uint32)
    put("item_ref_pos", np.int64, C.c_int64)
    put("item_cigar_off", np.uint64, C.c_uint64)
    put("item_cigar_len", np.uint32, C.c_uint32)
    put("cigar", np.uint32, C.c_uint32)
    o.n_cigar = len(res.cigar)
    return o, keep
