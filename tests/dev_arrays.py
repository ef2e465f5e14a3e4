"""A batch in device memory for the tests that call the device entry points directly.  TEST INFRASTRUCTURE ONLY."""
import ctypes as C

import numpy as np

from portello_amd import abi

TAIL = 64  # spare elements behind what a descriptor declares


class DevArrays:
    """a batch in device memory, every array with TAIL spare elements behind its declared extent"""

    def __init__(self, b: abi.BatchData):
        import torch

        def up(a, dt):
            a = np.ascontiguousarray(a)
            t = torch.zeros(len(a) + TAIL, dtype=dt, device="cuda")
            if len(a):
                t[:len(a)] = torch.from_numpy(a.view({1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize])).to("cuda")
            return t

        self.t = dict(read_is_reverse=up(b.read_is_reverse, torch.uint8), read_seq_len=up(b.read_seq_len, torch.int32), read_seq_off=up(b.read_seq_off, torch.int64),
                      seq=up(b.seq, torch.uint8), seg_read=up(b.seg_read, torch.int32), seg_contig=up(b.seg_contig, torch.int32), seg_pos=up(b.seg_pos, torch.int64),
                      seg_is_fwd_strand=up(b.seg_is_fwd_strand, torch.uint8), seg_cigar_off=up(b.seg_cigar_off, torch.int32), cigar=up(b.cigar, torch.int32))
        if b.item_seg is not None:
            self.t["item_seg"], self.t["item_cseg"] = up(b.item_seg, torch.int32), up(b.item_cseg, torch.int32)
        torch.cuda.synchronize()
        p = lambda name, ct: C.cast(C.c_void_p(self.t[name].data_ptr()), C.POINTER(ct))
        d = abi.PloBatchIn()
        d.n_reads, d.n_segs, d.seq_bytes, d.seq_fmt = b.n_reads, b.n_segs, b.seq.nbytes, b.seq_fmt
        d.read_is_reverse, d.read_seq_len, d.read_seq_off, d.seq = p("read_is_reverse", C.c_uint8), p("read_seq_len", C.c_uint32), p("read_seq_off", C.c_uint64), p("seq", C.c_uint8)
        d.seg_read, d.seg_contig, d.seg_pos = p("seg_read", C.c_uint32), p("seg_contig", C.c_uint32), p("seg_pos", C.c_int64)
        d.seg_is_fwd_strand, d.seg_cigar_off, d.cigar = p("seg_is_fwd_strand", C.c_uint8), p("seg_cigar_off", C.c_uint32), p("cigar", C.c_uint32)
        if b.item_seg is not None:
            d.n_items, d.item_seg, d.item_cseg = len(b.item_seg), p("item_seg", C.c_uint32), p("item_cseg", C.c_uint32)
        self.desc = d
