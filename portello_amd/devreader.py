"""The device reader (pipeline.run_bam_to_bam, device_input): a BAM file whose inflated stream is made in device memory and stays there.
Compressed bytes go from the file into a page-locked chunk, plo_bgzf_inflate_dev inflates them into a torch device buffer, and
plo_window_cut_dev cuts that buffer into the windows bam.BamReader.read_window would cut.  A window is a device buffer of its own with its
read_rec_off (what plo_batch_build_dev and plo_records_build_dev take); only the unmapped records come down."""
import struct
import zlib
from typing import Optional, Tuple

import torch

from . import abi, api
from .gather import device_view


class DeviceWindow:
    """a window cut on the device: what devbatch.DeviceBuiltWindow needs (records, read_rec_off, n_reads) and what the writer asks a
    bam.Window for (unmapped_bytes, eof, close)"""

    def __init__(self, records: torch.Tensor, records_bytes: int, read_rec_off: torch.Tensor, n_reads: int, unmapped: bytes, n_unmapped: int, eof: bool,
                 ended_by: int):
        self.records, self.records_bytes, self.read_rec_off, self.n_reads = records, records_bytes, read_rec_off, n_reads
        self._unmapped, self._n_unmapped, self.eof, self.ended_by = unmapped, n_unmapped, eof, ended_by

    @property
    def n_records(self) -> int:
        return self.n_reads

    def unmapped_bytes(self) -> Tuple[bytes, int]:
        return self._unmapped, self._n_unmapped

    def close(self):
        self.records = self.read_rec_off = None


def parse_header(inflated: bytes):
    """(header text, reference names, reference lengths, the header's inflated length) from the first inflated bytes of a BAM file; None
    when they end inside the header"""
    if len(inflated) < 12:
        return None
    if inflated[:4] != b"BAM\x01":
        raise api.PortelloError(abi.PLO_ERR_IO, "not a BAM file")
    l_text = struct.unpack_from("<I", inflated, 4)[0]
    at = 8 + l_text
    if len(inflated) < at + 4:
        return None
    text = inflated[8:at].split(b"\0")[0].decode(errors="replace")
    n_ref = struct.unpack_from("<I", inflated, at)[0]
    at += 4
    names, lens = [], []
    for _ in range(n_ref):
        if len(inflated) < at + 4:
            return None
        l_name = struct.unpack_from("<I", inflated, at)[0]
        if len(inflated) < at + 4 + l_name + 4:
            return None
        names.append(inflated[at + 4:at + 4 + l_name].split(b"\0")[0].decode())
        lens.append(struct.unpack_from("<I", inflated, at + 4 + l_name)[0])
        at += 8 + l_name
    return text, names, lens, at


class DeviceBamReader:
    """bam.BamReader's interface over a stream inflated on the device.  The whole file, one reader: parts of a file (plo_bam_open_range)
    stay on the host reader."""

    def __init__(self, path: str, index: api.Index, chunk_bytes: int = 64 << 20, stream_bytes: int = 256 << 20, max_unmapped: int = 0, max_bytes: int = 0):
        self.dev = torch.device("cuda", index.device)
        self.tstream = torch.cuda.Stream(device=self.dev)
        self.eng = api.Engine(index, stream=self.tstream.cuda_stream)
        self.fh = open(path, "rb", buffering=0)
        self.max_unmapped, self.max_bytes = max_unmapped, max_bytes
        self.inflate_ms = self.cut_ms = 0.0
        self.n_refills = self.n_recuts = 0
        self.chunk = torch.empty(max(1 << 16, int(chunk_bytes)), dtype=torch.uint8, pin_memory=True)
        self.chunk_np = self.chunk.numpy()
        self.c_have = 0          # compressed bytes at the front of the chunk that no call consumed yet
        self.file_done = False
        with torch.cuda.stream(self.tstream):
            self.buf = torch.empty(max(1 << 17, int(stream_bytes)), dtype=torch.uint8, device=self.dev)
        self.pos = self.have = 0  # the unconsumed inflated bytes are buf[pos:have]
        # the header, from the first inflated bytes (zlib on the host over the first blocks: they are in the chunk anyway)
        self._read_file()
        hdr, at, z = None, 0, b""
        while hdr is None:
            blk = self._host_block(at)
            if blk is None:
                raise api.PortelloError(abi.PLO_ERR_IO, f"{path}: the file ends inside the BAM header")
            z += blk[0]
            at += blk[1]
            hdr = parse_header(z)
        self.header_text, self.ref_names, self.ref_lens, self.header_bytes = hdr
        self._skip = self.header_bytes  # inflated bytes in front of the first record

    # ---- the compressed side ----
    def _read_file(self):
        while not self.file_done and self.c_have < self.chunk_np.size:
            n = self.fh.readinto(memoryview(self.chunk_np)[self.c_have:])
            if not n:
                self.file_done = True
                break
            self.c_have += n

    def _host_block(self, at: int):
        """(inflated bytes, block size) of the BGZF block at chunk offset `at`, for the header only"""
        b = self.chunk_np
        if self.c_have - at < 28 or bytes(b[at:at + 4]) != b"\x1f\x8b\x08\x04":
            return None
        xlen = int(b[at + 10]) | (int(b[at + 11]) << 8)
        bsize, x = 0, 0
        while x + 4 <= xlen:
            e = at + 12 + x
            slen = int(b[e + 2]) | (int(b[e + 3]) << 8)
            if b[e] == 66 and b[e + 1] == 67 and slen == 2:
                bsize = (int(b[e + 4]) | (int(b[e + 5]) << 8)) + 1
            x += 4 + slen
        if bsize < 12 + xlen + 8 or bsize > self.c_have - at:
            return None
        return zlib.decompress(bytes(b[at + 12 + xlen:at + bsize - 8]), -15), bsize

    def _refill(self) -> bool:
        """more inflated bytes behind buf[pos:have] (the tail moves to the front); False when the file has nothing more to give"""
        left = self.have - self.pos
        with torch.cuda.stream(self.tstream):
            # room for at least one chunk's worth of new blocks; a record larger than the buffer makes it grow
            if self.buf.numel() - left < max(1 << 17, self.buf.numel() // 2):
                nb = torch.empty(2 * self.buf.numel(), dtype=torch.uint8, device=self.dev)
                nb[:left].copy_(self.buf[self.pos:self.have])
                self.buf = nb
            elif self.pos:
                if left <= self.pos:
                    self.buf[:left].copy_(self.buf[self.pos:self.have])
                else:
                    self.buf[:left].copy_(self.buf[self.pos:self.have].clone())
            self.pos, self.have = 0, left
            self._read_file()
            if not self.c_have:
                return False
            io = self.eng.bgzf_inflate_dev(self.chunk.data_ptr(), self.c_have, self.buf.data_ptr() + left, self.buf.numel() - left)
            self.inflate_ms += float(io.inflate_ms)
            self.n_refills += 1
            used = int(io.bgzf_consumed)
            if not used:
                if self.file_done and self.c_have < 28 + 65536:
                    raise api.PortelloError(abi.PLO_ERR_IO, "truncated BGZF block at the end of the file")
                return True  # (a block that does not fit: the next call grows the buffer)
            self.chunk_np[:self.c_have - used] = self.chunk_np[used:self.c_have].copy()
            self.c_have -= used
            self.have = left + int(io.n_bytes)
            if self._skip:
                k = min(self._skip, self.have - self.pos)
                self.pos += k
                self._skip -= k
        return True

    # ---- windows ----
    def read_window(self, max_records: int) -> Optional[DeviceWindow]:
        """next window of at most max_records primary records, cut as bam.BamReader.read_window cuts it; None at the end of the file"""
        first = True
        while True:
            final = self.file_done and not self.c_have and not self._skip
            with torch.cuda.stream(self.tstream):
                co = self.eng.window_cut_dev(self.buf.data_ptr() + self.pos, self.have - self.pos, max_records, final, self.max_unmapped, self.max_bytes)
            self.cut_ms += float(co.cut_ms)
            if not first:
                self.n_recuts += 1
            first = False
            if int(co.ended_by) == abi.CUT_END_OF_BYTES and not final:
                self._refill()
                continue
            break
        nr, nu, wb, ub = int(co.n_reads), int(co.n_unmapped), int(co.window_bytes), int(co.unmapped_bytes)
        if nr == 0 and nu == 0:
            self.pos += wb
            return None
        with torch.cuda.stream(self.tstream):
            rec = torch.empty(max(16, wb), dtype=torch.uint8, device=self.dev)
            rec[:wb].copy_(self.buf[self.pos:self.pos + wb])
            off = device_view(co.read_rec_off, nr, torch.int64, self.dev).clone() if nr else torch.zeros(1, dtype=torch.int64, device=self.dev)[:0]
            unm = b""
            if ub:
                h = torch.empty(ub, dtype=torch.uint8, pin_memory=True)
                h.copy_(device_view(co.unmapped, ub, torch.uint8, self.dev), non_blocking=True)
            self.tstream.synchronize()  # the window is complete before another thread's stream reads it
            if ub:
                unm = h.numpy().tobytes()
        self.pos += wb
        return DeviceWindow(rec, wb, off, nr, unm, nu, int(co.ended_by) == abi.CUT_EOF, int(co.ended_by))

    def close(self):
        if self.eng is not None:
            self.eng.close()
            self.eng = None
        if self.fh is not None:
            self.fh.close()
            self.fh = None
        self.buf = self.chunk = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
