"""The device reader (pipeline.run_bam_to_bam, device_input): a BAM file whose inflated stream is made in device memory and stays there.
Compressed bytes go from the file into a page-locked chunk, plo_bgzf_inflate_part_dev inflates them into a torch device buffer, and
plo_window_cut_part_dev cuts that buffer into the windows bam.BamReader.read_window would cut -- of the whole file, or of one part of it
(plo_bam_open_range's split by compressed offset; plo_part_start_dev finds a later part's first record).  A window is a device buffer of its own with its
read_rec_off (what plo_batch_build_dev and plo_records_build_dev take); only the unmapped records come down."""
import os
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


def bgzf_block_at(h: bytes, left: int):
    """BgzfIn::bgzf_block_at: (block size, ISIZE) of the BGZF block whose first bytes are `h` (a whole block, or 64 KiB), `left` bytes before
    the end of the file; None when no block stands there"""
    if left < 28 or len(h) < 28 or h[:3] != b"\x1f\x8b\x08" or not h[3] & 4:
        return None
    xlen = h[10] | (h[11] << 8)
    if 12 + xlen > left or 12 + xlen > len(h):
        return None
    bsize, x = 0, 0
    while x + 4 <= xlen:
        e = 12 + x
        slen = h[e + 2] | (h[e + 3] << 8)
        if h[e:e + 2] == b"BC" and slen == 2 and x + 6 <= xlen:
            bsize = (h[e + 4] | (h[e + 5] << 8)) + 1
        x += 4 + slen
    if bsize < 12 + xlen + 8 or bsize > left or bsize > len(h):
        return None
    return bsize, struct.unpack_from("<I", h, bsize - 4)[0]


class DeviceMemory:
    """where the reader's buffers live and what runs its calls: the GPU of the index, a stream and an engine of the reader's own"""

    def __init__(self, index: api.Index):
        self.dev = torch.device("cuda", index.device)
        self.tstream = torch.cuda.Stream(device=self.dev)
        self.eng = api.Engine(index, stream=self.tstream.cuda_stream)

    def on_stream(self):
        return torch.cuda.stream(self.tstream)

    def pinned(self, n: int) -> torch.Tensor:
        return torch.empty(n, dtype=torch.uint8, pin_memory=True)

    def empty(self, n: int) -> torch.Tensor:
        return torch.empty(n, dtype=torch.uint8, device=self.dev)

    def view(self, ptr, n: int, tdtype) -> torch.Tensor:
        return device_view(ptr, n, tdtype, self.dev)

    def synchronize(self):
        self.tstream.synchronize()

    def close(self):
        if self.eng is not None:
            self.eng.close()
            self.eng = None


class DeviceBamReader:
    """bam.BamReader's interface over a stream inflated on the device: the whole file (part None) or one part of it as plo_bam_open_range
    cuts it -- the file is cut at size x part / n_parts, a part owns the records whose first byte lies in a BGZF block that starts inside its
    stretch [lo, hi) and reads on past hi to finish the last of them.  The header and the blocks it ends in are read on the host (the ISIZE
    trailers say where the first record block starts); a part behind that block's owner finds its first block with the host's
    three-header chain, inflates start_bytes (then four times as much, from the same start: the host's schedule) and asks
    plo_part_start_dev for its first record.  plo_bgzf_inflate_part_dev says where the next part's blocks begin in the inflated bytes;
    the reader moves that position with the stream and hands it to every plo_window_cut_part_dev.  One reader per process.
    memory: tests only, a stand-in for DeviceMemory."""

    def __init__(self, path: str, index: api.Index, chunk_bytes: int = 64 << 20, stream_bytes: int = 256 << 20, max_unmapped: int = 0, max_bytes: int = 0,
                 part: Optional[int] = None, n_parts: int = 1, start_bytes: int = 4 << 20, memory=None):
        if part is not None and (int(n_parts) < 1 or not 0 <= int(part) < int(n_parts)):
            raise api.PortelloError(abi.PLO_ERR_INVALID_ARG, f"part {part} of {n_parts}")
        self.mem = memory if memory is not None else DeviceMemory(index)
        self.dev, self.eng = self.mem.dev, self.mem.eng
        self.tstream = getattr(self.mem, "tstream", None)
        self.fh = open(path, "rb", buffering=0)
        self.size = os.fstat(self.fh.fileno()).st_size
        self.max_unmapped, self.max_bytes = max_unmapped, max_bytes
        self.inflate_ms = self.cut_ms = self.part_start_ms = 0.0
        self.n_refills = self.n_recuts = self.n_start_calls = 0
        self.chunk = self.mem.pinned(max(1 << 16, int(chunk_bytes)))
        self.chunk_np = self.chunk.numpy()
        self.c_have = 0          # compressed bytes at the front of the chunk that no call consumed yet
        self.file_pos = 0        # file offset of chunk_np[0]
        self.file_done = False
        with self.mem.on_stream():
            self.buf = self.mem.empty(max(1 << 17, int(stream_bytes)))
        self.pos = self.have = 0  # the unconsumed inflated bytes are buf[pos:have]
        self.range_end = abi.NO_RANGE_END
        self.own_at = None        # where in buf the first block of the next part's stretch starts, once it has been inflated
        self.done = False         # the part's last window is out (or the part is empty)
        # the header, from the file's first blocks (zlib on the host)
        hdr, at, z = None, 0, b""
        while hdr is None:
            blk = self._block(at)
            if blk is None:
                raise api.PortelloError(abi.PLO_ERR_IO, f"{path}: the file ends inside the BAM header")
            h = os.pread(self.fh.fileno(), blk[0], at)
            xlen = h[10] | (h[11] << 8)
            z += zlib.decompress(h[12 + xlen:blk[0] - 8], -15)
            at += blk[0]
            hdr = parse_header(z)
        self.header_text, self.ref_names, self.ref_lens, self.header_bytes = hdr
        self._skip = self.header_bytes  # inflated bytes in front of the first record
        if part is not None:
            self._open_range(int(part), int(n_parts), max(36, int(start_bytes)))

    # ---- a part of the file (plo_bam_open_range, bam_host.cpp:132-212) ----
    def _block(self, off: int):
        left = self.size - off
        return bgzf_block_at(os.pread(self.fh.fileno(), min(left, 65536), off), left) if left >= 28 else None

    def _seek_block(self, frm: int) -> int:
        """BgzfIn::seek_block: the first offset >= frm from which three BGZF blocks follow each other (or blocks to the end of the file)"""
        p = frm
        while p + 28 <= self.size:
            win = os.pread(self.fh.fileno(), 1 << 16, p)
            i = win.find(b"\x1f\x8b")
            if i < 0:
                p += max(1, len(win) - 1)
                continue
            p += i
            if p + 28 > self.size:
                break
            q, ok = p, 0
            while ok < 3 and q < self.size:
                b = self._block(q)
                if b is None:
                    break
                q += b[0]
                ok += 1
            if ok == 3 or (ok > 0 and q == self.size):
                return p
            p += 1
        return self.size

    def _start_at(self, off: int, skip: int):
        self.fh.seek(off)
        self.file_pos, self.c_have, self.file_done = off, 0, off >= self.size
        self.pos = self.have = 0
        self._skip = skip

    def _open_range(self, part: int, n_parts: int, start_bytes: int):
        lo, hi = self.size * part // n_parts, self.size * (part + 1) // n_parts
        self.range_end = abi.NO_RANGE_END if part + 1 == n_parts else hi
        c = u = 0  # the blocks from the file's start until the inflated offset passes the header
        while c < self.size:
            b = self._block(c)
            if b is None:
                raise api.PortelloError(abi.PLO_ERR_IO, "not a BGZF block")
            if u + b[1] > self.header_bytes:
                break
            u += b[1]
            c += b[0]
        first_rec_block, skip = c, self.header_bytes - u
        if first_rec_block >= self.size or hi <= first_rec_block:  # no records at all, or this part lies in front of them
            self.done = True
            return
        if lo <= first_rec_block:  # the owner of the first records' block
            self._start_at(first_rec_block, skip)
            return
        blk = self._seek_block(lo)
        if blk >= self.size or blk >= hi:  # no block starts inside this part's stretch
            self.done = True
            return
        self._start_at(blk, 0)
        n_ref, want = len(self.ref_names), start_bytes
        while True:
            while self.have < want and not (self.file_done and not self.c_have):
                self._refill()
            final = self.file_done and not self.c_have
            with self.mem.on_stream():
                so = self.eng.part_start_dev(self.buf.data_ptr(), self.have, n_ref, final)
            self.part_start_ms += float(so.start_ms)
            self.n_start_calls += 1
            if int(so.kind) == abi.PART_FOUND:
                self.pos = int(so.first_off)
                return
            if final or want > (1 << 32):  # (the host buffers four times as much after "none" as well as after "need more")
                break
            want *= 4
        # no record boundary behind the part's first block: the tail of one record when little data is left, an error otherwise
        if self.have > (64 << 20) or not final:
            raise api.PortelloError(abi.PLO_ERR_DATA, "no BAM record boundary found behind the part's first BGZF block")
        self.done = True

    # ---- the compressed side ----
    def _read_file(self):
        while not self.file_done and self.c_have < self.chunk_np.size:
            n = self.fh.readinto(memoryview(self.chunk_np)[self.c_have:])
            if not n:
                self.file_done = True
                break
            self.c_have += n

    def _refill(self) -> bool:
        """more inflated bytes behind buf[pos:have] (the tail moves to the front); False when the file has nothing more to give"""
        left = self.have - self.pos
        with self.mem.on_stream():
            # room for at least one chunk's worth of new blocks; a record larger than the buffer makes it grow
            if self.buf.numel() - left < max(1 << 17, self.buf.numel() // 2):
                nb = self.mem.empty(2 * self.buf.numel())
                nb[:left].copy_(self.buf[self.pos:self.have])
                self.buf = nb
            elif self.pos:
                if left <= self.pos:
                    self.buf[:left].copy_(self.buf[self.pos:self.have])
                else:
                    self.buf[:left].copy_(self.buf[self.pos:self.have].clone())
            if self.own_at is not None:
                self.own_at = max(0, self.own_at - self.pos)
            self.pos, self.have = 0, left
            self._read_file()
            if not self.c_have:
                return False
            io = self.eng.bgzf_inflate_part_dev(self.chunk.data_ptr(), self.c_have, self.buf.data_ptr() + left, self.buf.numel() - left, self.file_pos, self.range_end)
            self.inflate_ms += float(io.inflate_ms)
            self.n_refills += 1
            used = int(io.bgzf_consumed)
            if not used:
                if self.file_done and self.c_have < 28 + 65536:
                    raise api.PortelloError(abi.PLO_ERR_IO, "truncated BGZF block at the end of the file")
                return True  # (a block that does not fit: the next call grows the buffer)
            self.chunk_np[:self.c_have - used] = self.chunk_np[used:self.c_have].copy()
            self.c_have -= used
            self.file_pos += used
            if self.own_at is None and int(io.own_bytes) < int(io.n_bytes):
                self.own_at = left + int(io.own_bytes)
            self.have = left + int(io.n_bytes)
            if self._skip:
                k = min(self._skip, self.have - self.pos)
                self.pos += k
                self._skip -= k
        return True

    # ---- windows ----
    def read_window(self, max_records: int) -> Optional[DeviceWindow]:
        """next window of at most max_records primary records, cut as bam.BamReader.read_window cuts it; None at the end of the file"""
        if self.done:
            return None
        first = True
        while True:
            final = self.file_done and not self.c_have and not self._skip
            own = abi.NO_RANGE_END if self.own_at is None else max(0, self.own_at - self.pos)
            with self.mem.on_stream():
                co = self.eng.window_cut_part_dev(self.buf.data_ptr() + self.pos, self.have - self.pos, max_records, final, own, self.max_unmapped, self.max_bytes)
            self.cut_ms += float(co.cut_ms)
            if not first:
                self.n_recuts += 1
            first = False
            if int(co.ended_by) == abi.CUT_END_OF_BYTES and not final:
                self._refill()
                continue
            break
        nr, nu, wb, ub = int(co.n_reads), int(co.n_unmapped), int(co.window_bytes), int(co.unmapped_bytes)
        if int(co.ended_by) == abi.CUT_PART_END:  # the next record is the next part's: nothing more is read
            self.done = True
        if nr == 0 and nu == 0:
            self.pos += wb
            return None
        with self.mem.on_stream():
            rec = self.mem.empty(max(16, wb))
            rec[:wb].copy_(self.buf[self.pos:self.pos + wb])
            off = self.mem.view(co.read_rec_off, nr, torch.int64).clone() if nr else torch.zeros(1, dtype=torch.int64, device=self.dev)[:0]
            unm = b""
            if ub:
                h = self.mem.pinned(ub)
                h.copy_(self.mem.view(co.unmapped, ub, torch.uint8), non_blocking=True)
            self.mem.synchronize()  # the window is complete before another thread's stream reads it
            if ub:
                unm = h.numpy().tobytes()
        self.pos += wb
        return DeviceWindow(rec, wb, off, nr, unm, nu, int(co.ended_by) in (abi.CUT_EOF, abi.CUT_PART_END), int(co.ended_by))

    def close(self):
        if self.eng is not None:
            self.mem.close()
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
