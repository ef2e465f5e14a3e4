"""tests/emu/emu_enumerate.cpp: whole batches through the emulated device code as a stand-alone program with AddressSanitizer and UBSan,
built and run the way emu_finish_lib builds and runs its program.  Every sequence, index array and batch array lives in a heap block of
its exact size there.  TEST INFRASTRUCTURE ONLY."""
import os
import struct
import subprocess

import numpy as np

from portello_amd import abi

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
_ASAN = os.path.join(_HERE, "emu", "emu_enumerate_asan")


def _sources():
    return [os.path.join(_HERE, "emu", f) for f in ("emu_enumerate.cpp", "emu_harness.cpp", "emu_batch_file.hpp", "plo_wave.hpp", "emu_inflate.hpp", "emu_finish.hpp")] + [
        os.path.join(ROOT, "portello_amd", "csrc", f) for f in ("lift_core.hpp", "lane_core.hpp", "lane_stream.hpp", "inflate.hpp", "finish_core.hpp",
                                                               "lift_types.hpp", "index_pack.hpp", "enumerate.hpp")]


def build_asan(force=False):
    srcs = _sources()
    stale = (not os.path.exists(_ASAN)) or any(os.path.getmtime(s) > os.path.getmtime(_ASAN) for s in srcs)
    if force or stale:
        subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-I" + os.path.join(_HERE, "emu"), "-o", _ASAN, srcs[0]])
    return _ASAN


def _t(a, dt) -> bytes:
    return np.ascontiguousarray(a, dtype=dt).tobytes()


def encode(index: abi.IndexData, cases, lane_max_w: int) -> bytes:
    """cases: (abi.BatchData, stages) pairs; a batch may carry an explicit item list"""
    ix = index
    parts = [struct.pack("<5I", 0x314D4E45, ix.n_contigs, ix.n_segments, len(ix.chrom_seq), len(ix.seg_cigar)),
             _t(ix.contig_len, np.int64), _t(ix.contig_seg_off, np.uint32), _t(ix.seg_chrom_index, np.uint32), _t(ix.seg_pos, np.int64),
             _t(ix.seg_is_fwd_strand, np.uint8), _t(ix.seg_mapq, np.uint8), _t(ix.seg_seq_order_start, np.int64), _t(ix.seg_seq_order_end, np.int64),
             _t(ix.seg_cigar_off, np.uint32), _t(ix.seg_cigar, np.uint32), _t(ix.chrom_len, np.int64)]
    for c, s in enumerate(ix.chrom_seq):
        assert len(s) == int(ix.chrom_len[c])
        parts.append(_t(s, np.uint8))
    for c, s in enumerate(ix.rev_contig_seq):
        parts.append(struct.pack("<I", 0 if s is None else 1))
        if s is not None:
            assert len(s) == int(ix.contig_len[c])
            parts.append(_t(s, np.uint8))
    parts.append(struct.pack("<I", len(cases)))
    for b, stages in cases:
        has_list = b.item_seg is not None
        parts += [struct.pack("<8IQ", stages, lane_max_w, b.seq_fmt, b.n_reads, b.n_segs, len(b.cigar), int(has_list), len(b.item_seg) if has_list else 0, b.seq.nbytes),
                  _t(b.read_is_reverse, np.uint8), _t(b.read_seq_len, np.uint32), _t(b.read_seq_off, np.uint64), _t(b.seq, np.uint8),
                  _t(b.seg_read, np.uint32), _t(b.seg_contig, np.uint32), _t(b.seg_pos, np.int64), _t(b.seg_is_fwd_strand, np.uint8),
                  _t(b.seg_cigar_off, np.uint32), _t(b.cigar, np.uint32)]
        if has_list:
            parts += [_t(b.item_seg, np.uint32), _t(b.item_cseg, np.uint32)]
    return b"".join(parts)


def decode(data: bytes, n_cases: int, n_modes=2):
    """-> per case [(rc, lane items, abi.BatchResult) for the lane-per-item run and for the scan formulation]; rc as emu_liftover_batch
    returns it (3: lifted, but an item has a negative rev_pos and the card refuses the batch).  (n_modes: the runs per case, one number or a
    number per case: emu_liftover_lib's program writes this format too.)"""
    at = 0

    def take(dt, n):
        nonlocal at
        a = np.frombuffer(data, dtype=dt, count=n, offset=at).copy()
        at += a.nbytes
        return a

    out = []
    for k in range(n_cases):
        modes = []
        for _m in range(n_modes if isinstance(n_modes, int) else n_modes[k]):
            rc, n, lanes = (int(x) for x in take(np.uint32, 3))
            seg, cseg = take(np.uint32, n), take(np.uint32, n)
            st, fl, mq = take(np.uint8, n), take(np.uint8, n), take(np.uint8, n)
            ch, pos, clen = take(np.uint32, n), take(np.int64, n), take(np.uint32, n)
            total = int(take(np.uint64, 1)[0])
            cig = take(np.uint32, total)
            off = (np.cumsum(clen, dtype=np.uint64) - clen).astype(np.uint64)
            modes.append((rc, lanes, abi.BatchResult(seg, cseg, st, fl, mq, ch, pos, off, clen, cig)))
        out.append(modes)
    assert at == len(data)
    return out


def run_asan(index, cases, tmp_dir, lane_max_w=192, name="enum"):
    """-> (exit status, stderr text, decoded results or None); the program runs in the environment as it stands"""
    exe = build_asan()
    src, dst = os.path.join(str(tmp_dir), name + ".in"), os.path.join(str(tmp_dir), name + ".out")
    with open(src, "wb") as fh:
        fh.write(encode(index, cases, lane_max_w))
    p = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=900)
    res = None
    if p.returncode == 0:
        with open(dst, "rb") as fh:
            res = decode(fh.read(), len(cases))
    return p.returncode, p.stderr, res
