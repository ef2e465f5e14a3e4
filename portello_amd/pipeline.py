"""BAM in -> lifted BAM out: the host-side mirror of the reference's phase 2 driver (scan_and_remap_reads,
src/read_alignment_scanner.rs:566-661) on top of the C ABI.

The reference spawns one rayon task per <= 20 Mb contig window; every task reads its records, lifts them one at a time and
writes through a shared, mutex-protected writer.  Here a *reader* thread decodes windows of primary records and builds
their batches (plo_bam_read_window + plo_bam_window_batch), `n_workers` *lift* threads -- each with its own plo_ctx and HIP
stream, the arrangement of INTEGRATION.md -- run plo_liftover_batch (page-locked H2D, kernels, D2H) and assemble the
output records (plo_records_build), and a *writer* thread emits them (plo_bam_write; BGZF level 0 = the reference's
stdout mode).  The three stages overlap; ctypes releases the GIL inside every native call.  Unmapped input records are
passed through to the "unassembled" writer (scan_unmapped_reads, :537-559).
"""
from __future__ import annotations

import os
import queue
import threading
import time
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

from . import abi, api, bam


def effective_cpus() -> int:
    """host cores this process can actually use: the smallest of the CPU count, the affinity mask and the cgroup CPU quota"""
    import os

    n = os.cpu_count() or 1
    try:
        n = min(n, len(os.sched_getaffinity(0)))
    except (AttributeError, OSError):
        pass
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    n = min(n, max(1, int(int(txt[0]) / int(txt[1]) + 0.5)))
            else:
                q = int(txt[0])
                per = int(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
                if q > 0:
                    n = min(n, max(1, int(q / per + 0.5)))
            break
        except (OSError, ValueError, IndexError):
            continue
    return n


@dataclass
class PipelineStats:
    reads: int = 0
    windows: int = 0
    records_out: int = 0
    lifted: int = 0
    unmapped_copies: int = 0
    unmapped_passed_through: int = 0
    bytes_out: int = 0
    seconds: float = 0.0
    read_s: float = 0.0      # BGZF inflate + record walk (reader thread busy time)
    batch_s: float = 0.0     # batch construction (batcher thread busy time)
    lift_s: float = 0.0      # plo_liftover_batch, summed over workers
    build_s: float = 0.0     # plo_records_build, summed over workers
    write_s: float = 0.0     # BGZF output (writer thread busy time)
    device_ms: float = 0.0   # HIP-event time of the lift calls
    bgzf_device_ms: float = 0.0  # device_bgzf: HIP-event time of plo_bgzf_compress_dev (deflate / stored framing, scan, pack)
    out_file_bytes: int = 0      # size of the closed output file(s) of the lifted records (header and EOF blocks included)
    records_device_ms: float = 0.0  # device_records: HIP-event time of plo_records_build_dev (plan, scan, emit); build_s then holds only the host time left
    batch_device_ms: float = 0.0  # device_batch: HIP-event time of plo_batch_build_dev (label table, plan, scans, emit); batch_s then holds only win.raw()
    inflate_device_ms: float = 0.0  # device_input: HIP-event time of plo_bgzf_inflate_dev (upload, inflate, CRC)
    cut_device_ms: float = 0.0      # device_input: HIP-event time of plo_window_cut_dev (guess, walk, resolve, scans, find, emit)
    part_start_device_ms: float = 0.0  # device_input with part / n_parts: HIP-event time of plo_part_start_dev (the part's first record)
    nm_device_ms: float = 0.0  # emit_nm: HIP-event time of plo_nm_dev (NM:i of the lifted records)
    md_device_ms: float = 0.0  # emit_md: HIP-event time of plo_md_dev (MD:Z of the lifted records: count, scan, emit)
    eqx_device_ms: float = 0.0  # emit_eqx: HIP-event time of plo_eqx_dev (= / X CIGARs of the lifted records: count, scan, emit)
    index_device_ms: float = 0.0  # index_runs: HIP-event time of plo_records_index_dev (a wave per record of the sorted buffer)
    index_paths: List[str] = field(default_factory=list)  # index_runs: <run>.bai of every run of out_paths, in the same order
    merge_plan_device_ms: float = 0.0  # run_windows != 1: HIP-event time of plo_runs_merge_plan_dev (check + keys, rank rounds, offsets, chunk table)
    merge_emit_device_ms: float = 0.0  # run_windows != 1: HIP-event time of plo_runs_merge_emit_dev, summed over the chunks
    run_groups: List[int] = field(default_factory=list)  # sorted_runs: the windows with records in every written run, in out_paths order (all 1 with run_windows=1)
    depth_device_ms: float = 0.0  # depth_out: HIP-event time of plo_depth_add_dev over the windows, plus the finish, the windows and the runs
    depth_paths: List[str] = field(default_factory=list)  # depth_out: <prefix>.per-base.bed and <prefix>.regions.bed
    pileup_device_ms: float = 0.0  # pileup_out: HIP-event time of plo_pileup_add_dev over the windows and of the sites call (without depth_out: and of the depth calls made for it)
    pileup_paths: List[str] = field(default_factory=list)  # pileup_out: <prefix>.sites.tsv
    sort_device_ms: float = 0.0  # sorted_runs: HIP-event time of plo_records_sort_dev (check + keys + tile sort, merges, offsets, permuted copy)
    finish_device_ms: float = 0.0  # device_finish: HIP-event time of the finishing, reverse-complement and SA-text kernels
    stage_done_s: dict = field(default_factory=dict)  # when each stage's thread ended, and the closes behind them (seconds after the start)
    lift_detail_s: dict = field(default_factory=dict)  # device_finish: the lift stage by step (host clock; the steps that wait for the device carry its time)
    out_paths: List[str] = field(default_factory=list)  # the output file, the shards (out_shards > 1) or the runs in name order (sorted_runs)
    errors: List[str] = field(default_factory=list)


def run_bam_to_bam(in_path: str, out_path: str, index: api.Index, index_data: abi.IndexData, contig_names: Sequence[str],
                   ref_names: Sequence[str], ref_lens: Sequence[int], window_reads: int = 50_000, n_workers: int = 2,
                   io_threads: int = 16, level: int = 0, unassembled_path: Optional[str] = None, is_target_region: bool = False,
                   cmdline: str = "", sparse_margin: Optional[int] = 32, device_inflate: Optional[bool] = True,
                   device_finish: bool = False, read_threads: Optional[int] = None, build_threads: Optional[int] = None,
                   write_threads: Optional[int] = None, ramp: bool = True, part: Optional[int] = None, n_parts: int = 1,
                   out_shards: int = 1, n_readers: int = 1, device_records: bool = False, device_bgzf: bool = False, device_batch: bool = False,
                   device_input: bool = False, emit_nm: bool = False, emit_md: bool = False, sorted_runs: bool = False,
                   index_runs: bool = False, emit_eqx: bool = False, run_windows: int = 1, run_budget_bytes: Optional[int] = None,
                   run_chunk_bytes: int = 1 << 30, depth_out: Optional[str] = None, depth_window: int = 500, depth_deletions: bool = False,
                   pileup_out: Optional[str] = None, pileup_min_count: int = 2, pileup_min_frac: Sequence[int] = (1, 5),
                   pileup_regions: Optional[Sequence[Sequence[int]]] = None) -> PipelineStats:  # noqa: E501
    """pileup_out (default None; a path prefix; needs device_records=True): the allele pileup of the output records against the index's
    chrom_seq, taken while the records lie on the device.  The process holds ONE pileup object (pileup.DevicePileup over ref_lens, or over
    pileup_regions = [(ref_id, beg, end)], at most one a chromosome: 32 bytes a base), made by the first lift worker; every worker adds its
    window's plo_records_out right behind plo_records_build_dev (plo_pileup_add_dev: integer atomics, so neither the order of the windows
    nor the number of workers changes a value).  When the workers are joined the main thread's context lists the candidate sites -- a base
    whose largest counter among A C G T DEL INS is at least pileup_min_count and at least pileup_min_frac = (num, den) of the depth -- and
    writes <prefix>.sites.tsv (pileup.write_sites).  The depth is the run's depth object; without depth_out one is made for the purpose and
    no beds are written.  PipelineStats: pileup_device_ms, pileup_paths.  With pileup_out=None every byte of every output is what it was.
    depth_out (default None; a path prefix; needs device_records=True): the depth of the output records is taken while they lie on the
    device, so that no mosdepth or `samtools depth` pass has to read the written file back.  The process holds ONE depth object
    (depth.DeviceDepth over ref_lens: 4 bytes a reference base); every lift worker adds its window's plo_records_out right behind
    plo_records_build_dev (plo_depth_add_dev on the worker's own context and stream: the adds are integer atomics, so neither the order of
    the windows nor the number of workers changes a value).  When the workers are joined the differences become depths
    (plo_depth_finish_dev) and two files are written: <prefix>.per-base.bed (chrom, beg, end, depth: maximal runs of equal depth, zero
    ones too) and <prefix>.regions.bed (chrom, beg, end, mean over windows of depth_window bases, two decimals, round-half-even).  The
    counting rule is mosdepth's and samtools depth's flag mask 0x704 over the records' real CIGARs; depth_deletions=True lets D cover its
    bases (mosdepth, `samtools depth -J`), False (default) is `samtools depth`.  PipelineStats: depth_device_ms, depth_paths.  Combines
    with every other output switch (the unsorted records are added, so sorted_runs makes no difference); with depth_out=None every byte
    of every output is what it was.
    run_windows (default 1; anything else needs sorted_runs=True): how many windows leave as one run.  1: every window is a run of its
    own, as below -- same file names, same bytes, no new allocation.  K > 1: the windows [mK, (m + 1)K) of a reader, by the reader's window
    sequence number and not by arrival at the lift workers, form group m.  Every worker keeps its sorted window on the device
    (devbatch.RetainedWindow: a device-to-device copy of plo_sort_out) and hands it to ONE merger thread with a context of its own on the
    same device; the merger plans the group's merge (plo_runs_merge_plan_dev: the order of plo_records_sort_dev over the windows'
    concatenation, which is the order of bam.merge_runs over the windows' runs), and for every chunk of at most run_chunk_bytes it emits
    (plo_runs_merge_emit_dev), indexes with index_runs, compresses on the device with device_bgzf or else downloads for the host writer,
    and writes ONE run <stem>.r<reader:02d>m<group:06d><ext> (plus .bai), then frees the group.  0: all windows of a reader are one
    group; with n_readers == 1 and one group that single run is written to `out_path` itself (and out_path + ".bai"): a sorted, indexed BAM
    with nothing left to merge.  run_budget_bytes: a reader's group is closed early, in window order, when the next window would take
    its retained bytes past the reader's share of the budget (run_budget_bytes // n_readers), so a group's composition is a function of
    the windows' sizes alone; a worker waits while the groups that are being written hold the reader's share, and a window larger than
    it forms a group alone.  Default: half of the device's free memory when the pipeline starts -- a policy, not a measurement: the
    workers' own buffers, the merger's chunk and the allocator's cache take their share of the other half.  Groups closed early are
    numbered on (m counts the groups of the reader).  A window without an output record takes its place in its group and is not
    counted.  PipelineStats: merge_plan_device_ms, merge_emit_device_ms, run_groups (the windows with records of every written run), out_paths / index_paths in name order, which stays the tie order of bam.merge_runs.  Combines with
    emit_nm, emit_md, emit_eqx, device_bgzf, index_runs, device_batch and device_input.
    emit_eqx (default off; needs device_records=True): every lifted record leaves with a pbmm2-style CIGAR, every M op replaced by its
    maximal runs of '=' (the read's base matches the reference chromosome of the index, by emit_nm's pair rule) and 'X' (it does not);
    every other op stays (plo_eqx_dev between the finishing and plo_records_build_dev, which then writes these ops, by bam_write1's rule
    in CG:B,I where there are more than 65535 of them).  Positions, bins, reference ends and SA:Z, whose CIGARs stay in M, do not
    change, nor do the unmapped copies.  Combines with emit_nm, emit_md, device_bgzf, sorted_runs and index_runs.  Off, every byte is
    what it was.
    index_runs (default off; needs sorted_runs=True): every run leaves with its BAM index <run>.bai, so that a caller or a viewer opens
    it as it is.  plo_records_index_dev runs behind plo_records_sort_dev on the sorted buffer (24 bytes a record: where it stands, its
    reference, [beg, end) from its CIGAR, the unmapped flag, its bin); the entries come down with the window's bytes -- or, with
    device_bgzf, with its blocks: the host never holds an uncompressed record -- and the run's writer, which notes where every BGZF block
    starts, writes the index when it closes.  PipelineStats.index_paths lists them beside out_paths; bam.merge_runs(..., index=True)
    indexes the merged file.  Off, every byte and every file name is what it was.
    sorted_runs (default off; needs device_records=True, out_shards must be 1): every window's records are put in coordinate order on
    the device (plo_records_sort_dev behind plo_records_build_dev: reference in header order, position, forward before reverse, unmapped
    copies last, ties in input order) and leave as a run file of their own, a complete BAM with an SO:coordinate header, named
    <stem>.r<reader:02d>w<window:06d><ext> after the window's sequence number at its reader -- `out_path` itself is not written.
    PipelineStats.out_paths lists the runs in name order, which is the tie order of bam.merge_runs(st.out_paths, final_path) (or samtools
    merge); the pipeline neither merges nor deletes.  A run of the pipeline without an output record writes one header-only run.  Works
    with emit_nm, emit_md, device_batch, device_input, device_bgzf and part / n_parts; the unassembled file is untouched.  Off, every byte
    and every file name is what it was.
    emit_md (default off; needs device_records=True): every lifted record leaves with MD:Z, calmd's text against the reference
    chromosomes of the index (plo_md_dev between the finishing and plo_records_build_dev, which then writes the field behind ZM:C, behind
    NM:i with emit_nm, and cuts the MD the source record carried); the unmapped copies get none and keep theirs.  Combines with emit_nm:
    both on, the output needs no samtools calmd pass.  Off, every byte is what it was.
    emit_nm (default off; needs device_records=True): every lifted record leaves with NM:i, calmd's edit distance against the
    reference chromosomes of the index (plo_nm_dev between the finishing and plo_records_build_dev, which then writes the field behind ZM:C);
    the unmapped copies get none.  Works with device_batch, device_input, device_bgzf and part / n_parts.  Off, every byte is what it was.
    device_input (default off; needs device_batch=True and so device_records=True; n_readers must be 1): the input's inflated
    stream is made in device memory and stays there (devreader.DeviceBamReader: plo_bgzf_inflate_dev into a device buffer,
    plo_window_cut_dev for the record walk and the window cut) -- a window reaches plo_batch_build_dev as a device buffer with its
    read_rec_off, no inflated byte of a primary read comes down or goes up again; only the unmapped records are downloaded for the
    pass-through.  Same windows as the host reader's (tests/test_window_cut_dev.py).  With part / n_parts the device reader takes this
    process's part of the file as plo_bam_open_range cuts it (plo_part_start_dev finds the part's first record, plo_bgzf_inflate_part_dev
    and plo_window_cut_part_dev end it where the next part's blocks begin: tests/test_part_dev.py).  One device reader per process is the
    design -- a rank is a process with a GPU and a part -- so n_readers > 1 stays on the host reader.
    device_batch (default off; needs device_records=True): the window's liftover batch is built on the device too -- the batcher thread
    only asks the window for its raw stretch (bam.Window.raw), the records and read_rec_off go up, and plo_batch_build_dev (split segments,
    SA parse, sort, label look-up, CIGAR gather) runs on the worker's stream in front of plo_liftover_batch_dev: no segment, CIGAR or
    per-read array crosses the bus and the host parses no record.  Input the host batcher refuses (PLO_ERR_DATA) aborts the run as it does
    there.  Same arrays as the host batcher's (tests/test_batch_dev.py).
    device_bgzf (default off; needs device_records=True): the window's record bytes are framed as BGZF blocks on the device too
    (plo_bgzf_compress_dev behind plo_records_build_dev) and only the finished blocks come down; the writer appends them as they are
    (plo_bam_write_blocks: no CRC pass, no deflate on the host).  `level` then selects between the device's two forms: level == 0 is
    stored framing, byte for byte the host writer's; level >= 1 is the device's ONE deflate level (LZ77 + dynamic Huffman codes, about
    zlib level 1) -- levels 2-9 do not exist on the device and mean the same as 1.  Every window ends its last block, as the host writer
    does only at the end of the file, so a file of several windows has a few more (short) blocks than the host-framed one.  The unmapped
    pass-through and the unassembled file stay on the host writer at `level`.
    device_records (default off; implies device_finish): the output records are assembled on the device too -- the window's records
    go up ONCE as they stand (bam.Window.batch_raw: bases and qualities are views into them), lift -> compact -> finish -> SA ->
    plo_records_build_dev run on the worker's stream, ONE copy brings the record bytes down and the writer takes them: the host touches
    no record byte between the reader and plo_bam_write.  Same bytes as the other two modes (tests/test_records_dev.py).
    device_finish: the records are finished on the device -- the window's batch goes up with all its bases and qualities
    (sparse_margin is ignored), plo_finish_batch_dev (flags, bin, primary record, reverse_alignment_seq_and_qual) and
    plo_sa_segments_dev (SA text) run behind the lift kernels, their results come back and plo_records_build_finished only copies
    them into place.  Same bytes as the host finishing (tests/test_bam.py).
    sparse_margin: the windows' read bases go to the device as PLO_SEQ_BAM4_SPARSE (granules within that many bases of an indel;
    the complete bases stay in the window's records for the engine's second look); None = dense bases.  device_inflate: the BGZF
    blocks of the input are inflated on the GPU (leaves the host cores to record assembly and output; falls back to the host without
    a device), None = as the environment says.
    part / n_parts: this process's share of the input (plo_bam_open_range: a split by compressed offset) -- with several GPUs every rank
    runs the pipeline over its part and writes its own output shard (the reference's output order is unspecified: the shards'
    concatenation is a valid result)
    n_readers > 1: the input (or this process's part of it) is cut again into that many parts by compressed offset (plo_bam_open_range),
    every part with a reader and a batcher thread of its own feeding the same lift workers: with the output in shards the reader -- one
    chain of refills: stage, inflate on the device, copy back, walk -- is what the run waits for (390 k reads/s alone on the bench sample).
    out_shards > 1: the lifted records go into that many files (`out_path` with .0, .1, ... in front of its extension), one writer thread
    each, a window's records to whichever writer is free -- the reference's output order is unspecified (docs/user_guide.md:227-230), so the
    shards' union is the output (`samtools cat` joins them).  Buffered writes into ONE file are serialised by its inode lock (9.5 GB/s
    from any number of threads on the GPU box, 61-126 GB/s into a file per thread: tools/write_bench.cpp), which is what bounds the
    one-file pipeline at ~320 k reads/s of 15 kb HiFi records."""
    # threads inside the stages (inflate / batch construction, record assembly per worker, BGZF output).  The stages run at the same
    # time: half of io_threads each by default (tools/bench_e2e_threads.py on the 16-core GPU box, best of three runs: 80.6-81.4 k reads/s
    # with 8 / 4-8 / 6-8 threads against 77.1 k with 16 each; the input and output stages are bound by the page cache either way)
    run_windows = int(run_windows)
    if depth_out is not None and not device_records:
        raise ValueError("depth_out adds the records plo_records_build_dev leaves on the device: it needs device_records=True")
    if pileup_out is not None and not device_records:
        raise ValueError("pileup_out adds the records plo_records_build_dev leaves on the device: it needs device_records=True")
    if pileup_out is not None and (int(pileup_min_count) < 1 or len(pileup_min_frac) != 2 or (int(pileup_min_frac[0]) != 0 and int(pileup_min_frac[1]) == 0)):
        raise ValueError("pileup_min_count must be 1 or more and pileup_min_frac a pair (num, den) with den != 0 unless num == 0")
    if depth_out is not None and int(depth_window) < 1:
        raise ValueError("depth_window is the size of the windows of <prefix>.regions.bed in bases: it must be 1 or more")
    if run_windows != 1 and not sorted_runs:
        raise ValueError("run_windows merges the coordinate-sorted windows of a group into one run: it needs sorted_runs=True")
    if run_windows < 0:
        raise ValueError("run_windows is 0 (all windows of a reader), 1 (a run per window) or the number of windows of a run")
    if run_windows != 1 and int(run_chunk_bytes) <= 0:
        raise ValueError("run_chunk_bytes is the size of the chunks a merged run is emitted in: it must be above 0")
    if run_windows != 1 and run_budget_bytes is not None and int(run_budget_bytes) <= 0:
        raise ValueError("run_budget_bytes is the device memory the retained windows may hold: it must be above 0 (None: half of the free memory)")
    if index_runs and not sorted_runs:
        raise ValueError("index_runs writes the BAM index of every coordinate-sorted run: it needs sorted_runs=True")
    if sorted_runs and not device_records:
        raise ValueError("sorted_runs sorts the records plo_records_build_dev leaves on the device: it needs device_records=True")
    if sorted_runs and int(out_shards) > 1:
        raise ValueError("sorted_runs writes a run file per window: out_shards > 1 has no meaning with it")
    if emit_nm and not device_records:
        raise ValueError("emit_nm counts NM on the device, from the bases and CIGARs plo_records_build_dev writes: it needs device_records=True")
    if emit_eqx and not device_records:
        raise ValueError("emit_eqx writes = / X CIGARs on the device, into the records plo_records_build_dev writes: it needs device_records=True")
    if emit_md and not device_records:
        raise ValueError("emit_md writes MD on the device, from the bases and CIGARs plo_records_build_dev writes: it needs device_records=True")
    if device_input and not device_batch:
        raise ValueError("device_input hands plo_batch_build_dev windows that exist in device memory only: it needs device_batch=True (and device_records=True)")
    if device_input and int(n_readers) != 1:
        raise ValueError("device_input reads the file (or this process's part of it) with one reader: n_readers > 1 stays on the host reader")
    if device_batch and not device_records:
        raise ValueError("device_batch builds the batch from the records device_records uploads as they stand: it needs device_records=True")
    if device_bgzf and not device_records:
        raise ValueError("device_bgzf compresses the records plo_records_build_dev leaves on the device: it needs device_records=True")
    device_finish = bool(device_finish or device_records)
    half = max(2, io_threads // 2)
    read_threads = read_threads or half
    build_threads = build_threads or half
    write_threads = write_threads or half
    st = PipelineStats()
    ixd = index_data.to_desc()
    n_readers = max(1, int(n_readers))
    dev_arg = (index.device if device_inflate else (-1 if device_inflate is False else None))
    if device_input:
        from . import devreader

        rds = [devreader.DeviceBamReader(in_path, index, part=part, n_parts=n_parts)]
    elif n_readers == 1:
        rds = [bam.BamReader(in_path, read_threads, device_inflate=dev_arg, part=part, n_parts=n_parts)]
    else:
        p0, np0 = (part or 0), max(1, n_parts)
        rds = [bam.BamReader(in_path, max(1, read_threads // n_readers), device_inflate=dev_arg, part=p0 * n_readers + i, n_parts=np0 * n_readers) for i in range(n_readers)]
    rd = rds[0]
    if list(rd.ref_names) != list(contig_names):
        raise ValueError("the read->contig BAM's @SQ list differs from the contig names of the index")
    out_shards = max(1, int(out_shards))
    if out_shards == 1:
        out_paths = [out_path]
    else:
        stem, ext = os.path.splitext(out_path)
        out_paths = [f"{stem}.{k}{ext}" for k in range(out_shards)]
    st.out_paths = list(out_paths)
    hdr_out = bam.output_header(ref_names, ref_lens, cmdline=cmdline, sort_order="coordinate" if sorted_runs else "unsorted")
    if sorted_runs:  # a writer per run, opened when the window's records arrive
        run_stem, run_ext = os.path.splitext(out_path)
        out_paths, wrs = [], []
    else:
        wrs = [bam.BamWriter(p_, hdr_out, ref_names, ref_lens, level=level, n_threads=max(1, write_threads // out_shards)) for p_ in out_paths]
    un = None
    if unassembled_path:
        un = bam.BamWriter(unassembled_path, bam.output_header(ref_names, ref_lens, cmdline=cmdline), ref_names, ref_lens, level=level,
                           n_threads=max(1, write_threads // 2))
    q_in: "queue.Queue" = queue.Queue(maxsize=2 * n_workers)
    q_out: "queue.Queue" = queue.Queue(maxsize=2 * n_workers)
    lock = threading.Lock()
    abort = threading.Event()  # a stage that fails releases the others instead of leaving them blocked on a full / empty queue
    t0 = time.perf_counter()

    def put(q, item):
        while not abort.is_set():
            try:
                q.put(item, timeout=0.2)
                return
            except queue.Full:
                pass

    def get(q):
        while not abort.is_set():
            try:
                return q.get(timeout=0.2)
            except queue.Empty:
                pass
        return None

    depth_box = [None]  # depth_out: the process's one depth object, made by the first lift worker that has a context
    depth_lock = threading.Lock()

    def depth_object(eng):
        from . import depth as _depth

        with depth_lock:
            if depth_box[0] is None:
                depth_box[0] = _depth.DeviceDepth(eng, ref_lens, count_deletions=depth_deletions)
            return depth_box[0]

    want_depth = depth_out is not None or pileup_out is not None  # the sites are tested against the depth
    pileup_box = [None]  # pileup_out: the process's one pileup object, made by the first lift worker that has a context

    def pileup_object(eng):
        from . import pileup as _pileup

        with depth_lock:
            if pileup_box[0] is None:
                pileup_box[0] = _pileup.DevicePileup(eng, ref_lens, regions=pileup_regions)
            return pileup_box[0]

    merge_windows = sorted_runs and run_windows != 1
    if merge_windows:
        import torch as _torch

        if run_budget_bytes is None:
            run_budget_bytes = _torch.cuda.mem_get_info(index.device)[0] // 2
        share = max(1, int(run_budget_bytes) // len(rds))  # a reader's part of the budget: no reader waits for another one's open group
        q_merge: "queue.Queue" = queue.Queue()
        mcond = threading.Condition()
        # per reader: the next window to take its place, the open group (windows, their retained bytes), the bytes of the groups on their
        # way through the merger, the groups closed so far
        m_next, m_open, m_open_bytes, m_closing, m_groups = [0] * len(rds), [[] for _ in rds], [0] * len(rds), [0] * len(rds), [0] * len(rds)
        written = []  # (path, windows of the run)

    def close_group(ci):  # (under mcond)
        if m_open[ci]:
            q_merge.put((ci, m_groups[ci], m_open[ci], m_open_bytes[ci]))
            m_closing[ci] += m_open_bytes[ci]
            m_groups[ci] += 1
            m_open[ci], m_open_bytes[ci] = [], 0

    def retain(run_id, n_bytes, make):
        """the window takes its place in its reader's open group, in window order: make() -> the devbatch.RetainedWindow (None: no record)"""
        ci, seq = run_id
        with mcond:
            while m_next[ci] != seq and not abort.is_set():
                mcond.wait(0.2)
            if m_open[ci] and ((run_windows and len(m_open[ci]) >= run_windows) or m_open_bytes[ci] + n_bytes > share):
                close_group(ci)
            while m_closing[ci] and m_closing[ci] + m_open_bytes[ci] + n_bytes > share and not abort.is_set():
                mcond.wait(0.2)
        held = make() if not abort.is_set() else None
        with mcond:
            m_open[ci].append(held)
            m_open_bytes[ci] += n_bytes
            m_next[ci] = seq + 1
            mcond.notify_all()

    def merger():
        eng = None
        try:
            import torch

            from . import devbatch
            dev = torch.device("cuda", index.device)
            tstream = torch.cuda.Stream(device=dev)
            eng = api.Engine(index, stream=tstream.cuda_stream)
            pool = devbatch.PinnedPool()
            while True:
                item = get(q_merge)
                if item is None:
                    break
                ci, group, held, nbytes = item
                runs = [h for h in held if h is not None and h.n_records]
                if runs:
                    if run_windows == 0 and len(rds) == 1 and group == 0:
                        run_path = out_path + ".m000000"  # renamed to out_path when it stays the only one
                    else:
                        run_path = "%s.r%02dm%06d%s" % (run_stem, ci, group, run_ext)
                    with torch.cuda.stream(tstream):
                        plan = eng.runs_merge_plan_dev([h.run() for h in runs], len(ref_names), int(run_chunk_bytes))
                        wr = bam.BamWriter(run_path, hdr_out, ref_names, ref_lens, level=level, n_threads=max(1, write_threads),
                                           index_path=run_path + ".bai" if index_runs else None)
                        emit_ms = index_ms = bgzf_ms = 0.0
                        for ch in devbatch.merged_chunks(eng, plan):
                            ixo = None
                            if index_runs:
                                ixo = eng.records_index_dev(ch.bytes, ch.n_bytes, ch.n_records, ch.record_off, len(ref_names))
                                index_ms += float(ixo.index_ms)
                            if device_bgzf:
                                rb = devbatch.DeviceBlocks(eng, ch, 0 if level == 0 else 1, pool=pool, dev=dev, index_out=ixo)
                                bgzf_ms += rb.bgzf_ms
                            else:
                                rb = devbatch.DeviceRecords(ch, pool=pool, dev=dev, index_out=ixo)
                            if index_runs:
                                wr.index_add(rb.index_entries)
                            if device_bgzf:
                                wr.write_blocks((rb.bytes, rb.n_bytes))
                            else:
                                wr.write((rb.bytes, rb.n_bytes))
                            rb.release()
                            emit_ms += ch.emit_ms
                        wr.close()
                    with lock:
                        written.append((run_path, len(runs)))
                        st.merge_plan_device_ms += float(plan.plan_ms)
                        st.merge_emit_device_ms += emit_ms
                        st.index_device_ms += index_ms
                        st.bgzf_device_ms += bgzf_ms
                for h in held:
                    if h is not None:
                        h.free()
                with mcond:
                    m_closing[ci] -= nbytes
                    mcond.notify_all()
        except BaseException as e:  # noqa: BLE001
            st.errors.append(f"merger: {e!r}")
            abort.set()
        finally:
            st.stage_done_s["merger"] = time.perf_counter() - t0
            if eng is not None:
                eng.close()

    # the input side is two stages: BGZF inflate + record walk (read_window), then the window's batch arrays (batch_desc: CIGARs,
    # bases, qualities gathered into the plo_batch_in layout) -- about half of the reader's time each
    q_wins = [queue.Queue(maxsize=2) for _ in rds]
    chains_left = [len(rds)]  # batcher chains still running: the last one posts the lift workers' sentinels and starts the readers' teardown

    def reader(ci):
        rd, q_win = rds[ci], q_wins[ci]
        try:
            # the first windows are small and double up to window_reads: the stages behind the reader start after milliseconds instead of
            # after a whole window's decode -- a five-stage pipeline over a handful of full windows is mostly ramp otherwise
            n_win = 0
            while True:
                t = time.perf_counter()
                size = window_reads if not ramp else min(window_reads, max(256, window_reads >> max(0, 4 - n_win)))
                n_win += 1
                win = rd.read_window(size)
                if win is None:
                    break
                with lock:
                    st.read_s += time.perf_counter() - t
                put(q_win, (win, (ci, n_win - 1)))  # (reader, the window's sequence number at it): names the window's run with sorted_runs
        except BaseException as e:  # noqa: BLE001
            st.errors.append(f"reader {ci}: {e!r}")
            abort.set()
        finally:
            st.stage_done_s["reader" if len(rds) == 1 else f"reader {ci}"] = time.perf_counter() - t0
            put(q_win, None)

    def batcher(ci):
        q_win = q_wins[ci]
        try:
            while True:
                item = get(q_win)
                if item is None:
                    break
                win, run_id = item
                t = time.perf_counter()
                if not win.n_records:
                    desc = None
                elif device_input:
                    desc = win  # (the records and read_rec_off are on the device already)
                elif device_batch:
                    desc = win.raw()  # plo_window_raw alone: the batch is built on the device
                elif device_records:
                    desc = win.batch_raw()  # (plo_batch_in, plo_finish_in, plo_window_raw): nothing gathered, views into the records
                elif device_finish:
                    desc = win.batch_desc(with_finish=True)  # (plo_batch_in, plo_finish_in), dense bases
                else:
                    desc = win.batch_desc(sparse_margin=sparse_margin, index_desc=ixd if sparse_margin is not None else None)
                with lock:
                    st.batch_s += time.perf_counter() - t
                put(q_in, (win, desc, run_id))
        except BaseException as e:  # noqa: BLE001
            st.errors.append(f"batcher {ci}: {e!r}")
            abort.set()
        finally:
            st.stage_done_s["batcher" if len(rds) == 1 else f"batcher {ci}"] = time.perf_counter() - t0
            with lock:
                chains_left[0] -= 1
                last = chains_left[0] == 0
            if last:
                for _ in range(n_workers):
                    put(q_in, None)
                # the readers' teardown (page-locked stream buffers and device buffers: ~0.1 s for a 4 GB input) runs beside the last
                # windows' lifting and writing: no window needs its reader once its batch is built
                closer.start()

    def lifter(k):
        eng = None
        try:
            # the set-up is inside the try: a failure here (no CUDA torch, out of memory, a bad device) must set `abort` and still post
            # the worker's sentinel, or the writer waits for it forever and the run hangs instead of raising
            if device_finish:
                import torch

                from . import devbatch
                dev = torch.device("cuda", index.device)
                tstream = torch.cuda.Stream(device=dev)  # uploads, kernels and downloads of this worker, in order
                eng = api.Engine(index, stream=tstream.cuda_stream)
                sa_in, _sa_keep = devbatch.sa_inputs(ref_names, dev)
                arena = devbatch.PinnedArena() if not os.environ.get("PLO_PIPELINE_PAGEABLE_RESULTS") and not device_records else None
                if device_records:
                    labels = devbatch.contig_labels(contig_names, dev)
                    pool = devbatch.PinnedPool()
            else:
                eng = api.Engine(index)
            while True:
                item = get(q_in)
                if item is None:
                    break
                win, desc, run_id = item
                rb = None
                if desc is not None:
                    t = time.perf_counter()
                    if device_records:
                        marks = [("start", t)]
                        with torch.cuda.stream(tstream):
                            if device_batch:
                                ur = (devbatch.UploadedRecords(desc.records, desc.records_bytes, desc.read_rec_off, desc.n_reads) if device_input
                                      else devbatch.upload_records(desc, dev))
                                marks.append(("upload (issue)", time.perf_counter()))
                                up = devbatch.DeviceBuiltWindow(ur, eng.batch_build_dev(ur.build_in(labels)))
                                marks.append(("batch", time.perf_counter()))
                                ddesc = up.desc()
                            else:
                                up = devbatch.upload_raw_window(desc[0], desc[1], desc[2], dev)
                                marks.append(("upload (issue)", time.perf_counter()))
                                ddesc = up.batch.desc()
                            out = eng.liftover_batch_dev(ddesc)
                            marks.append(("liftover", time.perf_counter()))
                            eng.compact_output_dev(out)
                            marks.append(("compact", time.perf_counter()))
                            fo = eng.finish_batch_dev(ddesc, up.finish_in())
                            marks.append(("finish", time.perf_counter()))
                            so = eng.sa_segments_dev(sa_in)
                            marks.append(("sa text", time.perf_counter()))
                            nm_ms = 0.0
                            if emit_nm:
                                nm_ms = float(eng.nm_dev(ddesc).nm_ms)
                                marks.append(("nm", time.perf_counter()))
                            md_ms = 0.0
                            if emit_md:
                                md_ms = float(eng.md_dev(ddesc).md_ms)
                                marks.append(("md", time.perf_counter()))
                            eqx_ms = 0.0
                            if emit_eqx:
                                eqx_ms = float(eng.eqx_dev(ddesc).eqx_ms)
                                marks.append(("eqx", time.perf_counter()))
                            ro = eng.records_build_dev(ddesc, up.records_in(labels, is_target_region))
                            marks.append(("records", time.perf_counter()))
                            depth_ms = 0.0
                            if want_depth and ro.n_records:
                                depth_ms = float(depth_object(eng).add(eng, ro.bytes, ro.n_bytes, ro.n_records, ro.record_off).add_ms)
                                marks.append(("depth", time.perf_counter()))
                            pileup_ms = 0.0
                            if pileup_out is not None and ro.n_records:
                                pileup_ms = float(pileup_object(eng).add(ro, eng).add_ms)
                                marks.append(("pileup", time.perf_counter()))
                            srt, sort_ms = None, 0.0
                            if sorted_runs and ro.n_records:
                                srt = eng.records_sort_dev(ro.bytes, ro.n_bytes, ro.n_records, ro.record_off, len(ref_names))
                                sort_ms = float(srt.sort_ms)
                                marks.append(("sort", time.perf_counter()))
                            ixo, index_ms = None, 0.0
                            if merge_windows:  # the sorted window stays on the device; the merger writes its group's run
                                rb = devbatch.RetainedCounts(ro)
                                retain(run_id, int(ro.n_bytes), (lambda: devbatch.RetainedWindow(srt, dev)) if srt is not None else (lambda: None))
                                marks.append(("retain", time.perf_counter()))
                            elif index_runs and srt is not None:
                                ixo = eng.records_index_dev(srt.bytes, srt.n_bytes, srt.n_records, srt.record_off, len(ref_names))
                                index_ms = float(ixo.index_ms)
                                marks.append(("index", time.perf_counter()))
                            if not merge_windows and device_bgzf:
                                rb = devbatch.DeviceBlocks(eng, ro, 0 if level == 0 else 1, pool=pool, dev=dev, sorted_out=srt, index_out=ixo)
                                marks.append(("bgzf", time.perf_counter() - rb.block_s - rb.copy_s))
                            elif not merge_windows:
                                rb = devbatch.DeviceRecords(ro, pool=pool, dev=dev, sorted_out=srt, index_out=ixo)
                            if not merge_windows:
                                now = time.perf_counter()
                                marks.append(("download: page-locked block", now - rb.copy_s))
                                marks.append(("download: copy", now))
                        t1 = time.perf_counter()
                        with lock:
                            for (_, a), (name, b) in zip(marks, marks[1:]):
                                st.lift_detail_s[name] = st.lift_detail_s.get(name, 0.0) + (b - a)
                            st.finish_device_ms += float(fo.finish_ms) + float(fo.revcomp_ms) + float(so.sa_ms)
                            st.records_device_ms += rb.records_ms
                            st.nm_device_ms += nm_ms
                            st.md_device_ms += md_ms
                            st.eqx_device_ms += eqx_ms
                            st.sort_device_ms += sort_ms
                            if depth_out is not None:
                                st.depth_device_ms += depth_ms
                            else:
                                pileup_ms += depth_ms
                            st.pileup_device_ms += pileup_ms
                            st.index_device_ms += index_ms
                            st.batch_device_ms += getattr(up, "batch_ms", 0.0)
                            st.bgzf_device_ms += getattr(rb, "bgzf_ms", 0.0)
                        del up
                    elif device_finish:
                        marks = [("start", t)]
                        with torch.cuda.stream(tstream):
                            up = devbatch.upload_window(desc[0], desc[1], dev)
                            marks.append(("upload (issue)", time.perf_counter()))
                            ddesc = up.batch.desc()
                            out = eng.liftover_batch_dev(ddesc)
                            marks.append(("liftover", time.perf_counter()))
                            eng.compact_output_dev(out)
                            marks.append(("compact", time.perf_counter()))
                            fo = eng.finish_batch_dev(ddesc, up.finish_in())
                            marks.append(("finish", time.perf_counter()))
                            so = eng.sa_segments_dev(sa_in)
                            marks.append(("sa text", time.perf_counter()))
                            if arena is not None:
                                arena.reset()
                            host = devbatch.HostResults(eng, out, fo, so, win.n_records, arena=arena, dev=dev)
                            marks.append(("download", time.perf_counter()))
                        t1 = time.perf_counter()
                        with lock:
                            for (_, a), (name, b) in zip(marks, marks[1:]):
                                st.lift_detail_s[name] = st.lift_detail_s.get(name, 0.0) + (b - a)
                        rb = win.build_records_finished_raw(host.lift, host.fin, host.sa, ixd, contig_names, ref_names, is_target_region, build_threads)
                        with lock:
                            st.finish_device_ms += float(fo.finish_ms) + float(fo.revcomp_ms) + float(so.sa_ms)
                        del up
                    else:
                        lift = eng.liftover_batch_host(desc)
                        t1 = time.perf_counter()
                        rb = win.build_records_raw(lift, ixd, contig_names, ref_names, is_target_region, build_threads)
                    t2 = time.perf_counter()
                    tm = eng.timing()
                    with lock:
                        st.lift_s += t1 - t
                        st.build_s += t2 - t1
                        st.device_ms += tm.total_ms
                        st.reads += win.n_records
                        st.windows += 1
                        st.records_out += int(rb.n_records)
                        st.lifted += int(rb.n_lifted)
                        st.unmapped_copies += int(rb.n_unmapped_copies)
                        st.bytes_out += int(getattr(rb, "n_in", rb.n_bytes))
                elif merge_windows:
                    retain(run_id, 0, lambda: None)  # a window without a primary record still takes its place in its group
                put(q_out, (win, rb, run_id))
        except BaseException as e:  # noqa: BLE001
            st.errors.append(f"lift worker {k}: {e!r}")
            abort.set()
        finally:
            st.stage_done_s[f"lift worker {k}"] = time.perf_counter() - t0
            if eng is not None:
                eng.close()

    un_lock = threading.Lock()

    def close_reader():
        t = time.perf_counter()
        for r_ in rds:
            st.inflate_device_ms += getattr(r_, "inflate_ms", 0.0)
            st.cut_device_ms += getattr(r_, "cut_ms", 0.0)
            st.part_start_device_ms += getattr(r_, "part_start_ms", 0.0)
            r_.close()
        st.stage_done_s["reader closed"] = time.perf_counter() - t0
        st.stage_done_s["reader close took"] = time.perf_counter() - t

    closer = threading.Thread(target=close_reader)

    def writer(k):
        # (one sentinel per writer, posted by the main thread when every lift worker has ended)
        try:
            while not abort.is_set():
                item = get(q_out)
                if item is None:
                    break
                win, rb, run_id = item
                t = time.perf_counter()
                if rb is not None and rb.n_bytes and not merge_windows:
                    if sorted_runs:  # the window's run: a complete BAM of its own
                        run_path = "%s.r%02dw%06d%s" % (run_stem, run_id[0], run_id[1], run_ext)
                        wr = bam.BamWriter(run_path, hdr_out, ref_names, ref_lens, level=level, n_threads=max(1, write_threads),
                                           index_path=run_path + ".bai" if index_runs else None)
                        out_paths.append(run_path)
                        if index_runs:
                            wr.index_add(rb.index_entries)
                    else:
                        wr = wrs[k]
                    if getattr(rb, "is_blocks", False):
                        wr.write_blocks((rb.bytes, rb.n_bytes))
                    else:
                        wr.write((rb.bytes, rb.n_bytes))
                    if sorted_runs:
                        wr.close()
                ub, nu = win.unmapped_bytes()
                if nu:
                    with un_lock:
                        st.unmapped_passed_through += nu
                        if un is not None:
                            un.write(ub)
                if rb is not None and hasattr(rb, "release"):
                    rb.release()  # (device_records: the page-locked block of the window's bytes goes back to its worker's pool)
                win.close()
                with lock:
                    st.write_s += time.perf_counter() - t
        except BaseException as e:  # noqa: BLE001
            st.errors.append(f"writer {k}: {e!r}")
            abort.set()
        st.stage_done_s["writer" if out_shards == 1 else f"writer {k}"] = time.perf_counter() - t0

    st.stage_done_s["set up"] = time.perf_counter() - t0
    front = ([threading.Thread(target=reader, args=(ci,)) for ci in range(len(rds))] + [threading.Thread(target=batcher, args=(ci,)) for ci in range(len(rds))] +
             [threading.Thread(target=lifter, args=(k,)) for k in range(n_workers)])
    writers = [threading.Thread(target=writer, args=(k,)) for k in range(out_shards)]
    for t in front + writers:
        t.start()
    if merge_windows:
        t_merger = threading.Thread(target=merger)
        t_merger.start()
    for t in front:
        t.join()
    if want_depth and not st.errors:  # every add is through: the workers are joined
        from . import depth as _depth
        from . import pileup as _pileup

        deng = None
        try:
            deng = api.Engine(index)
            dobj = depth_object(deng)
            ms = dobj.finish(deng)
            if depth_out is not None:
                win_first, win_sums, wms = dobj.windows(deng, int(depth_window))
                runs_, rms = dobj.runs(deng, with_ms=True)
                st.depth_device_ms += ms + wms + rms
                st.depth_paths = [depth_out + ".per-base.bed", depth_out + ".regions.bed"]
                _depth.write_per_base(st.depth_paths[0], ref_names, runs_)
                _depth.write_regions(st.depth_paths[1], ref_names, [int(n) for n in ref_lens], int(depth_window), win_first, win_sums)
            else:
                st.pileup_device_ms += ms
            if pileup_out is not None:
                sites_, sms = pileup_object(deng).sites(dobj, min_count=int(pileup_min_count), min_frac=(int(pileup_min_frac[0]), int(pileup_min_frac[1])), engine=deng, with_ms=True)
                st.pileup_device_ms += sms
                st.pileup_paths = [pileup_out + ".sites.tsv"]
                _pileup.write_sites(st.pileup_paths[0], ref_names, sites_)
        except BaseException as e:  # noqa: BLE001
            st.errors.append(f"{'depth' if pileup_out is None else 'depth / pileup'}: {e!r}")
            abort.set()
        finally:
            for box in (depth_box, pileup_box):
                if box[0] is not None:
                    box[0].close()
            if deng is not None:
                deng.close()
    else:
        for box in (depth_box, pileup_box):
            if box[0] is not None:
                box[0].close()
    if merge_windows:
        with mcond:
            for ci in range(len(rds)):
                close_group(ci)
        q_merge.put(None)
        t_merger.join()
        written.sort()
        if run_windows == 0 and len(rds) == 1 and written and not st.errors:
            if len(written) == 1:  # the run is the output
                os.replace(written[0][0], out_path)
                if index_runs:
                    os.replace(written[0][0] + ".bai", out_path + ".bai")
                written = [(out_path, written[0][1])]
            else:  # the budget cut the reader's windows into several groups: the first one takes its name among them
                first = "%s.r%02dm%06d%s" % (run_stem, 0, 0, run_ext)
                os.replace(written[0][0], first)
                if index_runs:
                    os.replace(written[0][0] + ".bai", first + ".bai")
                written[0] = (first, written[0][1])
                written.sort()
        out_paths.extend(p_ for p_, _ in written)
    for _ in writers:
        put(q_out, None)
    for t in writers:
        t.join()
    for wr in wrs:
        wr.close()
    if sorted_runs:
        if not out_paths and not st.errors:  # no output record at all: one header-only run, so that a merge has a header
            out_paths.append(out_path if run_windows == 0 and len(rds) == 1 else "%s.r%02d%s%06d%s" % (run_stem, 0, "m" if merge_windows else "w", 0, run_ext))
            bam.BamWriter(out_paths[0], hdr_out, ref_names, ref_lens, level=level, n_threads=1, index_path=out_paths[0] + ".bai" if index_runs else None).close()
        out_paths.sort()
        st.out_paths = list(out_paths)
        st.run_groups = [dict(written).get(p_, 0) for p_ in out_paths] if merge_windows else [1] * len(out_paths)
        if index_runs:
            st.index_paths = [p_ + ".bai" for p_ in out_paths]
    st.out_file_bytes = sum(os.path.getsize(p_) for p_ in out_paths if os.path.exists(p_))
    st.stage_done_s["output closed"] = time.perf_counter() - t0
    if un is not None:
        un.close()
    if closer.ident is not None:  # (started by the last batcher)
        closer.join()
    else:
        for r_ in rds:
            r_.close()
    st.seconds = time.perf_counter() - t0
    st.stage_done_s["all closed"] = st.seconds
    if st.errors:
        raise RuntimeError("; ".join(st.errors))
    return st
