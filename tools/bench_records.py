"""Record assembly of ONE window on the device against the host builder: one process, one context, a time limit of its own.

For a chr20 window of --reads reads held in memory, JSON with
  - the yardstick: wall time of plo_records_build_finished with --threads host threads (what the pipeline's device_finish mode does);
  - plo_records_build_dev: records_ms (HIP events), bytes read + written per records_ms, the D2H time of the record bytes, the H2D time
    of the raw window against the H2D of the separate seq + qual arrays it replaces;
  - the byte-copy instantiation (PLO_RECORDS_BYTECOPY=1, a context of its own) against the 16-byte one.
  - plo_bgzf_compress_dev on the records where plo_records_build_dev left them (--bgzf-out): bgzf_ms at level 0 and at --level, the
    compressed bytes and their D2H time beside the D2H of the raw bytes, payload GB/s through the kernels beside the 16-thread host writer
    at the same level on the same bytes; every block is inflated with zlib and compared.  With --e2e-reads also run_bam_to_bam with the
    host writer against device_bgzf, at level 0 and at --level, three alternating runs each.
  - plo_batch_build_dev on the uploaded records (--batch-out; this leg runs alone): batch_ms (HIP events) and the call's wall time beside
    the wall time of the host's plo_bam_window_batch_raw with --threads threads on the same window, the bytes of segment / CIGAR / per-read
    arrays whose upload it saves and the time of that upload; every array is compared with the host's.  With --e2e-reads also
    run_bam_to_bam device_records against device_records + device_batch, three alternating runs each.
  - plo_part_start_dev and the first cut of part 1 of 2 of the window's file against plo_bam_open_range and its first window on the host
    (--part-out; this leg runs alone)
  - plo_nm_dev on the window (--nm-out; this leg runs alone): nm_ms beside the window's lift, finish and records_ms event times, the bases
    compared and the kernel's algorithmic bytes, and one device-to-device hipMemcpyAsync of that many bytes taken in the same process
  - plo_md_dev on the window (--md-out; runs alone or behind --nm-out): md_ms (count pass, scan, emit pass) beside the same window's nm_ms,
    lift, finish and records_ms event times, the text's bytes and the two passes' algorithmic bytes, and one device-to-device
    hipMemcpyAsync of that many bytes taken in the same process
  - plo_eqx_dev on the window (--eqx-out; runs alone or behind --nm-out / --md-out): eqx_ms (count pass, scan, emit pass) beside the same
    window's nm_ms, md_ms, lift, finish and records_ms event times (records_ms without a result and with the eqx result alone), the ops
    written and the two passes' algorithmic bytes, and one device-to-device hipMemcpyAsync of that many bytes taken in the same process
  - plo_records_sort_dev on the window's records (--sort-out; this leg runs alone): sort_ms beside the window's records_ms, and one
    device-to-device hipMemcpyAsync of n_bytes taken in the same process (the floor of the permuted copy).  perm, key, record_off and the
    bytes are compared with the order computed on the host (numpy, from the definition of the key) before anything is timed
  - plo_runs_merge_plan_dev / plo_runs_merge_emit_dev on --merge-windows sorted, retained windows (--merge-out; this leg runs alone): plan_ms
    and the summed emit_ms beside plo_records_sort_dev over the windows' concatenation and a device-to-device copy of the same bytes;
    the merged bytes are compared with that sort's output before any timing
  - plo_records_index_dev on the window's sorted records (--index-out; this leg runs alone): index_ms beside the window's sort_ms and
    records_ms, and one device-to-device hipMemcpyAsync of the call's algorithmic read bytes (36 + 4 n_cigar_op a record) taken in the
    same process; the entries are compared with those computed on the host (numpy, from the rule) before anything is timed.  On the CPU:
    the writer's close with and without an index, and the merge of the window's two halves with and without one
  - plo_depth_add_dev on the window's records (--depth-out; this leg runs alone): add_ms beside index_ms of the same records (the same walk
    of every CIGAR without atomics), and finish_ms, windows_ms and runs_ms beside one device-to-device hipMemcpyAsync of the array's bytes
    taken in the same process; differences, depths, window sums and the run count are compared with numpy's before anything is timed
  - plo_pileup_add_dev on the window's records (--pileup-out; this leg runs alone): add_ms beside nm_ms of the same window (the same base
    pairs, no scattered atomics) and depth's add_ms on the same records, sites_ms beside one device-to-device copy of the array's bytes;
    events per record and their share by channel; the array and the sites are compared with numpy's (tests/pileup_expect.py) first
  - plo_bgzf_inflate_dev + plo_window_cut_dev on the window's file (--cut-out; this leg runs alone): inflate_ms and cut_ms (HIP events) and
    the calls' wall time beside the wall time of bam.BamReader.read_window + devbatch.upload_records on the same file; read_rec_off, the
    window's bytes and the unmapped records are compared with the host reader's before anything is timed.  With --e2e-reads also
    run_bam_to_bam device_records + device_batch against the same plus device_input, three alternating runs each.
Exits non-zero on any byte mismatch between the device's records and the host's.

    python tools/bench_records.py --reads 50000 --out profiles/r07_records_window.json
    python tools/bench_records.py --reads 50000 --level 1 --bgzf-out profiles/r08_bgzf_window.json --e2e-reads 180000
    python tools/bench_records.py --reads 50000 --batch-out profiles/r09_batch_window.json --e2e-reads 180000
    python tools/bench_records.py --reads 50000 --cut-out profiles/r10_cut_window.json --e2e-reads 180000
    python tools/bench_records.py --reads 50000 --part-out profiles/r11_part_start.json
    python tools/bench_records.py --reads 50000 --nm-out profiles/r12_nm_window.json
    python tools/bench_records.py --reads 50000 --nm-out profiles/r13_nm_window.json --md-out profiles/r13_md_window.json
    python tools/bench_records.py --reads 50000 --sort-out profiles/r14_sort_window.json
    python tools/bench_records.py --reads 50000 --index-out profiles/r15_index_window.json
    python tools/bench_records.py --reads 50000 --merge-out profiles/r18_merge_runs.json --merge-windows 4
    python tools/bench_records.py --reads 50000 --depth-out profiles/r19_depth.json
    python tools/bench_records.py --reads 50000 --pileup-out profiles/r20_pileup.json
"""
import argparse
import ctypes as C
import json
import os
import shutil
import signal
import statistics
import subprocess
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

COPY_CEILING_GBS = 6290.0  # bytes read + written per second of a float4 copy kernel measured on one MI355X (79 % of the 8 TB/s HBM3E peak)


def stats(xs):
    xs = sorted(xs)
    return {"median": statistics.median(xs), "min": xs[0], "max": xs[-1], "n": len(xs)}


def end_to_end(n_reads):
    """run_bam_to_bam reads/s, device_finish against device_records, three runs each, alternating (no gate: a report)"""
    import shutil

    import torch

    from portello_amd import api, bamsynth, pipeline, synth

    w = synth.generate(synth.config("chr20", n_reads=n_reads), device="cuda")
    d = tempfile.mkdtemp(prefix="plo_rec_e2e_")
    try:
        inp = os.path.join(d, "reads.bam")
        meta = bamsynth.write_read_bam(w, inp, level=1, n_threads=16)
        ixd = w.index_data()
        index = api.Index(w.index_data_device())
        cn, rn, rl = meta["contig_names"], bamsynth.ref_names(w), [int(s.numel()) for s in w.chrom_seq]
        kw = dict(window_reads=7500, n_workers=3, io_threads=16, out_shards=4)
        pipeline.run_bam_to_bam(inp, os.path.join(d, "warm.bam"), index, ixd, cn, rn, rl, window_reads=2000, n_workers=1, device_records=True)
        runs = {"device_finish": [], "device_records": []}
        detail = {}
        for k in range(3):
            for mode in ("device_finish", "device_records"):
                out = os.path.join(d, f"{mode}_{k}.bam")
                st = pipeline.run_bam_to_bam(inp, out, index, ixd, cn, rn, rl, **dict(kw, **{mode: True}))
                runs[mode].append(st.reads / st.seconds)
                detail[mode] = {"lift_s": st.lift_s, "build_s": st.build_s, "batch_s": st.batch_s, "write_s": st.write_s, "read_s": st.read_s,
                                "records_device_ms": st.records_device_ms, "lift_detail_s": dict(st.lift_detail_s), "records_out": st.records_out, "bytes_out": st.bytes_out}
                for p_ in st.out_paths:
                    os.unlink(p_)
        index.close()
        return {"reads": n_reads, "config": kw, "unit": "reads/s", **{m: {"median": statistics.median(v), "best": max(v), "runs": v} for m, v in runs.items()},
                "last_run_detail": detail}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def end_to_end_bgzf(n_reads, level):
    """run_bam_to_bam reads/s with device_records=True: the host writer against device_bgzf, at level 0 and at `level`, three alternating runs each"""
    import shutil

    from portello_amd import api, bamsynth, pipeline, synth

    w = synth.generate(synth.config("chr20", n_reads=n_reads), device="cuda")
    d = tempfile.mkdtemp(prefix="plo_bgzf_e2e_")
    try:
        inp = os.path.join(d, "reads.bam")
        meta = bamsynth.write_read_bam(w, inp, level=1, n_threads=16)
        ixd = w.index_data()
        index = api.Index(w.index_data_device())
        cn, rn, rl = meta["contig_names"], bamsynth.ref_names(w), [int(s.numel()) for s in w.chrom_seq]
        kw = dict(window_reads=7500, n_workers=3, io_threads=16, out_shards=4, device_records=True)
        pipeline.run_bam_to_bam(inp, os.path.join(d, "warm.bam"), index, ixd, cn, rn, rl, window_reads=2000, n_workers=1, device_records=True, device_bgzf=True, level=level)
        res = {"reads": n_reads, "config": kw, "unit": "reads/s"}
        for lv in (level, 0):
            runs = {"host_writer": [], "device_bgzf": []}
            detail = {}
            for k in range(3):
                for mode in ("host_writer", "device_bgzf"):
                    st = pipeline.run_bam_to_bam(inp, os.path.join(d, f"{mode}_{k}.bam"), index, ixd, cn, rn, rl, level=lv, device_bgzf=mode == "device_bgzf", **kw)
                    runs[mode].append(st.reads / st.seconds)
                    detail[mode] = {"seconds": st.seconds, "lift_s": st.lift_s, "write_s": st.write_s, "read_s": st.read_s, "bgzf_device_ms": st.bgzf_device_ms,
                                    "records_device_ms": st.records_device_ms, "out_file_bytes": st.out_file_bytes, "bytes_out": st.bytes_out,
                                    "lift_detail_s": dict(st.lift_detail_s)}
                    for p_ in st.out_paths:
                        os.unlink(p_)
            res[f"level_{lv}"] = {**{m: {"median": statistics.median(v), "best": max(v), "runs": v} for m, v in runs.items()}, "last_run_detail": detail}
        index.close()
        return res
    finally:
        shutil.rmtree(d, ignore_errors=True)


def end_to_end_batch(n_reads):
    """run_bam_to_bam reads/s with device_records=True: the host batcher against device_batch, three alternating runs each"""
    import shutil

    from portello_amd import api, bamsynth, pipeline, synth

    w = synth.generate(synth.config("chr20", n_reads=n_reads), device="cuda")
    d = tempfile.mkdtemp(prefix="plo_batch_e2e_")
    try:
        inp = os.path.join(d, "reads.bam")
        meta = bamsynth.write_read_bam(w, inp, level=1, n_threads=16)
        ixd = w.index_data()
        index = api.Index(w.index_data_device())
        cn, rn, rl = meta["contig_names"], bamsynth.ref_names(w), [int(s.numel()) for s in w.chrom_seq]
        kw = dict(window_reads=7500, n_workers=3, io_threads=16, out_shards=4, device_records=True)
        pipeline.run_bam_to_bam(inp, os.path.join(d, "warm.bam"), index, ixd, cn, rn, rl, window_reads=2000, n_workers=1, device_records=True, device_batch=True)
        runs = {"host_batch": [], "device_batch": []}
        detail = {}
        for k in range(3):
            for mode in ("host_batch", "device_batch"):
                st = pipeline.run_bam_to_bam(inp, os.path.join(d, f"{mode}_{k}.bam"), index, ixd, cn, rn, rl, device_batch=mode == "device_batch", **kw)
                runs[mode].append(st.reads / st.seconds)
                detail.setdefault(mode, []).append({"seconds": st.seconds, "batch_s": st.batch_s, "lift_s": st.lift_s, "write_s": st.write_s, "read_s": st.read_s,
                                                    "batch_device_ms": st.batch_device_ms, "records_device_ms": st.records_device_ms, "records_out": st.records_out,
                                                    "lift_detail_s": dict(st.lift_detail_s)})
                for p_ in st.out_paths:
                    os.unlink(p_)
        index.close()
        return {"reads": n_reads, "config": kw, "unit": "reads/s", **{m: {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v} for m, v in runs.items()},
                "run_detail": detail}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def end_to_end_cut(n_reads):
    """run_bam_to_bam reads/s with device_records + device_batch: the host reader against device_input, three alternating runs each"""
    import shutil

    from portello_amd import api, bamsynth, pipeline, synth

    w = synth.generate(synth.config("chr20", n_reads=n_reads), device="cuda")
    d = tempfile.mkdtemp(prefix="plo_cut_e2e_")
    try:
        inp = os.path.join(d, "reads.bam")
        meta = bamsynth.write_read_bam(w, inp, level=1, n_threads=16)
        ixd = w.index_data()
        index = api.Index(w.index_data_device())
        cn, rn, rl = meta["contig_names"], bamsynth.ref_names(w), [int(s.numel()) for s in w.chrom_seq]
        kw = dict(window_reads=7500, n_workers=3, io_threads=16, out_shards=4, device_records=True, device_batch=True)
        pipeline.run_bam_to_bam(inp, os.path.join(d, "warm.bam"), index, ixd, cn, rn, rl, window_reads=2000, n_workers=1, device_records=True, device_batch=True, device_input=True)
        runs = {"host_input": [], "device_input": []}
        detail = {}
        for k in range(3):
            for mode in ("host_input", "device_input"):
                st = pipeline.run_bam_to_bam(inp, os.path.join(d, f"{mode}_{k}.bam"), index, ixd, cn, rn, rl, device_input=mode == "device_input", **kw)
                runs[mode].append(st.reads / st.seconds)
                detail.setdefault(mode, []).append({"seconds": st.seconds, "read_s": st.read_s, "batch_s": st.batch_s, "lift_s": st.lift_s, "write_s": st.write_s,
                                                    "inflate_device_ms": st.inflate_device_ms, "cut_device_ms": st.cut_device_ms, "records_out": st.records_out,
                                                    "lift_detail_s": dict(st.lift_detail_s)})
                for p_ in st.out_paths:
                    os.unlink(p_)
        index.close()
        return {"reads": n_reads, "config": kw, "unit": "reads/s", **{m: {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v} for m, v in runs.items()},
                "run_detail": detail}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def cut_leg(a, path, index, dev):
    """ONE window: bam.BamReader.read_window + upload_records against inflate + cut on the device -> (JSON, results equal)"""
    import numpy as np
    import torch

    from portello_amd import api, bam, build, devbatch, devreader

    def host_route():
        rd = bam.BamReader(path, a.threads)
        t = time.perf_counter()
        win = rd.read_window(a.reads + 10)
        t1 = time.perf_counter()
        ur = devbatch.upload_records(win.raw(), dev)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return rd, win, ur, (t1 - t) * 1e3, (t2 - t1) * 1e3

    def device_route():
        rdr = devreader.DeviceBamReader(path, index)
        torch.cuda.synchronize()
        t = time.perf_counter()
        dw = rdr.read_window(a.reads + 10)
        return rdr, dw, (time.perf_counter() - t) * 1e3

    # compared before anything is timed
    rd, win, ur, _, _ = host_route()
    rdr, dw, _ = device_route()
    raw = win.raw()
    same = (dw.n_reads == int(raw.n_reads) and dw.records_bytes == int(raw.raw_bytes) and dw.unmapped_bytes() == win.unmapped_bytes() and
            bool(torch.equal(dw.read_rec_off, ur.rec_off)) and bool(torch.equal(dw.records[:dw.records_bytes], ur.raw[:ur.raw_bytes])))
    res = {"tool": "tools/bench_records.py", "reads": a.reads, "raw_window_bytes": int(raw.raw_bytes), "seg_bytes": 32768,
           "commit": a.commit or subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None, "source_hash": build.source_hash(),
           "warmup": a.warmup, "reps": a.reps, "window_equal_host": bool(same), "refills": rdr.n_refills, "recuts": rdr.n_recuts}
    win.close()
    rd.close()
    rdr.close()
    del ur, dw
    h_read, h_up, d_wall, d_inf, d_cut = [], [], [], [], []
    for k in range(a.warmup + a.reps):
        rd, win, ur, r_ms, u_ms = host_route()
        win.close()
        rd.close()
        del ur
        rdr, dw, w_ms = device_route()
        if k >= a.warmup:
            h_read.append(r_ms)
            h_up.append(u_ms)
            d_wall.append(w_ms)
            d_inf.append(rdr.inflate_ms)
            d_cut.append(rdr.cut_ms)
        rdr.close()
        del dw
    res.update({"host_read_window_ms": dict(stats(h_read), threads=a.threads), "host_upload_records_ms": stats(h_up), "device_read_window_wall_ms": stats(d_wall),
                "device_inflate_ms": stats(d_inf), "device_cut_ms": stats(d_cut)})
    return res, bool(same)


def part_leg(a, path, index):
    """part 1 of 2 of the window's file: plo_bam_open_range + the first read_window on the host against DeviceBamReader(part=1, n_parts=2)
    + its first read_window (plo_part_start_dev inside the open) -> (JSON, first windows equal)"""
    import torch

    from portello_amd import bam, build, devreader

    mr = max(1, a.reads // 4)

    def host_route():
        t = time.perf_counter()
        rd = bam.BamReader(path, a.threads, part=1, n_parts=2)
        t1 = time.perf_counter()
        win = rd.read_window(mr)
        return rd, win, (t1 - t) * 1e3, (time.perf_counter() - t1) * 1e3

    def device_route():
        torch.cuda.synchronize()
        t = time.perf_counter()
        rdr = devreader.DeviceBamReader(path, index, part=1, n_parts=2)
        t1 = time.perf_counter()
        dw = rdr.read_window(mr)
        return rdr, dw, (t1 - t) * 1e3, (time.perf_counter() - t1) * 1e3

    rd, win, _, _ = host_route()
    rdr, dw, _, _ = device_route()
    raw = win.raw()
    same = (dw.n_reads == int(raw.n_reads) and dw.records_bytes == int(raw.raw_bytes) and dw.unmapped_bytes() == win.unmapped_bytes() and
            dw.records[:dw.records_bytes].cpu().numpy().tobytes() == bytes(bytearray(raw.raw[:int(raw.raw_bytes)])))
    res = {"tool": "tools/bench_records.py", "reads": a.reads, "part": 1, "n_parts": 2, "first_window_reads": int(raw.n_reads), "first_window_bytes": int(raw.raw_bytes),
           "commit": a.commit or subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None, "source_hash": build.source_hash(),
           "warmup": a.warmup, "reps": a.reps, "first_window_equal_host": bool(same), "part_start_calls": rdr.n_start_calls}
    win.close()
    rd.close()
    rdr.close()
    del dw
    h_open, h_win, d_open, d_win, d_start, d_cut = [], [], [], [], [], []
    for k in range(a.warmup + a.reps):
        rd, win, o_ms, w_ms = host_route()
        win.close()
        rd.close()
        rdr, dw, do_ms, dw_ms = device_route()
        if k >= a.warmup:
            h_open.append(o_ms)
            h_win.append(w_ms)
            d_open.append(do_ms)
            d_win.append(dw_ms)
            d_start.append(rdr.part_start_ms)
            d_cut.append(rdr.cut_ms)
        rdr.close()
        del dw
    res.update({"host_open_range_ms": dict(stats(h_open), threads=a.threads), "host_first_window_ms": stats(h_win), "device_open_wall_ms": stats(d_open),
                "device_first_window_wall_ms": stats(d_win), "device_part_start_ms": stats(d_start), "device_first_cut_ms": stats(d_cut)})
    return res, bool(same)


def batch_leg(a, win, index, cn, dev):
    """ONE window: the host's plo_bam_window_batch_raw against plo_batch_build_dev on the uploaded records -> (JSON, arrays equal)"""
    import numpy as np
    import torch

    from portello_amd import api, build, devbatch

    def arr(ptr, dtype, count):
        if not count:
            return np.zeros(0, dtype)
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(count * np.dtype(dtype).itemsize,)).view(dtype)

    host_ms = []
    for k in range(a.warmup + a.reps):
        t = time.perf_counter()
        b, f, r = win.batch_raw()  # (the window's own thread count: the reader's, --threads)
        if k >= a.warmup:
            host_ms.append((time.perf_counter() - t) * 1e3)
    n, ns = int(b.n_reads), int(b.n_segs)
    n_ops = int(arr(b.seg_cigar_off, np.uint32, ns + 1)[-1])
    fields = (("read_is_reverse", np.uint8, n, b), ("read_seq_len", np.uint32, n, b), ("read_seq_off", np.uint64, n, b), ("read_flags", np.uint16, n, f),
              ("read_qual_off", np.uint64, n, f), ("seg_read", np.uint32, ns, b), ("seg_contig", np.uint32, ns, b), ("seg_pos", np.int64, ns, b),
              ("seg_is_fwd_strand", np.uint8, ns, b), ("seg_cigar_off", np.uint32, ns + 1, b), ("cigar", np.uint32, n_ops, b))
    saved = sum(cnt * np.dtype(dt).itemsize for _, dt, cnt, _ in fields)
    # the upload those arrays cost today: the whole raw window against the records + read_rec_off alone
    h2d_full, h2d_raw = [], []
    for k in range(a.warmup + a.reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        up_full = devbatch.upload_raw_window(b, f, r, dev)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ur = devbatch.upload_records(win.raw(), dev)
        torch.cuda.synchronize()
        if k >= a.warmup:
            h2d_full.append((t1 - t) * 1e3)
            h2d_raw.append((time.perf_counter() - t1) * 1e3)
    del up_full
    eng = api.Engine(index)
    labels = devbatch.contig_labels(cn, dev)
    torch.cuda.synchronize()
    bin_ = ur.build_in(labels)
    ms, wall = [], []
    for k in range(a.warmup + a.reps):
        t = time.perf_counter()
        bo = eng.batch_build_dev(bin_)
        if k >= a.warmup:
            wall.append((time.perf_counter() - t) * 1e3)
            ms.append(float(bo.batch_ms))
    same = int(bo.batch.n_reads) == n and int(bo.batch.n_segs) == ns
    for name, dt, cnt, src in fields:
        same = same and np.array_equal(eng.download(getattr(bo.fin if src is f else bo.batch, name), dt, cnt), arr(getattr(src, name), dt, cnt))
    eng.close()
    res = {"tool": "tools/bench_records.py", "reads": a.reads, "segments": ns, "cigar_ops": n_ops, "raw_window_bytes": int(r.raw_bytes),
           "commit": a.commit or subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None, "source_hash": build.source_hash(),
           "warmup": a.warmup, "reps": a.reps, "arrays_equal_host": bool(same),
           "host_window_batch_raw_ms": dict(stats(host_ms), threads=a.threads), "device_batch_ms": stats(ms), "device_batch_call_wall_ms": stats(wall),
           "upload_bytes_saved": int(saved), "h2d_raw_window_with_batch_ms": stats(h2d_full), "h2d_records_only_ms": stats(h2d_raw)}
    return res, bool(same)


def nm_leg(a, win, index, cn, rn, dev):
    """ONE window: plo_nm_dev beside the window's lift, finish and records calls, and against a device-to-device copy of its algorithmic bytes"""
    import numpy as np
    import torch

    from portello_amd import abi, api, build, devbatch

    def arr(ptr, dtype, count):
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(count * np.dtype(dtype).itemsize,)).view(dtype) if count else np.zeros(0, dtype)

    eng = api.Engine(index)
    b, f, r = win.batch_raw()
    up = devbatch.upload_raw_window(b, f, r, dev)
    torch.cuda.synchronize()
    ddesc = up.batch.desc()
    sa_in, keep = devbatch.sa_inputs(rn, dev)
    labels = devbatch.contig_labels(cn, dev)
    rin = up.records_in(labels, False)
    lift_ms, fin_ms, nm_ms, rec_ms, rec_plain_ms = [], [], [], [], []
    for k in range(a.warmup + a.reps):
        out = eng.liftover_batch_dev(ddesc)
        eng.compact_output_dev(out)
        tm = eng.timing()
        fo = eng.finish_batch_dev(ddesc, up.finish_in())
        so = eng.sa_segments_dev(sa_in)
        plain = eng.records_build_dev(ddesc, rin)  # (no NM result on the context yet: today's bytes)
        plain_bytes, plain_ms = int(plain.n_bytes), float(plain.records_ms)
        no = eng.nm_dev(ddesc)
        ro = eng.records_build_dev(ddesc, rin)
        if k >= a.warmup:
            lift_ms.append(float(tm.total_ms))
            fin_ms.append(float(fo.finish_ms) + float(fo.revcomp_ms) + float(so.sa_ms))
            nm_ms.append(float(no.nm_ms))
            rec_ms.append(float(ro.records_ms))
            rec_plain_ms.append(plain_ms)
    lift = devbatch.download(eng, out)
    lifted = np.flatnonzero(lift.item_status == abi.ITEM_LIFTED)
    l_seq = arr(b.read_seq_len, np.uint32, int(b.n_reads))[arr(b.seg_read, np.uint32, int(b.n_segs))[lift.item_seg[lifted]]].astype(np.int64)
    ops = lift.cigar.astype(np.int64)
    ref_adv = np.where(np.isin(ops & 15, (0, 2, 3, 7, 8)), ops >> 4, 0)
    csum = np.concatenate([[0], np.cumsum(ref_adv)])
    o0 = lift.item_cigar_off[lifted].astype(np.int64)
    o1 = o0 + lift.item_cigar_len[lifted]
    ref_span = csum[o1] - csum[o0]
    algo = int(((l_seq + 1) // 2).sum() + ref_span.sum() + 4 * int(lift.item_cigar_len[lifted].sum()))
    same = int(ro.n_bytes) == plain_bytes + 7 * len(lifted) and int(no.n_items) == lift.n_items
    # the yardstick: one device-to-device hipMemcpyAsync of that many bytes, in this process
    src, dst = torch.empty(algo, dtype=torch.uint8, device=dev), torch.empty(algo, dtype=torch.uint8, device=dev)
    src.zero_()
    d2d = []
    for k in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src, non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        if k >= a.warmup:
            d2d.append(e0.elapsed_time(e1))
    eng.close()
    med = lambda v: sorted(v)[len(v) // 2]
    res = {"tool": "tools/bench_records.py", "reads": a.reads, "items": int(lift.n_items), "lifted_items": int(len(lifted)), "cigar_ops_of_lifted": int(lift.item_cigar_len[lifted].sum()),
           "commit": a.commit or subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None, "source_hash": build.source_hash(),
           "warmup": a.warmup, "reps": a.reps, "records_grow_by_7_per_lifted": bool(same), "n_cmp_bases": int(no.n_cmp_bases), "algorithmic_bytes": algo,
           "algorithmic_bytes_note": "(l_seq + 1) / 2 + reference span + 4 x ops over the lifted items", "nm_ms": stats(nm_ms), "lift_ms": stats(lift_ms),
           "finish_sa_ms": stats(fin_ms), "records_ms": stats(rec_ms), "records_without_nm_ms": stats(rec_plain_ms), "d2d_copy_same_bytes_ms": stats(d2d),
           "nm_gbs": algo / med(nm_ms) / 1e6, "d2d_copy_gbs_read_plus_write": 2 * algo / med(d2d) / 1e6, "nm_over_d2d_copy_time": med(nm_ms) / med(d2d)}
    return res, bool(same)


def md_leg(a, win, index, cn, rn, dev):
    """ONE window: plo_md_dev beside the window's lift, finish, plo_nm_dev and records calls, and against a device-to-device copy of its
    algorithmic bytes"""
    import numpy as np
    import torch

    from portello_amd import abi, api, build, devbatch

    def arr(ptr, dtype, count):
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(count * np.dtype(dtype).itemsize,)).view(dtype) if count else np.zeros(0, dtype)

    eng = api.Engine(index)
    b, f, r = win.batch_raw()
    up = devbatch.upload_raw_window(b, f, r, dev)
    torch.cuda.synchronize()
    ddesc = up.batch.desc()
    sa_in, keep = devbatch.sa_inputs(rn, dev)
    labels = devbatch.contig_labels(cn, dev)
    rin = up.records_in(labels, False)
    lift_ms, fin_ms, nm_ms, md_ms, md_wall_ms, rec_ms, rec_plain_ms = [], [], [], [], [], [], []
    for k in range(a.warmup + a.reps):
        out = eng.liftover_batch_dev(ddesc)
        eng.compact_output_dev(out)
        tm = eng.timing()
        fo = eng.finish_batch_dev(ddesc, up.finish_in())
        so = eng.sa_segments_dev(sa_in)
        plain = eng.records_build_dev(ddesc, rin)  # (no NM or MD result on the context yet: the host builder's bytes)
        plain_bytes, plain_ms = int(plain.n_bytes), float(plain.records_ms)
        no = eng.nm_dev(ddesc)
        t0 = time.perf_counter()
        mo = eng.md_dev(ddesc)
        t1 = time.perf_counter()
        ro = eng.records_build_dev(ddesc, rin)
        if k >= a.warmup:
            lift_ms.append(float(tm.total_ms))
            fin_ms.append(float(fo.finish_ms) + float(fo.revcomp_ms) + float(so.sa_ms))
            nm_ms.append(float(no.nm_ms))
            md_ms.append(float(mo.md_ms))
            md_wall_ms.append((t1 - t0) * 1e3)
            rec_ms.append(float(ro.records_ms))
            rec_plain_ms.append(plain_ms)
    lift = devbatch.download(eng, out)
    lifted = np.flatnonzero(lift.item_status == abi.ITEM_LIFTED)
    l_seq = arr(b.read_seq_len, np.uint32, int(b.n_reads))[arr(b.seg_read, np.uint32, int(b.n_segs))[lift.item_seg[lifted]]].astype(np.int64)
    ops = lift.cigar.astype(np.int64)
    ref_adv = np.where(np.isin(ops & 15, (0, 2, 3, 7, 8)), ops >> 4, 0)
    csum = np.concatenate([[0], np.cumsum(ref_adv)])
    o0 = lift.item_cigar_off[lifted].astype(np.int64)
    o1 = o0 + lift.item_cigar_len[lifted]
    ref_span = csum[o1] - csum[o0]
    one_pass = int(((l_seq + 1) // 2).sum() + ref_span.sum() + 4 * int(lift.item_cigar_len[lifted].sum()))
    md_bytes = int(mo.md_bytes)
    algo = 2 * one_pass + md_bytes + 24 * int(lift.n_items)
    # the source records of this window carry no MD: the records grow by NM:i (7) and MD:Z (3 + text + NUL) per lifted record
    same = int(ro.n_bytes) == plain_bytes + (7 + 4) * len(lifted) + md_bytes and int(mo.n_items) == lift.n_items
    src, dst = torch.empty(algo, dtype=torch.uint8, device=dev), torch.empty(algo, dtype=torch.uint8, device=dev)
    src.zero_()
    d2d = []
    for k in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src, non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        if k >= a.warmup:
            d2d.append(e0.elapsed_time(e1))
    eng.close()
    med = lambda v: sorted(v)[len(v) // 2]
    res = {"tool": "tools/bench_records.py", "reads": a.reads, "items": int(lift.n_items), "lifted_items": int(len(lifted)), "cigar_ops_of_lifted": int(lift.item_cigar_len[lifted].sum()),
           "commit": a.commit or subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None, "source_hash": build.source_hash(),
           "warmup": a.warmup, "reps": a.reps, "records_grow_by_nm_and_md": bool(same), "md_bytes": md_bytes, "algorithmic_bytes": algo,
           "algorithmic_bytes_note": "2 x ((l_seq + 1) / 2 + reference span + 4 x ops over the lifted items) + the text + 24 x items (length out, offsets in and out)",
           "md_ms": stats(md_ms), "md_call_wall_ms": stats(md_wall_ms), "nm_ms": stats(nm_ms), "lift_ms": stats(lift_ms), "finish_sa_ms": stats(fin_ms),
           "records_ms": stats(rec_ms), "records_without_tags_ms": stats(rec_plain_ms), "d2d_copy_same_bytes_ms": stats(d2d),
           "md_gbs": algo / med(md_ms) / 1e6, "d2d_copy_gbs_read_plus_write": 2 * algo / med(d2d) / 1e6, "md_over_d2d_copy_time": med(md_ms) / med(d2d),
           "md_over_nm_time": med(md_ms) / med(nm_ms)}
    return res, bool(same)


def eqx_leg(a, win, index, cn, rn, dev):
    """ONE window: plo_eqx_dev beside the window's lift, finish, plo_nm_dev, plo_md_dev and records calls (records_ms without a result and
    with the eqx result alone), and against a device-to-device copy of its algorithmic bytes"""
    import numpy as np
    import torch

    from portello_amd import abi, api, build, devbatch

    def arr(ptr, dtype, count):
        return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(count * np.dtype(dtype).itemsize,)).view(dtype) if count else np.zeros(0, dtype)

    eng = api.Engine(index)
    b, f, r = win.batch_raw()
    up = devbatch.upload_raw_window(b, f, r, dev)
    torch.cuda.synchronize()
    ddesc = up.batch.desc()
    sa_in, keep = devbatch.sa_inputs(rn, dev)
    labels = devbatch.contig_labels(cn, dev)
    rin = up.records_in(labels, False)
    lift_ms, fin_ms, nm_ms, md_ms, eqx_ms, eqx_wall_ms, rec_ms, rec_plain_ms = [], [], [], [], [], [], [], []
    for k in range(a.warmup + a.reps):
        out = eng.liftover_batch_dev(ddesc)
        eng.compact_output_dev(out)
        tm = eng.timing()
        fo = eng.finish_batch_dev(ddesc, up.finish_in())
        so = eng.sa_segments_dev(sa_in)
        plain = eng.records_build_dev(ddesc, rin)  # (no result on the context yet: the host builder's bytes)
        plain_bytes, plain_ms = int(plain.n_bytes), float(plain.records_ms)
        t0 = time.perf_counter()
        eo = eng.eqx_dev(ddesc)
        t1 = time.perf_counter()
        ro = eng.records_build_dev(ddesc, rin)  # (the eqx result alone: the same records but for their CIGARs)
        ro_bytes, ro_ms = int(ro.n_bytes), float(ro.records_ms)
        no = eng.nm_dev(ddesc)
        mo = eng.md_dev(ddesc)
        if k >= a.warmup:
            lift_ms.append(float(tm.total_ms))
            fin_ms.append(float(fo.finish_ms) + float(fo.revcomp_ms) + float(so.sa_ms))
            nm_ms.append(float(no.nm_ms))
            md_ms.append(float(mo.md_ms))
            eqx_ms.append(float(eo.eqx_ms))
            eqx_wall_ms.append((t1 - t0) * 1e3)
            rec_ms.append(ro_ms)
            rec_plain_ms.append(plain_ms)
    lift = devbatch.download(eng, out)
    lifted = np.flatnonzero(lift.item_status == abi.ITEM_LIFTED)
    l_seq = arr(b.read_seq_len, np.uint32, int(b.n_reads))[arr(b.seg_read, np.uint32, int(b.n_segs))[lift.item_seg[lifted]]].astype(np.int64)
    ops = lift.cigar.astype(np.int64)
    ref_adv = np.where(np.isin(ops & 15, (0, 2, 3, 7, 8)), ops >> 4, 0)
    csum = np.concatenate([[0], np.cumsum(ref_adv)])
    o0 = lift.item_cigar_off[lifted].astype(np.int64)
    o1 = o0 + lift.item_cigar_len[lifted]
    ref_span = csum[o1] - csum[o0]
    one_pass = int(((l_seq + 1) // 2).sum() + ref_span.sum() + 4 * int(lift.item_cigar_len[lifted].sum()))
    n_ops = int(eo.n_ops)
    algo = 2 * one_pass + 4 * n_ops + 24 * int(lift.n_items)
    # the records differ by their CIGARs alone: 4 bytes an op, 16 more where the new count passes 65535 and the old one did not
    new_n = np.diff(eng.download(eo.item_eqx_off, np.uint64, int(eo.n_items) + 1).astype(np.int64))[lifted]
    old_n = lift.item_cigar_len[lifted].astype(np.int64)
    size = lambda n: 4 * n + 16 * (n > 0xFFFF)
    same = ro_bytes == plain_bytes + int((size(new_n) - size(old_n)).sum()) and int(eo.n_items) == lift.n_items and int(new_n.sum()) == n_ops
    src, dst = torch.empty(algo, dtype=torch.uint8, device=dev), torch.empty(algo, dtype=torch.uint8, device=dev)
    src.zero_()
    d2d = []
    for k in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src, non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        if k >= a.warmup:
            d2d.append(e0.elapsed_time(e1))
    eng.close()
    med = lambda v: sorted(v)[len(v) // 2]
    res = {"tool": "tools/bench_records.py", "reads": a.reads, "items": int(lift.n_items), "lifted_items": int(len(lifted)), "cigar_ops_of_lifted": int(old_n.sum()),
           "commit": a.commit or subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None, "source_hash": build.source_hash(),
           "warmup": a.warmup, "reps": a.reps, "records_differ_by_their_cigars_alone": bool(same), "eqx_ops": n_ops, "items_past_65535_ops": int((new_n > 0xFFFF).sum()),
           "algorithmic_bytes": algo,
           "algorithmic_bytes_note": "2 x ((l_seq + 1) / 2 + reference span + 4 x ops over the lifted items) + 4 x the ops written + 24 x items (count out, offsets in and out)",
           "eqx_ms": stats(eqx_ms), "eqx_call_wall_ms": stats(eqx_wall_ms), "nm_ms": stats(nm_ms), "md_ms": stats(md_ms), "lift_ms": stats(lift_ms), "finish_sa_ms": stats(fin_ms),
           "records_with_eqx_ms": stats(rec_ms), "records_without_result_ms": stats(rec_plain_ms), "d2d_copy_same_bytes_ms": stats(d2d),
           "eqx_gbs": algo / med(eqx_ms) / 1e6, "d2d_copy_gbs_read_plus_write": 2 * algo / med(d2d) / 1e6, "eqx_over_d2d_copy_time": med(eqx_ms) / med(d2d),
           "eqx_over_md_time": med(eqx_ms) / med(md_ms), "eqx_over_nm_time": med(eqx_ms) / med(nm_ms)}
    return res, bool(same)


def sort_leg(a, win, index, cn, rn, dev):
    """ONE window: plo_records_sort_dev on the records of plo_records_build_dev, against the host's expected order and a device-to-device
    copy of the same bytes"""
    import numpy as np
    import torch

    from portello_amd import api, build, devbatch
    from portello_amd.gather import device_view

    eng = api.Engine(index)
    b, f, r = win.batch_raw()
    up = devbatch.upload_raw_window(b, f, r, dev)
    torch.cuda.synchronize()
    ddesc = up.batch.desc()
    sa_in, keep = devbatch.sa_inputs(rn, dev)
    labels = devbatch.contig_labels(cn, dev)
    rin = up.records_in(labels, False)
    out = eng.liftover_batch_dev(ddesc)
    eng.compact_output_dev(out)
    eng.finish_batch_dev(ddesc, up.finish_in())
    eng.sa_segments_dev(sa_in)
    ro = eng.records_build_dev(ddesc, rin)
    n, nb, n_ref = int(ro.n_records), int(ro.n_bytes), len(rn)

    def down(ptr, count, dtype):
        return device_view(ptr, count * np.dtype(dtype).itemsize, torch.uint8, dev).cpu().numpy().view(dtype) if count else np.zeros(0, dtype)

    # the expected order, from the definition of the key
    data, off = down(ro.bytes, nb, np.uint8), down(ro.record_off, n + 1, np.uint64).astype(np.int64)
    at = off[:-1]
    fld = lambda o, w: sum(data[at + o + k].astype(np.int64) << (8 * k) for k in range(w))
    ref, pos, flag = fld(4, 4).astype(np.uint32).view(np.int32).astype(np.int64), fld(8, 4).astype(np.uint32).view(np.int32).astype(np.int64), fld(18, 2)
    key = (np.where(ref < 0, n_ref, ref) << 32) | ((pos + 1) << 1) | ((flag >> 4) & 1)
    perm = np.lexsort((np.arange(n), key))
    lens = np.diff(off)[perm]
    exp_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    so = eng.records_sort_dev(ro.bytes, nb, n, ro.record_off, n_ref)
    same = (int(so.n_records) == n and int(so.n_bytes) == nb and np.array_equal(down(so.perm, n, np.uint32), perm.astype(np.uint32)) and
            np.array_equal(down(so.key, n, np.uint64), key[perm].astype(np.uint64)) and np.array_equal(down(so.record_off, n + 1, np.uint64), exp_off) and
            int(so.n_mapped) == int((ref >= 0).sum()))
    if same and n:
        got = down(so.bytes, nb, np.uint8)
        same = all(np.array_equal(got[int(exp_off[j]):int(exp_off[j + 1])], data[int(off[i]):int(off[i + 1])]) for j, i in enumerate(perm))
        del got
    same = same and np.array_equal(down(ro.bytes, nb, np.uint8), data)  # the input is unchanged
    sort_ms, wall_ms, rec_ms = [], [], []
    for k in range(a.warmup + a.reps):
        ro = eng.records_build_dev(ddesc, rin)
        t0 = time.perf_counter()
        so = eng.records_sort_dev(ro.bytes, nb, n, ro.record_off, n_ref)
        t1 = time.perf_counter()
        if k >= a.warmup:
            sort_ms.append(float(so.sort_ms))
            wall_ms.append((t1 - t0) * 1e3)
            rec_ms.append(float(ro.records_ms))
    src, dst = torch.empty(max(16, nb), dtype=torch.uint8, device=dev), torch.empty(max(16, nb), dtype=torch.uint8, device=dev)
    src.zero_()
    d2d = []
    for k in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src, non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        if k >= a.warmup:
            d2d.append(e0.elapsed_time(e1))
    eng.close()
    med = lambda v: sorted(v)[len(v) // 2]
    tiles = (n + 1023) // 1024
    res = {"tool": "tools/bench_records.py", "reads": a.reads, "records": n, "n_bytes": nb, "n_ref": n_ref, "n_mapped": int(so.n_mapped),
           "commit": a.commit or subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None, "source_hash": build.source_hash(),
           "warmup": a.warmup, "reps": a.reps, "equals_host_order": bool(same), "launches_per_call": 6 + max(0, (tiles - 1).bit_length()),
           "sort_ms": stats(sort_ms), "sort_call_wall_ms": stats(wall_ms), "records_ms": stats(rec_ms), "d2d_copy_n_bytes_ms": stats(d2d),
           "sort_gbs_read_plus_write": 2 * nb / med(sort_ms) / 1e6, "d2d_copy_gbs_read_plus_write": 2 * nb / med(d2d) / 1e6,
           "sort_over_d2d_copy_time": med(sort_ms) / med(d2d), "sort_over_records_time": med(sort_ms) / med(rec_ms)}
    return res, bool(same)


def merge_leg(a, rd, index, cn, rn, dev):
    """K windows: each is lifted, its records are sorted (plo_records_sort_dev) and retained on the device (devbatch.RetainedWindow); then
    plo_runs_merge_plan_dev and the plo_runs_merge_emit_dev calls of all chunks, against plo_records_sort_dev over the concatenation of the K
    retained windows -- the way to get the same buffer without the merge -- and a device-to-device copy of the same bytes"""
    import numpy as np
    import torch

    from portello_amd import api, build, devbatch
    from portello_amd.gather import device_view

    eng = api.Engine(index)
    sa_in, keep = devbatch.sa_inputs(rn, dev)
    labels = devbatch.contig_labels(cn, dev)
    n_ref, K = len(rn), max(1, a.merge_windows)
    per, held, sort_window_ms = (a.reads + K - 1) // K, [], []
    for k in range(K):
        win = rd.read_window(per)
        if win is None or not win.n_records:
            break
        b, f, r = win.batch_raw()
        up = devbatch.upload_raw_window(b, f, r, dev)
        torch.cuda.synchronize()
        ddesc = up.batch.desc()
        out = eng.liftover_batch_dev(ddesc)
        eng.compact_output_dev(out)
        eng.finish_batch_dev(ddesc, up.finish_in())
        eng.sa_segments_dev(sa_in)
        ro = eng.records_build_dev(ddesc, up.records_in(labels, False))
        so = eng.records_sort_dev(ro.bytes, int(ro.n_bytes), int(ro.n_records), ro.record_off, n_ref)
        sort_window_ms.append(float(so.sort_ms))
        held.append(devbatch.RetainedWindow(so, dev))
        del up
        win.close()
    n, nb = sum(h.n_records for h in held), sum(h.n_bytes for h in held)
    runs = [h.run() for h in held]
    # the concatenation of the retained windows: the input of the sort the merge is read against
    cat = torch.empty(max(16, nb), dtype=torch.uint8, device=dev)
    cat_off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    at_b = at_r = 0
    for h in held:
        cat[at_b:at_b + h.n_bytes].copy_(h.raw[:h.n_bytes])
        cat_off[at_r:at_r + h.n_records + 1].copy_(h.off.view(torch.int64) + at_b)
        at_b, at_r = at_b + h.n_bytes, at_r + h.n_records
    torch.cuda.synchronize()

    def down(ptr, count, dtype):
        return device_view(ptr, count * np.dtype(dtype).itemsize, torch.uint8, dev).cpu().numpy().view(dtype) if count else np.zeros(0, dtype)

    # the merged bytes against that sort's output, before any timing
    so = eng.records_sort_dev(cat.data_ptr(), nb, n, cat_off.data_ptr(), n_ref)
    want, want_off = down(so.bytes, nb, np.uint8).copy(), down(so.record_off, n + 1, np.uint64).copy()
    po = eng.runs_merge_plan_dev(runs, n_ref, a.merge_chunk_bytes)
    nc = int(po.n_chunks)
    same = (int(po.n_records) == n and int(po.n_bytes) == nb and int(po.n_mapped) == int(so.n_mapped) and np.array_equal(down(po.src, n, np.uint32), down(so.perm, n, np.uint32)) and
            np.array_equal(down(po.key, n, np.uint64), down(so.key, n, np.uint64)) and np.array_equal(down(po.record_off, n + 1, np.uint64), want_off))
    chunk_off = np.ctypeslib.as_array(po.chunk_off, (nc + 1,)).copy()
    chunk_records = np.diff(np.ctypeslib.as_array(po.chunk_first, (nc + 1,))).tolist()
    for c in range(nc):
        co = eng.runs_merge_emit_dev(c)
        same = same and np.array_equal(down(co.bytes, int(co.n_bytes), np.uint8), want[int(chunk_off[c]):int(chunk_off[c + 1])])
    del want
    plan_ms, emit_ms, plan_wall, emit_wall, sort_ms = [], [], [], [], []
    for k in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        po = eng.runs_merge_plan_dev(runs, n_ref, a.merge_chunk_bytes)
        t1 = time.perf_counter()
        e = sum(float(eng.runs_merge_emit_dev(c).emit_ms) for c in range(nc))
        t2 = time.perf_counter()
        so = eng.records_sort_dev(cat.data_ptr(), nb, n, cat_off.data_ptr(), n_ref)
        if k >= a.warmup:
            plan_ms.append(float(po.plan_ms))
            emit_ms.append(e)
            plan_wall.append((t1 - t0) * 1e3)
            emit_wall.append((t2 - t1) * 1e3)
            sort_ms.append(float(so.sort_ms))
    dst, d2d = torch.empty(max(16, nb), dtype=torch.uint8, device=dev), []
    for k in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(cat, non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        if k >= a.warmup:
            d2d.append(e0.elapsed_time(e1))
    eng.close()
    med = lambda v: sorted(v)[len(v) // 2]
    res = {"tool": "tools/bench_records.py", "reads": a.reads, "windows": len(held), "window_records": [h.n_records for h in held], "records": n, "n_bytes": nb, "n_ref": n_ref,
           "chunk_bytes": a.merge_chunk_bytes, "n_chunks": nc, "chunk_records": chunk_records,
           "commit": a.commit or subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None, "source_hash": build.source_hash(),
           "warmup": a.warmup, "reps": a.reps, "equals_sort_of_concatenation": bool(same), "plan_launches_per_call": 6 + max(0, (len(held) - 1).bit_length()),
           "plan_ms": stats(plan_ms), "emit_ms_summed_over_chunks": stats(emit_ms), "plan_call_wall_ms": stats(plan_wall), "emit_calls_wall_ms": stats(emit_wall),
           "sort_of_concatenation_ms": stats(sort_ms), "sort_of_each_window_ms": sort_window_ms, "d2d_copy_n_bytes_ms": stats(d2d),
           "emit_gbs_read_plus_write": 2 * nb / med(emit_ms) / 1e6, "d2d_copy_gbs_read_plus_write": 2 * nb / med(d2d) / 1e6,
           "plan_plus_emit_over_sort_of_concatenation_time": (med(plan_ms) + med(emit_ms)) / med(sort_ms), "emit_over_d2d_copy_time": med(emit_ms) / med(d2d),
           "not_measured": ["genome-size groups (dozens of windows of 1.2 GB)", "short records", "n_runs in the hundreds"]}
    return res, bool(same)


def index_leg(a, win, index, cn, rn, rl, dev):
    """ONE window: plo_records_index_dev on the sorted records, against the entries computed on the host and a device-to-device copy of the
    call's algorithmic bytes; then, on the CPU, the writer's close with and without an index and the merge of the window's two halves with
    and without one"""
    import numpy as np
    import torch

    from portello_amd import api, bam, build, devbatch
    from portello_amd.gather import device_view

    eng = api.Engine(index)
    b, f, r = win.batch_raw()
    up = devbatch.upload_raw_window(b, f, r, dev)
    torch.cuda.synchronize()
    ddesc = up.batch.desc()
    sa_in, keep = devbatch.sa_inputs(rn, dev)
    labels = devbatch.contig_labels(cn, dev)
    rin = up.records_in(labels, False)
    out = eng.liftover_batch_dev(ddesc)
    eng.compact_output_dev(out)
    eng.finish_batch_dev(ddesc, up.finish_in())
    eng.sa_segments_dev(sa_in)
    ro = eng.records_build_dev(ddesc, rin)
    n, nb, n_ref = int(ro.n_records), int(ro.n_bytes), len(rn)
    so = eng.records_sort_dev(ro.bytes, nb, n, ro.record_off, n_ref)

    def down(ptr, count, dtype):
        return device_view(ptr, count * np.dtype(dtype).itemsize, torch.uint8, dev).cpu().numpy().view(dtype) if count else np.zeros(0, dtype)

    # the expected entries, from the rule: fixed fields, the CIGAR's reference length, reg2bin
    data, off = down(so.bytes, nb, np.uint8), down(so.record_off, n + 1, np.uint64).astype(np.int64)
    exp = np.zeros(n, abi_entry_dtype())
    n_ops = 0
    for i in range(n):
        p = int(off[i])
        ref, pos = (int(x) for x in data[p + 4:p + 12].view("<i4"))
        lrn, ncig, flag = int(data[p + 12]), int(data[p + 16:p + 18].view("<u2")[0]), int(data[p + 18:p + 20].view("<u2")[0])
        n_ops += ncig
        unm = (flag >> 2) & 1
        if ref < 0:
            exp[i] = (p, -1, -1, 0, unm | (4680 << 16))
            continue
        ops = data[p + 36 + lrn:p + 36 + lrn + 4 * ncig].view("<u4")
        rlen = int((ops >> 4)[np.isin(ops & 15, (0, 2, 3, 7, 8))].sum())
        beg = max(pos, 0)
        end = beg + 1 if unm or rlen == 0 else beg + rlen
        e1, bn = end - 1, 0
        for sh, base in ((14, 4681), (17, 585), (20, 73), (23, 9), (26, 1)):
            if beg >> sh == e1 >> sh:
                bn = base + (beg >> sh)
                break
        exp[i] = (p, ref, beg, end, unm | (bn << 16))
    io = eng.records_index_dev(so.bytes, nb, n, so.record_off, n_ref)
    got = down(io.entry, 24 * n, np.uint8).view(exp.dtype)
    same = int(io.n_records) == n and np.array_equal(got, exp) and int(io.n_placed) == int((exp["ref_id"] >= 0).sum())
    same = same and np.array_equal(down(so.bytes, nb, np.uint8), data)  # the input is unchanged
    index_ms, wall_ms, sort_ms, rec_ms = [], [], [], []
    for k in range(a.warmup + a.reps):
        ro = eng.records_build_dev(ddesc, rin)
        so = eng.records_sort_dev(ro.bytes, nb, n, ro.record_off, n_ref)
        t0 = time.perf_counter()
        io = eng.records_index_dev(so.bytes, nb, n, so.record_off, n_ref)
        t1 = time.perf_counter()
        if k >= a.warmup:
            index_ms.append(float(io.index_ms))
            wall_ms.append((t1 - t0) * 1e3)
            sort_ms.append(float(so.sort_ms))
            rec_ms.append(float(ro.records_ms))
    algo_read, algo_write = 36 * n + 4 * n_ops, 24 * n
    src, dst = torch.empty(max(16, algo_read), dtype=torch.uint8, device=dev), torch.empty(max(16, algo_read), dtype=torch.uint8, device=dev)
    src.zero_()
    d2d = []
    for k in range(a.warmup + a.reps):  # read + write of this copy = 2 algo_read >= the call's algo_read + algo_write
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src, non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        if k >= a.warmup:
            d2d.append(e0.elapsed_time(e1))
    eng.close()
    # the host side, on the CPU: level-0 files of the window's sorted records
    tmp = tempfile.mkdtemp(prefix="plo_index_host_")
    hdr = bam.output_header(rn, rl, sort_order="coordinate")
    half = n // 2
    cut = int(off[half])
    host = {}

    def write(path, lo, hi, e_lo, e_hi, indexed):
        wr = bam.BamWriter(path, hdr, rn, rl, level=0, n_threads=a.threads, index_path=path + ".bai" if indexed else None)
        if indexed:
            ent = exp[e_lo:e_hi].copy()
            ent["off"] -= lo
            wr.index_add(ent)
        wr.write(data[lo:hi])
        t0 = time.perf_counter()
        wr.close()
        return (time.perf_counter() - t0) * 1e3

    try:
        host["writer_close_ms_without_index"] = write(os.path.join(tmp, "plain.bam"), 0, nb, 0, n, False)
        host["writer_close_ms_with_index"] = write(os.path.join(tmp, "whole.bam"), 0, nb, 0, n, True)
        host["bai_bytes"] = os.path.getsize(os.path.join(tmp, "whole.bam.bai"))
        runs = [os.path.join(tmp, "h0.bam"), os.path.join(tmp, "h1.bam")]
        write(runs[0], 0, cut, 0, half, False)
        write(runs[1], cut, nb, half, n, False)
        for name, indexed in (("merge_ms_without_index", False), ("merge_ms_with_index", True), ("merge_ms_without_index_again", False)):
            t0 = time.perf_counter()
            bam.merge_runs(runs, os.path.join(tmp, name + ".bam"), n_threads=a.threads, index=indexed)
            host[name] = (time.perf_counter() - t0) * 1e3
        host["merged_files_equal"] = open(os.path.join(tmp, "merge_ms_without_index.bam"), "rb").read() == open(os.path.join(tmp, "merge_ms_with_index.bam"), "rb").read()
        same = same and host["merged_files_equal"]
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    med = lambda v: sorted(v)[len(v) // 2]
    res = {"tool": "tools/bench_records.py", "reads": a.reads, "records": n, "n_bytes": nb, "n_ref": n_ref, "n_placed": int(io.n_placed), "cigar_ops": n_ops,
           "commit": a.commit or subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None, "source_hash": build.source_hash(),
           "warmup": a.warmup, "reps": a.reps, "equals_host_entries": bool(same), "launches_per_call": 1,
           "algo_bytes_read": algo_read, "algo_bytes_written": algo_write,
           "index_ms": stats(index_ms), "index_call_wall_ms": stats(wall_ms), "sort_ms": stats(sort_ms), "records_ms": stats(rec_ms), "d2d_copy_algo_read_bytes_ms": stats(d2d),
           "index_gbs_algo_read_plus_write": (algo_read + algo_write) / med(index_ms) / 1e6, "d2d_copy_gbs_read_plus_write": 2 * algo_read / med(d2d) / 1e6,
           "index_over_d2d_copy_time": med(index_ms) / med(d2d), "index_over_sort_time": med(index_ms) / med(sort_ms), "index_over_records_time": med(index_ms) / med(rec_ms),
           "host_cpu": host,
           "not_timed": "the entries' download (24 bytes a record, it rides with the window's bytes in the pipeline); end-to-end throughput with index_runs"}
    return res, bool(same)


def depth_leg(a, win, index, cn, rn, rl, dev):
    """ONE window: plo_depth_add_dev on the window's records beside plo_records_index_dev on the same records (the same walk of every CIGAR
    without atomics); then plo_depth_finish_dev, plo_depth_windows_dev and plo_depth_runs_dev beside a device-to-device copy of the array's
    bytes.  The array is checked against numpy's: differences by np.add.at from every counted record's ops, depths by cumsum"""
    import numpy as np
    import torch

    from portello_amd import abi, api, depth, devbatch
    from portello_amd.gather import device_view

    eng = api.Engine(index)
    b, f, r = win.batch_raw()
    up = devbatch.upload_raw_window(b, f, r, dev)
    torch.cuda.synchronize()
    ddesc = up.batch.desc()
    sa_in, keep = devbatch.sa_inputs(rn, dev)
    labels = devbatch.contig_labels(cn, dev)
    rin = up.records_in(labels, False)
    out = eng.liftover_batch_dev(ddesc)
    eng.compact_output_dev(out)
    eng.finish_batch_dev(ddesc, up.finish_in())
    eng.sa_segments_dev(sa_in)
    ro = eng.records_build_dev(ddesc, rin)
    n, nb, n_ref = int(ro.n_records), int(ro.n_bytes), len(rn)
    so = eng.records_sort_dev(ro.bytes, nb, n, ro.record_off, n_ref)  # (the index call wants them sorted; the depth does not care)

    def down(ptr, count, dtype):
        return device_view(ptr, count * np.dtype(dtype).itemsize, torch.uint8, dev).cpu().numpy().view(dtype) if count else np.zeros(0, dtype)

    obj = depth.DeviceDepth(eng, rl, count_deletions=a.depth_deletions)
    info = obj.info()
    n_entries = int(info.n_entries)
    slot = np.ctypeslib.as_array(info.slot_off, (n_ref + 1,)).astype(np.int64)
    # the expected array, from the rule (records of this workload carry their CIGAR in the record: none has more than 65 535 ops)
    data, off = down(so.bytes, nb, np.uint8), down(so.record_off, n + 1, np.uint64).astype(np.int64)
    diff = np.zeros(n_entries, np.int64)
    n_ops = n_counted = n_atomics = 0
    for i in range(n):
        p = int(off[i])
        ref, pos = (int(x) for x in data[p + 4:p + 12].view("<i4"))
        lrn, ncig, flag = int(data[p + 12]), int(data[p + 16:p + 18].view("<u2")[0]), int(data[p + 18:p + 20].view("<u2")[0])
        n_ops += ncig
        if ref < 0 or pos < 0 or flag & abi.DEPTH_EXCLUDE_DEFAULT:
            continue
        n_counted += 1
        ops = data[p + 36 + lrn:p + 36 + lrn + 4 * ncig].view("<u4").astype(np.int64)
        ln, code = ops >> 4, ops & 15
        rlen = np.where(np.isin(code, (0, 2, 3, 7, 8)), ln, 0)
        start = slot[ref] + pos + np.cumsum(rlen) - rlen
        cov = (ln > 0) & (np.isin(code, (0, 7, 8)) | ((code == 2) & bool(a.depth_deletions)))
        np.add.at(diff, start[cov], 1)
        np.add.at(diff, (start + rlen)[cov], -1)
        cons = cov[rlen > 0]  # the stretches: runs of covering ops among the reference-consuming ones
        n_atomics += 2 * int((cons & ~np.concatenate([[False], cons[:-1]])).sum())
    ao = obj.add(eng, so.bytes, nb, n, so.record_off)
    same = int(ao.n_counted) == n_counted and np.array_equal(obj.array(eng), diff.astype(np.int32))
    obj.finish(eng)
    want = np.cumsum(diff)
    same = same and np.array_equal(obj.array(eng), want.astype(np.int32))
    first, sums, _ = obj.windows(eng, a.depth_window)
    exp_sums = np.concatenate([np.add.reduceat(want[slot[r_]:slot[r_] + rl[r_]], np.arange(0, rl[r_], a.depth_window)) for r_ in range(n_ref) if rl[r_]] or [np.zeros(0, np.int64)])
    same = same and np.array_equal(sums, exp_sums.astype(np.uint64))
    runs = obj.runs(eng)
    exp_runs = sum(1 + int((want[slot[r_] + 1:slot[r_] + rl[r_]] != want[slot[r_]:slot[r_] + rl[r_] - 1]).sum()) for r_ in range(n_ref) if rl[r_])
    same = same and len(runs) == exp_runs and int((runs["end"] - runs["beg"]).sum()) == int(sum(rl))
    add_ms, index_ms, finish_ms, windows_ms, runs_ms = [], [], [], [], []
    for k in range(a.warmup + a.reps):
        obj.reset(eng)
        ao = obj.add(eng, so.bytes, nb, n, so.record_off)
        io = eng.records_index_dev(so.bytes, nb, n, so.record_off, n_ref)
        fms = obj.finish(eng)
        _, _, wms = obj.windows(eng, a.depth_window)
        rms = float(obj.runs_dev(eng).runs_ms)
        if k >= a.warmup:
            add_ms.append(float(ao.add_ms))
            index_ms.append(float(io.index_ms))
            finish_ms.append(fms)
            windows_ms.append(wms)
            runs_ms.append(rms)
    bytes_allocated = int(obj.info().bytes_allocated)
    obj.close()
    src, dst = torch.zeros(max(16, 4 * n_entries), dtype=torch.uint8, device=dev), torch.empty(max(16, 4 * n_entries), dtype=torch.uint8, device=dev)
    d2d = []
    for k in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src, non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        if k >= a.warmup:
            d2d.append(e0.elapsed_time(e1))
    eng.close()
    res = {"leg": "depth", "reads": win.n_records, "n_records": n, "n_counted": n_counted, "n_cigar_ops": n_ops, "n_atomics": n_atomics, "count_deletions": bool(a.depth_deletions),
           "n_ref": n_ref, "array_entries": n_entries, "array_bytes": 4 * n_entries, "bytes_allocated": bytes_allocated, "window": a.depth_window, "n_windows": int(len(sums)), "n_runs": int(len(runs)),
           "matches_numpy": bool(same), "add_ms": stats(add_ms), "index_ms_same_records": stats(index_ms), "finish_ms": stats(finish_ms), "windows_ms": stats(windows_ms),
           "runs_ms": stats(runs_ms), "d2d_copy_of_array_ms": stats(d2d),
           "note": "add_ms: check + add kernels (HIP events); index_ms: plo_records_index_dev, the same walk of every CIGAR without atomics; the copy moves array_bytes in and out (2 x array_bytes), the three-phase scan moves 3 x array_bytes"}
    return res, bool(same)


def pileup_leg(a, win, index, cn, rn, chrom_seq, dev):
    """ONE window: plo_pileup_add_dev on the window's records beside plo_nm_dev on the same window (the same base pairs walked, no scattered
    atomics) and plo_depth_add_dev on the same records; plo_pileup_sites_dev beside a device-to-device copy of the array's bytes.  Before
    anything is timed the array and the sites are compared with numpy's (tests/pileup_expect.py, counts_numpy): every non-zero base of the
    array comes down as a site of the mask 0xFF, and the array's sum and its count of non-zero counters are taken on the device"""
    import numpy as np
    import torch

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
    import pileup_expect as px

    from portello_amd import abi, api, depth, devbatch, pileup
    from portello_amd.gather import device_view

    eng = api.Engine(index)
    b, f, r = win.batch_raw()
    up = devbatch.upload_raw_window(b, f, r, dev)
    torch.cuda.synchronize()
    ddesc = up.batch.desc()
    sa_in, keep = devbatch.sa_inputs(rn, dev)
    labels = devbatch.contig_labels(cn, dev)
    rin = up.records_in(labels, False)
    out = eng.liftover_batch_dev(ddesc)
    eng.compact_output_dev(out)
    eng.finish_batch_dev(ddesc, up.finish_in())
    eng.sa_segments_dev(sa_in)
    ro = eng.records_build_dev(ddesc, rin)
    n, nb, n_ref = int(ro.n_records), int(ro.n_bytes), len(rn)
    chroms = [x.cpu().numpy() for x in chrom_seq]
    rl = [len(c) for c in chroms]

    def down(ptr, count, dtype):
        return device_view(ptr, count * np.dtype(dtype).itemsize, torch.uint8, dev).cpu().numpy().view(dtype) if count else np.zeros(0, dtype)

    data, off = down(ro.bytes, nb, np.uint8), down(ro.record_off, n + 1, np.uint64).astype(np.int64)
    keys, counts, n_counted, n_events, per_channel = px.counts_numpy(data, off, chroms)
    obj = pileup.DevicePileup(eng, rl)
    dobj = depth.DeviceDepth(eng, rl)
    info = obj.info()
    n_bases = int(info.n_bases)
    ao = obj.add(ro, eng)
    same = (int(ao.n_counted), int(ao.n_events)) == (n_counted, n_events)
    arr = device_view(info.array, 32 * n_bases, torch.uint8, dev).view(torch.int32)
    same = same and int(arr.sum(dtype=torch.int64)) == n_events and int(torch.count_nonzero(arr)) == len(keys)
    every = obj.sites(channel_mask=0xFF, engine=eng)  # every base with a non-zero counter
    got = ((every["ref_id"].astype(np.int64)[:, None] << 40) | (every["pos"].astype(np.int64)[:, None] << 3) | np.arange(8)[None, :])[every["count"] != 0]
    same = same and np.array_equal(got, keys) and np.array_equal(every["count"][every["count"] != 0], counts)
    same = same and all(int(s["ref_base"]) == int(chroms[int(s["ref_id"])][int(s["pos"])]) for s in every[::max(1, len(every) // 1000)])
    dobj.add(eng, ro.bytes, nb, n, ro.record_off)
    dobj.finish(eng)
    sites = obj.sites(dobj, min_count=2, min_frac=(1, 5), engine=eng)
    add_ms, nm_ms, depth_ms, sites_ms = [], [], [], []
    for k in range(a.warmup + a.reps):
        obj.reset(eng)
        dobj.reset(eng)
        ao = obj.add(ro, eng)
        do = dobj.add(eng, ro.bytes, nb, n, ro.record_off)
        no = eng.nm_dev(ddesc)
        dobj.finish(eng)
        so = obj.sites_dev(dobj, min_count=2, min_frac=(1, 5), engine=eng)
        if k >= a.warmup:
            add_ms.append(float(ao.add_ms))
            depth_ms.append(float(do.add_ms))
            nm_ms.append(float(no.nm_ms))
            sites_ms.append(float(so.sites_ms))
    same = same and int(so.n_sites) == len(sites)
    bytes_allocated = int(obj.info().bytes_allocated)
    obj.close()
    dobj.close()
    src, dst = torch.zeros(max(16, 32 * n_bases), dtype=torch.uint8, device=dev), torch.empty(max(16, 32 * n_bases), dtype=torch.uint8, device=dev)
    d2d = []
    for k in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src, non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        if k >= a.warmup:
            d2d.append(e0.elapsed_time(e1))
    eng.close()
    res = {"leg": "pileup", "reads": win.n_records, "n_records": n, "n_counted": n_counted, "n_events": n_events, "events_per_record": n_events / max(1, n_counted),
           "event_share_by_channel": {name: per_channel[k] / max(1, n_events) for k, name in enumerate(abi.PILEUP_CHANNEL_NAMES)}, "n_ref": n_ref, "array_bases": n_bases,
           "array_bytes": 32 * n_bases, "bytes_allocated": bytes_allocated, "bases_with_an_event": int(len(every)), "n_sites_min2_frac_1_5": int(len(sites)), "matches_numpy": bool(same),
           "add_ms": stats(add_ms), "nm_ms_same_window": stats(nm_ms), "depth_add_ms_same_records": stats(depth_ms), "sites_ms": stats(sites_ms), "d2d_copy_of_array_ms": stats(d2d),
           "note": "add_ms: check + add kernels (HIP events); nm_ms: plo_nm_dev, the same base pairs without scattered atomics; the copy moves array_bytes in and out, the sites "
                   "call reads array_bytes twice (count, emit) and 4 bytes a base of the depth array",
           "not_measured": ["a whole-genome array (99 GB)", "deep pile-ups on one cache line (many reads mismatching at one base)", "adds of several contexts timed together"]}
    return res, bool(same)


def abi_entry_dtype():
    from portello_amd import abi

    return abi.INDEX_ENTRY_DTYPE


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=50_000)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=540, help="seconds before the process ends itself")
    ap.add_argument("--out", default="")
    ap.add_argument("--commit", default="", help="commit hash to record (a tree without .git cannot tell)")
    ap.add_argument("--e2e-reads", type=int, default=0, help="> 0: also run_bam_to_bam device_finish against device_records on that many reads, three runs each, alternating")
    ap.add_argument("--level", type=int, default=1, help="BGZF level of the compress step beside level 0 (the device has one deflate level: 1)")
    ap.add_argument("--bgzf-out", default="", help="run the compress step (plo_bgzf_compress_dev) and write its JSON there")
    ap.add_argument("--batch-out", default="", help="run the batch-construction leg (plo_batch_build_dev) alone and write its JSON there")
    ap.add_argument("--cut-out", default="", help="run the input leg (plo_bgzf_inflate_dev + plo_window_cut_dev) alone and write its JSON there")
    ap.add_argument("--part-out", default="", help="run the part leg (plo_part_start_dev and the first cut of part 1 of 2 against plo_bam_open_range) alone and write its JSON there")
    ap.add_argument("--nm-out", default="", help="run the NM leg (plo_nm_dev beside the window's lift, finish and records times, against a device-to-device copy) alone and write its JSON there")
    ap.add_argument("--md-out", default="", help="run the MD leg (plo_md_dev beside the window's nm, lift, finish and records times, against a device-to-device copy) and write its JSON there; alone or behind --nm-out")
    ap.add_argument("--eqx-out", default="", help="run the = / X leg (plo_eqx_dev beside the window's nm, md, lift, finish and records times, against a device-to-device copy) and write its JSON there; alone or behind --nm-out / --md-out")
    ap.add_argument("--sort-out", default="", help="run the sort leg (plo_records_sort_dev on the window's records, against the host's expected order and a device-to-device copy of n_bytes) alone and write its JSON there")
    ap.add_argument("--index-out", default="", help="run the index leg (plo_records_index_dev on the window's sorted records, against the host's entries and a device-to-device copy of its algorithmic bytes; the writer's and the merge's index on the CPU) alone and write its JSON there")
    ap.add_argument("--merge-out", default="", help="run the merge leg (--merge-windows windows sorted and retained on the device; plo_runs_merge_plan_dev and the summed plo_runs_merge_emit_dev against plo_records_sort_dev over their concatenation and a device-to-device copy of the same bytes) alone and write its JSON there")
    ap.add_argument("--depth-out", default="", help="run the depth leg (plo_depth_add_dev beside plo_records_index_dev on the same records; finish, windows and runs beside a device-to-device copy of the array) alone and write its JSON there")
    ap.add_argument("--pileup-out", default="", help="run the pileup leg (plo_pileup_add_dev beside plo_nm_dev on the same window and plo_depth_add_dev on the same records; plo_pileup_sites_dev beside a device-to-device copy of the array) alone and write its JSON there")
    ap.add_argument("--depth-window", type=int, default=500, help="window size of the depth leg")
    ap.add_argument("--depth-deletions", action="store_true", help="the depth leg counts D as covered")
    ap.add_argument("--merge-windows", type=int, default=4, help="windows of the merge leg: --reads is cut into that many")
    ap.add_argument("--merge-chunk-bytes", type=int, default=1 << 30, help="chunk_bytes of the merge leg's plan")
    a = ap.parse_args()
    signal.alarm(a.limit)

    import numpy as np
    import torch

    from portello_amd import abi, api, bam, bamsynth, build, devbatch, synth

    dev = torch.device("cuda", 0)
    w = synth.generate(synth.config("chr20", n_reads=a.reads), device="cuda")
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "reads.bam")
    meta = bamsynth.write_read_bam(w, path, level=0, n_threads=8, n_unmapped=0)
    ixd = w.index_data()
    index = api.Index(w.index_data_device())
    cn, rn = meta["contig_names"], bamsynth.ref_names(w)
    rd = bam.BamReader(path, 8)
    if a.merge_out:
        mres, ok = merge_leg(a, rd, index, cn, rn, dev)
        rd.close()
        os.makedirs(os.path.dirname(os.path.abspath(a.merge_out)), exist_ok=True)
        with open(a.merge_out, "w") as fh:
            fh.write(json.dumps(mres, indent=1) + "\n")
        print(json.dumps(mres))
        sys.exit(0 if ok else 1)
    win = rd.read_window(a.reads + 10)
    assert win.n_records == a.reads
    if a.part_out:
        win.close()
        rd.close()
        pres, ok = part_leg(a, path, index)
        os.makedirs(os.path.dirname(os.path.abspath(a.part_out)), exist_ok=True)
        with open(a.part_out, "w") as fh:
            fh.write(json.dumps(pres, indent=1) + "\n")
        print(json.dumps(pres))
        sys.exit(0 if ok else 1)
    if a.cut_out:
        win.close()
        rd.close()
        cres, ok = cut_leg(a, path, index, dev)
        os.makedirs(os.path.dirname(os.path.abspath(a.cut_out)), exist_ok=True)
        for part in ("window", "end_to_end"):
            if part == "end_to_end":
                if a.e2e_reads <= 0:
                    break
                cres["end_to_end"] = end_to_end_cut(a.e2e_reads)
            with open(a.cut_out, "w") as fh:
                fh.write(json.dumps(cres, indent=1) + "\n")
        print(json.dumps(cres))
        sys.exit(0 if ok else 1)
    if a.pileup_out:
        pres, ok = pileup_leg(a, win, index, cn, rn, w.chrom_seq, dev)
        win.close()
        rd.close()
        os.makedirs(os.path.dirname(os.path.abspath(a.pileup_out)), exist_ok=True)
        with open(a.pileup_out, "w") as fh:
            fh.write(json.dumps(pres, indent=1) + "\n")
        print(json.dumps(pres))
        sys.exit(0 if ok else 1)
    if a.depth_out:
        dres, ok = depth_leg(a, win, index, cn, rn, [int(x.numel()) for x in w.chrom_seq], dev)
        win.close()
        rd.close()
        os.makedirs(os.path.dirname(os.path.abspath(a.depth_out)), exist_ok=True)
        with open(a.depth_out, "w") as fh:
            fh.write(json.dumps(dres, indent=1) + "\n")
        print(json.dumps(dres))
        sys.exit(0 if ok else 1)
    if a.index_out:
        ires, ok = index_leg(a, win, index, cn, rn, [int(x.numel()) for x in w.chrom_seq], dev)
        win.close()
        rd.close()
        os.makedirs(os.path.dirname(os.path.abspath(a.index_out)), exist_ok=True)
        with open(a.index_out, "w") as fh:
            fh.write(json.dumps(ires, indent=1) + "\n")
        print(json.dumps(ires))
        sys.exit(0 if ok else 1)
    if a.sort_out:
        sres, ok = sort_leg(a, win, index, cn, rn, dev)
        win.close()
        rd.close()
        os.makedirs(os.path.dirname(os.path.abspath(a.sort_out)), exist_ok=True)
        with open(a.sort_out, "w") as fh:
            fh.write(json.dumps(sres, indent=1) + "\n")
        print(json.dumps(sres))
        sys.exit(0 if ok else 1)
    if a.nm_out or a.md_out or a.eqx_out:
        ok = True
        for path_out, leg in ((a.nm_out, nm_leg), (a.md_out, md_leg), (a.eqx_out, eqx_leg)):
            if not path_out:
                continue
            res, leg_ok = leg(a, win, index, cn, rn, dev)
            ok = ok and leg_ok
            os.makedirs(os.path.dirname(os.path.abspath(path_out)), exist_ok=True)
            with open(path_out, "w") as fh:
                fh.write(json.dumps(res, indent=1) + "\n")
            print(json.dumps(res))
        win.close()
        rd.close()
        sys.exit(0 if ok else 1)
    if a.batch_out:
        bres, ok = batch_leg(a, win, index, cn, dev)
        os.makedirs(os.path.dirname(os.path.abspath(a.batch_out)), exist_ok=True)
        for part in ("window", "end_to_end"):  # the window's figures are on disk before the long runs start
            if part == "end_to_end":
                if a.e2e_reads <= 0:
                    break
                win.close()
                rd.close()
                bres["end_to_end"] = end_to_end_batch(a.e2e_reads)
            with open(a.batch_out, "w") as fh:
                fh.write(json.dumps(bres, indent=1) + "\n")
        print(json.dumps(bres))
        sys.exit(0 if ok else 1)

    def device_route(bytecopy):
        if bytecopy:
            os.environ["PLO_RECORDS_BYTECOPY"] = "1"
        else:
            os.environ.pop("PLO_RECORDS_BYTECOPY", None)
        eng = api.Engine(index)
        b, f, r = win.batch_raw()
        h2d = []
        for _ in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            t = time.perf_counter()
            up = devbatch.upload_raw_window(b, f, r, dev)
            torch.cuda.synchronize()
            h2d.append((time.perf_counter() - t) * 1e3)
        ddesc = up.batch.desc()
        out = eng.liftover_batch_dev(ddesc)
        eng.compact_output_dev(out)
        fo = eng.finish_batch_dev(ddesc, up.finish_in())
        sa_in, keep = devbatch.sa_inputs(rn, dev)
        so = eng.sa_segments_dev(sa_in)
        labels = devbatch.contig_labels(cn, dev)
        rin = up.records_in(labels, False)
        from portello_amd.gather import device_view

        ms, d2h = [], []
        land = None  # ONE page-locked block, made before the timed copies
        for k in range(a.warmup + a.reps):
            ro = eng.records_build_dev(ddesc, rin)
            if land is None:
                land = torch.empty(max(16, int(ro.n_bytes)), dtype=torch.uint8, pin_memory=True)
            src = device_view(ro.bytes, int(ro.n_bytes), torch.uint8, dev)
            torch.cuda.synchronize()
            t = time.perf_counter()
            land[:int(ro.n_bytes)].copy_(src, non_blocking=True)  # the copy of `bytes` alone
            torch.cuda.synchronize()
            if k >= a.warmup:
                ms.append(float(ro.records_ms))
                d2h.append((time.perf_counter() - t) * 1e3)
        bgzf = {}
        if a.bgzf_out and not bytecopy:  # the records stay where plo_records_build_dev left them
            import zlib

            raw = land[:int(ro.n_bytes)].numpy()
            for lv in sorted({0, a.level}):
                zms, zd2h, bland = [], [], None
                for k in range(a.warmup + a.reps):
                    bo = eng.bgzf_compress_dev(ro.bytes, int(ro.n_bytes), lv)
                    if bland is None:
                        bland = torch.empty(max(16, int(bo.n_bytes)), dtype=torch.uint8, pin_memory=True)
                    src = device_view(bo.blocks, int(bo.n_bytes), torch.uint8, dev)
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    bland[:int(bo.n_bytes)].copy_(src, non_blocking=True)
                    torch.cuda.synchronize()
                    if k >= a.warmup:
                        zms.append(float(bo.bgzf_ms))
                        zd2h.append((time.perf_counter() - t) * 1e3)
                off = eng.download(bo.block_off, np.uint64, int(bo.n_blocks) + 1)
                blk = bland[:int(bo.n_bytes)].numpy()
                same = all(zlib.decompress(blk[int(off[i]):int(off[i + 1])].tobytes(), 31) == raw[i * 0xff00:(i + 1) * 0xff00].tobytes() for i in range(int(bo.n_blocks)))
                bgzf[f"level_{lv}"] = {"bgzf_ms": stats(zms), "d2h_blocks_ms": stats(zd2h), "blocks_bytes": int(bo.n_bytes), "n_blocks": int(bo.n_blocks),
                                      "ratio": int(bo.n_bytes) / max(1, int(ro.n_bytes)), "payload_gbs": int(ro.n_bytes) / (statistics.median(zms) * 1e-3) / 1e9,
                                      "inflates_to_the_records": bool(same)}
        rec = devbatch.DeviceRecords(ro, dev=dev, with_offsets=True)
        host = devbatch.HostResults(eng, out, fo, so, win.n_records, dev=dev)
        return dict(eng=eng, up=up, rec=rec, host=host, ms=ms, d2h=d2h, h2d=h2d[a.warmup:], fin_ms=float(fo.finish_ms) + float(fo.revcomp_ms) + float(so.sa_ms), keep=(keep, labels), bgzf=bgzf)

    vec = device_route(False)
    # the yardstick on the same window and the same lift result (the dense batch of plo_bam_window_batch, as the device_finish mode builds it)
    desc, fin_in = win.batch_desc(with_finish=True)
    host_ms = []
    for k in range(a.warmup + a.reps):
        t = time.perf_counter()
        rb = win.build_records_finished_raw(vec["host"].lift, vec["host"].fin, vec["host"].sa, ixd.to_desc(), cn, rn, False, a.threads)
        if k >= a.warmup:
            host_ms.append((time.perf_counter() - t) * 1e3)
    hdata = C.string_at(rb.bytes, rb.n_bytes)
    hoff = np.ctypeslib.as_array(rb.record_off, shape=(int(rb.n_records) + 1,)).copy()
    ok = vec["rec"].data() == hdata and np.array_equal(vec["rec"].record_off, hoff) and vec["rec"].n_lifted == int(rb.n_lifted)
    # H2D of the separate seq + qual arrays the raw upload replaces
    sq = []
    for _ in range(a.warmup + a.reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        up2 = devbatch.upload_window(desc, fin_in, dev)
        torch.cuda.synchronize()
        sq.append((time.perf_counter() - t) * 1e3)
    del up2
    byte = device_route(True)
    ok = ok and byte["rec"].data() == hdata
    n_bytes = len(hdata)
    med = statistics.median(vec["ms"])
    res = {
        "tool": "tools/bench_records.py", "reads": a.reads, "records": int(rb.n_records), "record_bytes": n_bytes, "raw_window_bytes": int(vec["up"].raw_bytes),
        "commit": a.commit or subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip() or None, "source_hash": build.source_hash(),
        "warmup": a.warmup, "reps": a.reps, "bytes_equal_host": bool(ok),
        "host_records_build_finished_ms": dict(stats(host_ms), threads=a.threads),
        "device_records_ms": stats(vec["ms"]), "device_records_bytecopy_ms": stats(byte["ms"]),
        "device_gbs_read_plus_written": 2.0 * n_bytes / (med * 1e-3) / 1e9, "copy_ceiling_gbs": COPY_CEILING_GBS,
        "gbs_note": "2 x record bytes over records_ms (plan, scans and emit): an approximation -- the reads of SA text, reversed bases, CIGARs and plans are not counted; the ceiling is the guide's measured float4 copy",
        "d2h_record_bytes_ms": stats(vec["d2h"]), "h2d_raw_window_ms": stats(vec["h2d"]), "h2d_separate_seq_qual_batch_ms": stats(sq[a.warmup:]),
        "finish_and_sa_ms_once": vec["fin_ms"],
    }
    res["device_kernel_plus_d2h_ms"] = res["device_records_ms"]["median"] + res["d2h_record_bytes_ms"]["median"]
    res["device_below_host"] = res["device_kernel_plus_d2h_ms"] < res["host_records_build_finished_ms"]["median"]
    if a.bgzf_out:
        # the 16-thread host writer on the same bytes, BGZF blocks only (a file on the temporary directory's filesystem)
        hw = {}
        for lv in sorted({0, a.level}):
            ts = []
            for k in range(3):
                wp = os.path.join(tmp, "host_writer.bam")
                wr = bam.BamWriter(wp, "@HD\tVN:1.6\n", ["c"], [1], level=lv, n_threads=16)
                t = time.perf_counter()
                wr.write(hdata)
                wr.close()
                ts.append((time.perf_counter() - t) * 1e3)
                size = os.path.getsize(wp)
                os.unlink(wp)
            hw[f"level_{lv}"] = {"write_ms": stats(ts), "file_bytes": size, "payload_gbs": n_bytes / (statistics.median(ts) * 1e-3) / 1e9, "threads": 16}
        zres = {"tool": "tools/bench_records.py", "reads": a.reads, "record_bytes": n_bytes, "commit": res["commit"], "source_hash": res["source_hash"], "warmup": a.warmup,
                "reps": a.reps, "d2h_record_bytes_ms": res["d2h_record_bytes_ms"], "device_records_ms": res["device_records_ms"], "device": vec["bgzf"], "host_writer": hw}
        ok = ok and all(v["inflates_to_the_records"] for v in vec["bgzf"].values())
        os.makedirs(os.path.dirname(os.path.abspath(a.bgzf_out)), exist_ok=True)
        for part in ("window", "end_to_end"):  # the window's figures are on disk before the long runs start
            if part == "end_to_end":
                if a.e2e_reads <= 0:
                    break
                zres["end_to_end"] = end_to_end_bgzf(a.e2e_reads, a.level)
            with open(a.bgzf_out, "w") as fh:
                fh.write(json.dumps(zres, indent=1) + "\n")
        print(json.dumps(zres))
    elif a.e2e_reads > 0:
        res["end_to_end"] = end_to_end(a.e2e_reads)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
