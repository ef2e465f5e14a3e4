"""Record assembly of ONE window on the device against the host builder: one process, one context, a time limit of its own.

For a chr20 window of --reads reads held in memory, JSON with
  - the yardstick: wall time of plo_records_build_finished with --threads host threads (what the pipeline's device_finish mode does);
  - plo_records_build_dev: records_ms (HIP events), bytes read + written per records_ms, the D2H time of the record bytes, the H2D time
    of the raw window against the H2D of the separate seq + qual arrays it replaces;
  - the byte-copy instantiation (PLO_RECORDS_BYTECOPY=1, a context of its own) against the 16-byte one.
Exits non-zero on any byte mismatch between the device's records and the host's.

    python tools/bench_records.py --reads 50000 --out profiles/r07_records_window.json
"""
import argparse
import ctypes as C
import json
import os
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
    win = rd.read_window(a.reads + 10)
    assert win.n_records == a.reads

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
        rec = devbatch.DeviceRecords(ro, dev=dev, with_offsets=True)
        host = devbatch.HostResults(eng, out, fo, so, win.n_records, dev=dev)
        return dict(eng=eng, up=up, rec=rec, host=host, ms=ms, d2h=d2h, h2d=h2d[a.warmup:], fin_ms=float(fo.finish_ms) + float(fo.revcomp_ms) + float(so.sa_ms), keep=(keep, labels))

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
    if a.e2e_reads > 0:
        res["end_to_end"] = end_to_end(a.e2e_reads)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
