#!/usr/bin/env python3
"""Times the load of a reference FASTA on the device (plo_fasta_load_file): python tools/bench_fasta.py --bases N --width 60 --out profiles/r17_fasta.json

Writes a synthetic reference of N bases (it downloads nothing), checks the loaded chromosomes against tests/fasta_expect.py on a sample of
positions and every length, then times, after warm-up loads,
  fasta_ms            the kernels of all pieces, summed (HIP events, plo_fasta_out::fasta_ms)
  load_wall_ms        the wall time of plo_fasta_load_file
  read_only_wall_ms   the wall time of only reading the same file into two page-locked buffers of the same piece size (the floor of the load)
  d2d_copy_ms         a device-to-device copy of text_bytes in the same process (the floor of a pass over the text)
and reports fasta_ms / d2d_copy_ms and load_wall_ms / read_only_wall_ms.  No ratio is asserted."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(v):
    s = sorted(v)
    return {"median": s[len(s) // 2], "min": s[0], "max": s[-1], "n": len(s)}


def write_reference(path, bases, width, lower_frac, n_chroms, seed):
    import numpy as np

    from portello_amd import bamsynth

    rng = np.random.default_rng(seed)
    share = np.array([2.0 ** -k for k in range(n_chroms)])  # chromosomes of falling length, like a genome's
    lens = np.maximum(1, (bases * share / share.sum()).astype(np.int64))
    lens[0] += bases - int(lens.sum())
    alphabet = np.frombuffer(b"ACGTN", np.uint8)

    class W:
        chrom_seq = [alphabet[rng.integers(0, 5, int(n), dtype=np.uint8)] for n in lens]

    bamsynth.write_reference_fasta(W, path, width=width, lower_frac=lower_frac)
    return W.chrom_seq


def read_only(path, piece_bytes, bufs):
    """the file into the two page-locked buffers in turn, as plo_fasta_load_file reads it"""
    t0 = time.perf_counter()
    n, k = 0, 0
    with open(path, "rb", buffering=0) as fh:
        while True:
            got = fh.readinto(bufs[k])
            if not got:
                break
            n += got
            k ^= 1
    return (time.perf_counter() - t0) * 1e3, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bases", type=int, default=200_000_000)
    ap.add_argument("--width", type=int, default=60)
    ap.add_argument("--lower-frac", type=float, default=0.3)
    ap.add_argument("--chroms", type=int, default=6)
    ap.add_argument("--piece-bytes", type=int, default=0, help="0: the library's (16 MiB)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sample", type=int, default=200_000, help="positions compared per chromosome besides its ends")
    ap.add_argument("--dir", default=None, help="where the synthetic file goes (default: a temporary directory)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    import fasta_expect as fx
    from portello_amd import api, build, fasta

    assert torch.cuda.is_available(), "bench_fasta.py needs a GPU"
    tmp = tempfile.TemporaryDirectory(dir=a.dir)
    path = os.path.join(tmp.name, "ref.fa")
    seqs = write_reference(path, a.bases, a.width, a.lower_frac, a.chroms, 17)
    text_bytes = os.path.getsize(path)
    names, lens = [f"chr{i + 1}" for i in range(len(seqs))], [len(s) for s in seqs]

    # the check: every length, the head of the file against the expectation byte for byte, a sample of positions of every chromosome
    head_bytes = min(text_bytes, 300_000)
    head = fx.load(open(path, "rb").read(head_bytes).rsplit(b"\n", 1)[0] + b"\n")
    ref = fasta.load_reference(path, names, lens, piece_bytes=a.piece_bytes)
    ok = ref.chrom_len == lens and ref.record_lens == lens and ref.stats["n_bases"] == sum(lens) and ref.stats["text_bytes"] == text_bytes
    rng = np.random.default_rng(3)
    got0 = ref.download(0)
    ok = ok and head.err_kind == 0 and got0[: len(head.seqs[0])].tobytes() == head.seqs[0]
    compared = len(head.seqs[0])
    for c, s in enumerate(seqs):
        got = got0 if c == 0 else ref.download(c)
        pos = np.unique(np.concatenate([rng.integers(0, len(s), min(a.sample, len(s))), np.arange(min(64, len(s))), len(s) - 1 - np.arange(min(64, len(s)))]))
        ok = ok and bool(np.array_equal(got[pos], s[pos]))  # (the synthetic bases are upper case; the file soft-masks a fraction of them)
        compared += len(pos)
    ref.close()
    if not ok:
        print(json.dumps({"tool": "tools/bench_fasta.py", "ok": False}))
        sys.exit(1)

    L = api.load_library()
    piece = a.piece_bytes or (16 << 20)
    bufs = []
    for _ in range(2):
        p = C.c_void_p()
        assert L.plo_host_alloc(piece, C.byref(p)) == 0
        bufs.append((p, (C.c_uint8 * piece).from_address(p.value)))
    fasta_ms, load_ms, read_ms = [], [], []
    for k in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        ref = fasta.load_reference(path, names, lens, piece_bytes=a.piece_bytes)
        t1 = time.perf_counter()
        ms = ref.stats["fasta_ms"]
        ref.close()
        r_ms, n = read_only(path, piece, [b[1] for b in bufs])
        assert n == text_bytes
        if k >= a.warmup:
            fasta_ms.append(ms)
            load_ms.append((t1 - t0) * 1e3)
            read_ms.append(r_ms)
    for p, _ in bufs:
        L.plo_host_free(p)
    dev = torch.device("cuda", 0)
    src, dst = torch.zeros(text_bytes, dtype=torch.uint8, device=dev), torch.empty(text_bytes, dtype=torch.uint8, device=dev)
    d2d = []
    for k in range(a.warmup + a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src, non_blocking=True)
        e1.record()
        torch.cuda.synchronize()
        if k >= a.warmup:
            d2d.append(e0.elapsed_time(e1))
    med = lambda v: sorted(v)[len(v) // 2]
    res = {"tool": "tools/bench_fasta.py", "ok": True, "bases": int(sum(lens)), "text_bytes": text_bytes, "width": a.width, "lower_frac": a.lower_frac, "chroms": len(seqs),
           "piece_bytes": piece, "tile_bytes": None, "byte_stores": os.environ.get("PLO_FASTA_BYTESTORES", "0") not in ("", "0"), "positions_compared": int(compared),
           "commit": a.commit or subprocess.run(["git", "rev-parse", "HEAD"], capture_output=True, text=True, cwd=ROOT).stdout.strip() or None,
           "source_hash": build.source_hash(), "warmup": a.warmup, "reps": a.reps, "fasta_ms": stats(fasta_ms), "load_wall_ms": stats(load_ms),
           "read_only_wall_ms": stats(read_ms), "d2d_copy_ms": stats(d2d), "fasta_ms_over_d2d_copy": med(fasta_ms) / med(d2d),
           "load_wall_over_read_only_wall": med(load_ms) / med(read_ms), "fasta_gbs_of_text": text_bytes / med(fasta_ms) / 1e6,
           "load_wall_gbs_of_text": text_bytes / med(load_ms) / 1e6,
           "not_measured": "a real 3.1 GB reference (none is on the machines); a cold page cache (the file was written just before it is read)"}
    try:
        import emu_fasta_lib

        res["tile_bytes"] = emu_fasta_lib.tile()
    except Exception:
        pass
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
