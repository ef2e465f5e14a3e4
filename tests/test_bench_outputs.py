"""A plain `bench.py` run times the steps and prints the headline line only (the rest is `--full`); `--dump-outputs DIR` writes a sample
of the last step's result records that equals the oracle's records of the same read set."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_dumps_the_last_steps_records(tmp_path, oracle):
    from portello_amd import abi, pipeline, synth

    out = str(tmp_path / "out")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "chr20", "--reads", "30000", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", out], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    r = json.loads(lines[0])
    assert r["steps"] == 3 and r["warmup"] == 1 and r["ms_per_step"] > 0 and r["value"] > 0 and r["unit"] == "reads/s"
    for k in ("roofline", "cpu_baseline", "window_50k", "overlap", "end_to_end"):
        assert k not in r  # (--full only)

    d = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    assert all(a.dtype == np.float64 for a in d.values())
    assert sum(a.nbytes for a in d.values()) <= 64 << 20
    n_items, n_ops = d["counts"][0]
    assert n_items == r["config"]["items_per_gpu"]
    assert 0 < d["item_seg"].size <= n_items and d["cigar"].size == d["item_cigar_len"].sum()

    # the same read set (bench.py's seed for the workload) through the oracle: every sampled item, field for field
    w = synth.generate(synth.config("chr20", n_reads=30000), device="cuda")  # (generated where bench.py generates it)
    ref = oracle.liftover_batch(w.index_data(), w.batch_data(), abi.STAGES_ALL, pipeline.effective_cpus())
    assert ref.n_items == n_items and n_ops == int(ref.item_cigar_len.sum())
    row = {(int(s), int(c)): i for i, (s, c) in enumerate(zip(ref.item_seg, ref.item_cseg))}
    off = np.concatenate([[0], np.cumsum(d["item_cigar_len"].astype(np.int64))])
    for j in range(d["item_seg"].size):
        i = row[(int(d["item_seg"][j]), int(d["item_cseg"][j]))]
        for f in ("item_status", "item_need_flipped", "item_mapq", "item_chrom_index", "item_ref_pos", "item_cigar_len"):
            assert d[f][j] == getattr(ref, f)[i], (f, j)
        assert np.array_equal(d["cigar"][off[j]:off[j + 1]], ref.item_cigar(i).astype(np.float64)), j
