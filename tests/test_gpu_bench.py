"""bench.py's contract on the GPU: one JSON line with the metric of
BASELINE.json, a positive whole-job value, the attention-kernel roofline
(--full) and the config fields the driver reads (a short run: 3 timed steps);
a plain run leaves the extra measurements out and --dump-outputs writes the
last step's outputs, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--steps", "3", "--warmup", "1",
                        "--cpu-baseline", "off", *args], capture_output=True, text=True, timeout=300, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_default_line():
    d = _bench("--full")
    base = json.load(open(os.path.join(REPO, "BASELINE.json")))
    assert d["metric"] == base["metric"]
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["higher_is_better"] is True
    assert abs(d["value"] - 64 * 1000.0 / d["ms_per_step"]) / d["value"] < 1e-3  # B=64 tokens per step
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and 0 < r["frac"] < 1
    assert abs(r["achieved"] / r["peak"] - r["frac"]) < 1e-3
    c = d["config"]
    assert c["global_batch"] == 64 and c["seq_len"] == 1024 and c["page_size"] == 16 and c["hip_graph"]


def test_bench_small_batch_split_attention_line():
    """B=8 (the per-GPU batch of strong scaling at N=8): the split-context
    attention is in use and the line is well formed"""
    d = _bench("--full", "--batch", "8")
    assert d["config"]["global_batch"] == 8 and d["config"]["attn_splits"] >= 2
    assert d["value"] > 0 and 0 < d["roofline"]["frac"] < 1


def test_bench_plain_run_is_lean_and_dumps_repeatable_outputs(tmp_path):
    """without --full the line carries the headline figure only (no roofline
    timing, no CPU baseline); --dump-outputs writes the last timed step's
    logits and next ids as float .npy files, identical between two runs of
    the same arguments, and --steps sets how far the decode went"""
    def run(name, steps):
        r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps),
                            "--warmup", "1", "--spinup", "0.1", "--batch", "8", "--dump-outputs",
                            str(tmp_path / name)], capture_output=True, text=True, timeout=300, cwd=REPO)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, r.stdout[-2000:]
        d = json.loads(lines[0])
        out = {f[:-4]: np.load(tmp_path / name / f) for f in sorted(os.listdir(tmp_path / name))}
        return d, out
    d, a = run("a", 3)
    base = json.load(open(os.path.join(REPO, "BASELINE.json")))
    assert d["metric"] == base["metric"] and d["unit"] == "tokens/s" and d["higher_is_better"] is True
    assert d["dtype"] == "fp32" and d["steps"] == 3 and d["ms_per_step"] > 0 and d["full"] is False
    assert abs(d["value"] - 8 * 1000.0 / d["ms_per_step"]) / d["value"] < 1e-3
    assert d["roofline"] is None and d["cpu_baseline"] is None
    assert sorted(a) == ["logits", "next_ids"]
    assert a["logits"].shape == (8, 50257) and a["logits"].dtype == np.float32
    assert a["next_ids"].shape == (8,) and a["next_ids"].dtype == np.float64
    assert np.isfinite(a["logits"]).all()
    assert np.array_equal(a["next_ids"], a["logits"].argmax(-1))  # greedy: the ids are the logits' argmax
    _, b = run("b", 3)
    assert all(np.array_equal(a[k], b[k]) for k in a)
    _, c = run("c", 4)  # one more timed step: another position, other logits
    assert not np.array_equal(a["logits"], c["logits"])


@pytest.mark.parametrize("n", [2, 8])
def test_bench_default_multi_gpu_line_is_the_metric(n):
    """the default N>1 line (rehearsed on one GPU with --emulate-rank N) is the
    headline metric: B = 64 split over the N ranks (BASELINE.md section 3's
    2/4/8-GPU rows), so value, global_batch and the metric string agree"""
    d = _bench("--emulate-rank", str(n))
    base = json.load(open(os.path.join(REPO, "BASELINE.json")))
    c, e = d["config"], d["emulated_rank"]
    assert d["metric"] == base["metric"] and d["scaling"] == "strong"
    assert c["global_batch"] == 64 and c["batch_per_gpu"] == 64 // n and "configs[1]" in c["workload"]
    assert e["rows"] == 64 // n and e["global_batch"] == 64
    # value = this GPU's rows; the projection = all N ranks' rows at this step time
    assert abs(d["value"] - (64 // n) * 1000.0 / d["ms_per_step"]) / d["value"] < 1e-3
    assert abs(e["projected_n_gpu_tokens_per_s"] * d["ms_per_step"] / 64000.0 - 1) < 1e-2
    assert "1-rank RCCL communicator" in e["gather"]  # rank 0's gather runs in the timed steps
    assert d["status"] == 0


def test_bench_weak_line_is_labelled_config4():
    """--scaling weak at N>1 (64 sequences per rank) is BASELINE configs[3],
    reported under its own metric string, never the headline's"""
    d = _bench("--emulate-rank", "2", "--scaling", "weak")
    base = json.load(open(os.path.join(REPO, "BASELINE.json")))
    assert d["metric"] != base["metric"] and "per GPU" in d["metric"]
    assert d["config"]["global_batch"] == 128 and "configs[3]" in d["config"]["workload"]
