"""bench.py driver-contract tests (CPU): one JSON line, required fields."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent

REQUIRED = {
    "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
    "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
}


@pytest.mark.timeout(300)
@pytest.mark.parametrize("model", ["linear", "logistic", "ode"])
def test_bench_json_contract(model):
    proc = subprocess.run(
        [sys.executable, str(REPO / "bench.py"), "--model", model,
         "--steps", "3", "--warmup", "1"],
        capture_output=True, text=True, timeout=280, cwd=REPO,
    )
    assert proc.returncode == 0, proc.stderr[-500:]
    line = [l for l in proc.stdout.strip().splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert REQUIRED.issubset(d.keys()), REQUIRED - set(d.keys())
    assert d["metric"] == "logp+grad calls/sec (whole node)"
    assert d["higher_is_better"] is True
    assert d["scaling"] == "weak"
    assert d["data"] == "synthetic"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert d["n_gpus"] == 1
    assert "model" in d["config"] and "parallelism" in d["config"]


@pytest.mark.timeout(300)
def test_bench_multirank_gloo():
    # two gloo ranks on the CPU: hide the GPUs from the ranks, so the test
    # runs the same plumbing on a box with fewer GPUs than ranks
    env = dict(os.environ, HIP_VISIBLE_DEVICES="-1", CUDA_VISIBLE_DEVICES="-1")
    proc = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29671", str(REPO / "bench.py"),
         "--gpus", "2", "--steps", "3", "--warmup", "1", "--full"],
        capture_output=True, text=True, timeout=280, cwd=REPO, env=env,
    )
    assert proc.returncode == 0, proc.stderr[-500:]
    line = [l for l in proc.stdout.strip().splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2
    assert "x2" in d["config"]["parallelism"]
    assert d["config"]["device"] == "cpu"
    # --full carries the per-call all-reduce latency probe
    assert d["config"]["allreduce_us"] > 0


def _run_bench_dump(out_dir, steps):
    proc = subprocess.run(
        [sys.executable, str(REPO / "bench.py"), "--gpus", "1", "--rows", "4096",
         "--steps", str(steps), "--warmup", "1", "--dump-outputs", str(out_dir)],
        capture_output=True, text=True, timeout=280, cwd=REPO,
    )
    assert proc.returncode == 0, proc.stderr[-500:]
    line = [l for l in proc.stdout.strip().splitlines() if l.startswith("{")][-1]
    return json.loads(line), np.load(out_dir / "logp.npy"), np.load(out_dir / "grad.npy")


@pytest.mark.timeout(300)
def test_bench_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes the last timed step's [logp, grads]; seeded
    inputs make two runs with the same arguments agree bit for bit."""
    d1, logp1, grad1 = _run_bench_dump(tmp_path / "a", 3)
    d2, logp2, grad2 = _run_bench_dump(tmp_path / "b", 3)
    assert d1["steps"] == 3 and d1["ms_per_step"] > 0
    assert d1["config"]["allreduce_us"] is None  # plain run: no extra probes
    assert logp1.dtype == np.float64 and logp1.shape == ()
    assert grad1.dtype == np.float64 and grad1.shape == (2,)
    assert np.isfinite(logp1) and np.all(np.isfinite(grad1))
    np.testing.assert_array_equal(logp1, logp2)
    np.testing.assert_array_equal(grad1, grad2)
