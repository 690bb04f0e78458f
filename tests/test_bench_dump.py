"""bench.py --dump-outputs DIR: what the timed path computed in its last step, as DIR/<name>.npy (float32, 64 MB at most)."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_write_outputs_keeps_small_arrays_whole_and_samples_past_the_budget(tmp_path, monkeypatch):
    import bench

    rng = np.random.default_rng(3)
    arrays = {"pred": rng.standard_normal(64).astype(np.float32), "grads": rng.standard_normal(3 << 20).astype(np.float32)}
    shapes = bench.write_outputs(str(tmp_path / "whole"), arrays)
    assert shapes == {"pred": [64], "grads": [3 << 20]}
    assert np.array_equal(np.load(tmp_path / "whole" / "grads.npy"), arrays["grads"])

    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 8 << 20)
    shapes = bench.write_outputs(str(tmp_path / "a"), arrays)
    bench.write_outputs(str(tmp_path / "b"), arrays)
    got = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in arrays}
    assert np.array_equal(got["pred"], arrays["pred"])  # small arrays stay whole
    assert sum(a.nbytes for a in got.values()) <= 8 << 20 and got["grads"].dtype == np.float32
    assert set(got["grads"].tolist()) <= set(arrays["grads"].tolist())
    assert np.array_equal(got["grads"], np.load(tmp_path / "b" / "grads.npy"))  # the same sample every run


@pytest.mark.gpu
def test_bench_dumps_the_last_timed_step(tmp_path):
    """A small headline-model run: prediction, loss, gradients and updated parameters of the last timed step land in DIR,
    float32, within 64 MB, and the line says so."""
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    d = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", "8", "--atoms", "20", "--no-cpu-baseline", "--streamed-steps", "0", "--no-micro",
                        "--other-configs", "0", "--dump-outputs", str(d)], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][0])
    assert out["steps"] == 3 and out["ms_per_step"] > 0
    # a plain run measures nothing beyond the headline (--full does)
    assert out["full"] is False and out["roofline"] is None and out["cpu_baseline"] is None and "other_configs" not in out
    files = {f[:-4]: np.load(d / f) for f in os.listdir(d)}
    assert set(files) == {"pred", "loss", "grads", "params"} == set(out["dumped_outputs"]["shapes"])
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in files.values())
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert files["pred"].shape == (8,) and files["loss"].shape == (1,)
    assert files["grads"].shape == files["params"].shape and np.abs(files["grads"]).max() > 0
    # the loss of the dumped step is the L1 distance of the dumped prediction from bench.py's seeded target
    import torch

    target = torch.randn(8, generator=torch.Generator().manual_seed(1)).numpy()
    assert abs(float(np.abs(files["pred"] - target).mean()) - float(files["loss"][0])) < 1e-5
