"""bench.py's command line: what a plain run prints, --dump-outputs (CPU: the sampling helper; GPU: a short run), and
the options that only make sense with --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

HEADLINE_KEYS = {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"}
FULL_ONLY_KEYS = {"roofline", "kernel_ms_per_step", "kernel_roofline_frac", "also", "cpu_baseline"}


def test_dump_outputs_whole_sampled_and_typed(tmp_path):
    g = torch.Generator().manual_seed(0)
    table = torch.arange(30000 * 300, dtype=torch.float32).view(30000, 300)
    arrays = {"loss": torch.tensor(0.5), "score": torch.randn(512, 5, generator=g).to(torch.bfloat16),
              "sums": torch.arange(5, dtype=torch.float64), "param.table": table, "flat": torch.arange(3_000_000.0)}
    bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(k + ".npy" for k in arrays)
    total = 0
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b), f          # same sample every run
        assert a.size <= bench.DUMP_MAX_VALUES, f
        total += a.nbytes
    assert total <= bench.DUMP_MAX_BYTES
    assert np.load(tmp_path / "a" / "sums.npy").dtype == np.float64
    assert np.load(tmp_path / "a" / "score.npy").shape == (512, 5)
    rows = np.load(tmp_path / "a" / "param.table.npy")
    assert rows.shape[1] == 300 and rows.shape[0] == bench.DUMP_MAX_VALUES // 300
    idx = rows[:, 0] / 300                                                                 # whole rows, in index order
    assert np.array_equal(rows, table.numpy()[idx.astype(np.int64)]) and np.all(np.diff(idx) > 0)
    flat = np.load(tmp_path / "a" / "flat.npy")
    assert flat.shape == (bench.DUMP_MAX_VALUES,) and np.all(np.diff(flat) > 0)


def test_all_kernels_needs_full():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--all-kernels"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--full" in r.stderr


@pytest.mark.gpu
def test_plain_run_prints_the_headline_only_and_dumps_the_same_outputs_every_run(tmp_path):
    lines = []
    for run in ("a", "b"):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                            "--dump-outputs", str(tmp_path / run)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    line = lines[0]
    assert HEADLINE_KEYS <= set(line) and not (FULL_ONLY_KEYS & set(line))
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert sorted(os.listdir(tmp_path / "a")) == ["loss.npy", "score.npy"]
    score = np.load(tmp_path / "a" / "score.npy")
    assert score.shape == (512, 5) and score.dtype == np.float32 and np.isfinite(score).all()
    assert np.isclose(float(np.load(tmp_path / "a" / "loss.npy")), line["config"]["final_loss"], atol=1e-4)
    # same seeded inputs, same computation: only the order of the backward's fp32 atomic adds may differ (bf16 compute)
    for f in ("loss.npy", "score.npy"):
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert np.allclose(a, b, rtol=1e-2, atol=1e-2 * float(np.abs(a).max())), f
