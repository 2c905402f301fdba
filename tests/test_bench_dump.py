"""bench.py --dump-outputs: the arrays of the last timed step as DIR/<name>.npy, float32 / float64, at most 64 MB in all, the same
sample from run to run; and `--steps` is the number of timed steps the result line reports."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _sizes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_small_outputs_are_written_whole(tmp_path):
    snap = bench.snapshot_outputs({"img": torch.arange(24, dtype=torch.float32).reshape(2, 3, 4),
                                   "radii": torch.tensor([0, 3, 7], dtype=torch.int32), "mask": torch.tensor([True, False]),
                                   "loss": torch.tensor(0.25, dtype=torch.float64), "half": torch.tensor([1.5], dtype=torch.float16),
                                   "none": None})
    bench.dump_outputs(str(tmp_path), snap)
    assert sorted(os.listdir(tmp_path)) == ["half.npy", "img.npy", "loss.npy", "mask.npy", "radii.npy"]
    img = np.load(tmp_path / "img.npy")
    assert img.dtype == np.float32 and img.shape == (2, 3, 4) and np.array_equal(img.ravel(), np.arange(24))
    assert np.load(tmp_path / "radii.npy").dtype == np.float32 and np.array_equal(np.load(tmp_path / "radii.npy"), [0, 3, 7])
    assert np.array_equal(np.load(tmp_path / "mask.npy"), [1.0, 0.0])
    loss = np.load(tmp_path / "loss.npy")
    assert loss.dtype == np.float64 and loss.shape == () and loss == 0.25
    assert np.load(tmp_path / "half.npy").dtype == np.float32


def test_large_outputs_are_a_fixed_sample_under_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 3_000_000)
    monkeypatch.setattr(bench, "DUMP_WHOLE_BYTES", 100_000)
    g = torch.Generator().manual_seed(0)
    P = 60_000
    named = {"color": torch.rand(3, 256, 256, generator=g), "grad_sh": torch.rand(P, 16, 3, generator=g),
             "grad_opacity": torch.rand(P, 1, generator=g), "small": torch.rand(100, generator=g)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), bench.snapshot_outputs(named))
        assert _sizes(tmp_path / d) <= 3_000_000
    for f in os.listdir(tmp_path / "a"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), named["small"].numpy())
    # per-Gaussian arrays keep whole rows, in order, the same rows for arrays of the same length
    sh, op = np.load(tmp_path / "a" / "grad_sh.npy"), np.load(tmp_path / "a" / "grad_opacity.npy")
    assert sh.shape[1:] == (16, 3) and 0 < sh.shape[0] < P and sh.shape[0] == op.shape[0]
    rows = [int(np.flatnonzero((named["grad_opacity"].numpy()[:, 0] == v))[0]) for v in op[:50, 0]]
    assert rows == sorted(rows)
    assert np.array_equal(sh[:50], named["grad_sh"].numpy()[rows])
    color = np.load(tmp_path / "a" / "color.npy")
    assert color.ndim == 1 and 0 < color.size < 3 * 256 * 256


def _run_bench(args, out_dir, env_extra=None):
    env = dict(os.environ, **(env_extra or {}))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--no-cpu-baseline", "--no-extra",
                        "--dump-outputs", str(out_dir)] + args, env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_dumps_the_c3_step(tmp_path):
    d = _run_bench(["--steps", "3", "--warmup", "1"], tmp_path)
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    names = sorted(f[:-4] for f in os.listdir(tmp_path))
    assert names == ["alpha", "color", "grad_means3D", "grad_opacity", "grad_rotations", "grad_scales", "grad_sh", "radii"]
    assert _sizes(tmp_path) <= 64_000_000
    assert all(np.load(tmp_path / f).dtype == np.float32 for f in os.listdir(tmp_path))
    # what the dump holds is what the same step computes in this process (radii and opacity gradient are small: written whole)
    sc = bench.Scene("C3", 0, 1, torch.device("cuda", 0))
    sc.one_step()
    torch.cuda.synchronize()
    want = sc.outputs()
    np.testing.assert_array_equal(np.load(tmp_path / "radii.npy"), want["radii"].float().cpu().numpy())
    util.assert_close("grad_opacity", np.load(tmp_path / "grad_opacity.npy"), want["grad_opacity"].cpu().numpy(), max_bad_frac=2e-4)


@pytest.mark.gpu
def test_bench_dumps_the_render_step(tmp_path):
    d = _run_bench(["--workload", "render", "--steps", "2", "--warmup", "1"], tmp_path, {"GSR_BENCH_P": "20000"})
    assert d["steps"] == 2 and d["ms_per_step"] > 0
    names = {f[:-4] for f in os.listdir(tmp_path)}
    assert {"render", "render_alpha", "normal", "loss", "radii", "grad__xyz"} <= names, names
    assert _sizes(tmp_path) <= 64_000_000
    assert np.isfinite(np.load(tmp_path / "loss.npy")).all()
