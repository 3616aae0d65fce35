"""bench.py --dump-outputs: what the timed path returned, as DIR/<name>.npy in float32 / float64, under 64 MB in all,
the same sample on every run.  CPU test on host tensors: the writer itself, not the GPU path that feeds it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_types_sample_and_budget(tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(bench, "DUMP_BYTES", 3 * 4096 * 4)      # a share of 4096 float32 / 2048 float64 per array
    small = torch.arange(24, dtype=torch.int32).reshape(2, 3, 4)
    big = torch.randperm(40 * 50 * 60, generator=torch.Generator().manual_seed(1)).float().reshape(40, 50, 60)
    wide = torch.rand(5000, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), [("small", small), ("big", big), ("wide", wide), ("none", None)])
    assert sorted(os.listdir(tmp_path / "a")) == ["big.npy", "small.npy", "wide.npy"]
    s, b, w = (np.load(tmp_path / "a" / (k + ".npy")) for k in ("small", "big", "wide"))
    assert s.dtype == np.float32 and s.shape == (2, 3, 4) and np.array_equal(s, small.numpy())
    assert b.dtype == np.float32 and b.shape == (4096,) and np.isin(b, big.numpy().ravel()).all()
    assert len(np.unique(b)) == 4096
    assert w.dtype == np.float64 and w.shape == (2048,) and np.isin(w, wide.numpy()).all()
    for k in ("small", "big", "wide"):
        assert np.array_equal(np.load(tmp_path / "a" / (k + ".npy")), np.load(tmp_path / "b" / (k + ".npy")))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) < 64 * 10 ** 6


def test_plain_run_is_lean_by_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 3, 1)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert (a.full, a.dump_outputs) == (True, "out")
