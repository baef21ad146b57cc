"""bench.py --dump-outputs: the files two builds are compared by.  Whole arrays when they fit the budget, otherwise the same seeded sample of
elements on every run; float32 unless the array is float64; never more than the budget on disk."""
import os

import numpy as np
import torch

import bench


def _bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_small_outputs_are_written_whole(tmp_path):
    comp = torch.rand(2, 5, 7, 3) * 255
    info = bench.dump_outputs(str(tmp_path), {"composite": comp, "mask": torch.ones(3, 4, dtype=torch.uint8), "x64": torch.ones(2, dtype=torch.float64)})
    got = np.load(tmp_path / "composite.npy")
    assert got.dtype == np.float32 and got.shape == (2, 5, 7, 3) and np.array_equal(got, comp.numpy())
    assert np.load(tmp_path / "mask.npy").dtype == np.float32
    assert np.load(tmp_path / "x64.npy").dtype == np.float64
    assert not any(v["sampled"] for v in info.values())


def test_large_outputs_are_a_fixed_sample_within_the_budget(tmp_path):
    limit = 64 * 1024
    comp = torch.arange(80 * 24 * 43 * 3, dtype=torch.float32).view(80, 24, 43, 3)      # 990 KB of float32: over the budget
    a, b = tmp_path / "a", tmp_path / "b"
    info = bench.dump_outputs(str(a), {"composite": comp}, limit=limit)
    bench.dump_outputs(str(b), {"composite": comp.clone()}, limit=limit)
    assert info["composite"]["sampled"] and info["composite"]["shape"] == [80, 24, 43, 3]
    assert _bytes(a) <= limit
    x, y = np.load(a / "composite.npy"), np.load(b / "composite.npy")
    assert x.dtype == np.float32 and x.size == info["composite"]["elements"] > limit // 8
    assert np.array_equal(x, y)                                      # same positions from run to run
    assert np.all(np.diff(x) > 0) and np.all(x == np.round(x))      # values of the array at ascending flat positions


def test_the_default_budget_is_64_mb():
    assert bench.DUMP_LIMIT == 64 * 2 ** 20
