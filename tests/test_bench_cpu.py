"""bench.py's options without a GPU: what a plain run includes, and the sampling of --dump-outputs."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_secondary_measurements_only_with_full():
    a = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert not a.full and a.dump_outputs is None and a.steps == 3 and a.warmup == 1
    assert bench.parse_args(["--full", "--dump-outputs", "d"]).full


def test_dump_outputs_whole_when_it_fits(tmp_path):
    arrays = {"a": np.arange(10, dtype=np.int64), "b": np.linspace(0.0, 1.0, 7)}
    bench.dump_outputs(str(tmp_path), arrays)
    assert sorted(p.name for p in tmp_path.iterdir()) == ["a.npy", "b.npy"]
    for k, want in arrays.items():
        got = np.load(tmp_path / (k + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, want)


def test_dump_outputs_fixed_sample_over_budget(tmp_path):
    rng = np.random.default_rng(5)
    arrays = {"x": rng.standard_normal(5000), "i": rng.integers(0, 1 << 40, 3000)}
    budget = 16000
    for d in ("one", "two"):
        bench.dump_outputs(str(tmp_path / d), arrays, budget=budget)
    total = 0
    for k, a in arrays.items():
        idx = np.load(tmp_path / "one" / (k + "_sample_idx.npy"))
        got = np.load(tmp_path / "one" / (k + ".npy"))
        assert got.dtype == np.float64 and np.all(np.diff(idx) > 0)
        assert np.array_equal(got, a[idx.astype(np.int64)].astype(np.float64))
        assert np.array_equal(idx, np.load(tmp_path / "two" / (k + "_sample_idx.npy")))  # the same positions every run
        total += got.nbytes + idx.nbytes
    assert total <= budget
