"""bench.py --dump-outputs: the files a step's fme_mv_result rows are written to."""
import os

import numpy as np

import bench
from nnfme.abi import MV_FIELDS, MV_RESULT_DTYPE


def _rows(n, seed=3):
    rng = np.random.default_rng(seed)
    rows = np.zeros(n, MV_RESULT_DTYPE)
    rows["mv_x"] = rng.integers(-2**15, 2**15, n)
    rows["mv_y"] = rng.integers(-2**15, 2**15, n)
    rows["cost"] = rng.integers(0, 2**32, n, dtype=np.uint64)
    rows["bits"] = rng.integers(0, 2**32, n, dtype=np.uint64)
    rows["nn_class"] = rng.integers(0, 49, n)
    rows["status"] = rng.integers(0, 2**16, n)
    return rows


def test_dump_is_exact_and_float(tmp_path):
    rows = _rows(1000)
    bench.dump_outputs(str(tmp_path / "d"), rows)
    assert sorted(os.listdir(tmp_path / "d")) == sorted(f + ".npy" for f in MV_FIELDS)
    for f in MV_FIELDS:
        a = np.load(tmp_path / "d" / (f + ".npy"))
        assert a.dtype in (np.float32, np.float64) and a.shape == (1000,)
        assert np.array_equal(a.astype(np.int64), rows[f].astype(np.int64)), f   # no field loses a bit


def test_dump_over_the_limit_is_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT", 4000)
    rows = _rows(1000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), rows, rank=1, world=2)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and all(n.startswith("rank1_") for n in names)
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert np.array_equal(a, b), n
        total += a.nbytes
    assert 0 < total <= 4000
    idx = np.load(tmp_path / "a" / "rank1_sample_index.npy").astype(np.int64)
    assert np.all(np.diff(idx) > 0) and idx[-1] < 1000
    assert np.array_equal(np.load(tmp_path / "a" / "rank1_cost.npy"), rows["cost"][idx].astype(np.float64))
