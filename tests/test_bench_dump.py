"""bench.py --dump-outputs: the writer's formats and its size budget (no GPU; the end-to-end run is
tests/test_gpu_engine.py::test_bench_plain_line_and_dump_outputs)."""
import os

import numpy as np

import bench


def test_dump_outputs_dtypes_and_values(tmp_path):
    arrays = {"state": np.arange(-42, 42, dtype=np.int8).reshape(2, 42),
              "probs": np.linspace(0, 1, 14, dtype=np.float32).reshape(2, 7),
              "q": np.array([1 / 3, -2 / 3], dtype=np.float64),
              "game": np.array([2 ** 40 + 1, 7], dtype=np.int64),
              "none": np.zeros((0, 7), dtype=np.float32)}
    shapes = bench.dump_outputs(str(tmp_path / "d"), arrays)
    assert sorted(os.listdir(tmp_path / "d")) == sorted(k + ".npy" for k in arrays)
    for k, a in arrays.items():
        b = np.load(tmp_path / "d" / (k + ".npy"))
        assert b.dtype == (np.float64 if a.dtype.itemsize == 8 else np.float32), k
        assert list(b.shape) == shapes[k] == list(a.shape) and np.array_equal(b, a), k  # exact, 2**40 + 1 included


def test_dump_outputs_budget_takes_the_same_rows_every_time(tmp_path):
    big = np.arange(4096 * 16, dtype=np.float32).reshape(4096, 16)
    small = np.arange(8, dtype=np.float64)
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), {"big": big, "small": small}, budget=2 * 64 * 100)
    a, b = (np.load(tmp_path / n / "big.npy") for n in ("a", "b"))
    assert a.shape == (100, 16) and np.array_equal(a, b)  # 100 rows of 64 bytes fill half the budget
    rows = a[:, 0].astype(int) // 16
    assert np.all(np.diff(rows) > 0) and np.array_equal(a, big[rows])  # whole rows, in order, none twice
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), small)
    assert sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in os.listdir(tmp_path / "a")) <= 2 * 64 * 100
