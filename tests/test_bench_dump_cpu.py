"""-m "not gpu": bench.dump_outputs, the writer behind `bench.py --dump-outputs`: float32 files, small arrays whole, large ones as the same
seeded sample of flat indices in every run, a byte budget checked before anything is written."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_dump_writes_float32_and_samples_large_arrays_the_same_way_every_time(tmp_path):
    import bench
    n = bench.DUMP_MAX_ELEMS + 12345
    big = torch.arange(n, dtype=torch.float64)
    small = torch.arange(12, dtype=torch.int32).reshape(3, 4)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"big": big, "small": small, "absent": None})
    assert sorted(os.listdir(tmp_path / "a")) == ["big.npy", "small.npy"]
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and s.shape == (3, 4) and np.array_equal(s, small.numpy())
    ba, bb = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert ba.dtype == np.float32 and ba.shape == (bench.DUMP_MAX_ELEMS,) and np.array_equal(ba, bb)
    idx = ba.astype(np.int64)            # (values = flat indices: exact in float32 below 2**24)
    assert (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < n


def test_dump_refuses_more_than_its_budget_before_writing(tmp_path):
    import bench
    arrays = {f"a{i}": torch.zeros(bench.DUMP_MAX_ELEMS) for i in range(bench.DUMP_MAX_BYTES // (4 * bench.DUMP_MAX_ELEMS) + 1)}
    with pytest.raises(RuntimeError, match="budget"):
        bench.dump_outputs(str(tmp_path / "d"), arrays)
    assert not os.path.exists(tmp_path / "d")
