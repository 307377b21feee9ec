"""bench.dump_outputs (bench.py --dump-outputs) on the CPU: small outputs are written whole, large
ones as the entries at fixed seeded positions, the same in every call; always float .npy files."""
import types

import numpy as np
import torch

import bench


def fake_problem(n):
    x = torch.arange(n, dtype=torch.float32)
    return types.SimpleNamespace(patterns_local=lambda: x.reshape(-1, 1), loss_hist=[3.0, 2.0, 1.5])


def test_small_output_is_written_whole(tmp_path):
    bench.dump_outputs(str(tmp_path / "a" / "b"), fake_problem(1000))
    pat = np.load(tmp_path / "a" / "b" / "patterns.npy")
    loss = np.load(tmp_path / "a" / "b" / "loss.npy")
    assert pat.dtype == np.float32 and np.array_equal(pat, np.arange(1000, dtype=np.float32))
    assert loss.dtype == np.float64 and loss.tolist() == [3.0, 2.0, 1.5]


def test_large_output_is_a_fixed_sample(tmp_path):
    n = bench.DUMP_MAX + 12345
    bench.dump_outputs(str(tmp_path / "one"), fake_problem(n))
    bench.dump_outputs(str(tmp_path / "two"), fake_problem(n))
    one = np.load(tmp_path / "one" / "patterns.npy")
    two = np.load(tmp_path / "two" / "patterns.npy")
    assert one.dtype == np.float32 and one.shape == (bench.DUMP_MAX,) and one.nbytes <= 64 << 20
    assert np.array_equal(one, two)
    # entries of the array itself (value = position), spread over all of it
    assert one.min() >= 0 and one.max() < n and one.max() > 0.99 * n and len(np.unique(one)) > 0.5 * bench.DUMP_MAX
