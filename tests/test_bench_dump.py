"""bench.py --dump-outputs: the writer (CPU; the GPU run of bench.py is tests/test_gpu_sweep.py's)."""
import numpy as np
import torch

import bench


def test_dump_outputs_rows_float32(tmp_path):
    lat = torch.arange(3 * 4 * 5, dtype=torch.float64).reshape(3, 4, 5)
    maps = torch.arange(3 * 2, dtype=torch.bfloat16).reshape(3, 2)
    bench.dump_outputs(str(tmp_path / "d"), [1, 2], {"lat": lat, "maps": maps})
    a, b = np.load(tmp_path / "d" / "lat.npy"), np.load(tmp_path / "d" / "maps.npy")
    assert a.dtype == np.float32 and b.dtype == np.float32
    assert np.array_equal(a, lat[1:].float().numpy()) and np.array_equal(b, maps[1:].float().numpy())


def test_dump_outputs_sample_is_fixed_and_within_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 64 << 10)
    big = torch.randn(2, 100000, generator=torch.Generator().manual_seed(3))
    small = torch.ones(2, 7)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), [0, 1], {"big": big, "small": small})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.ndim == 1 and 0 < a.size < big.numel() and np.array_equal(a, b)      # the same sample each time
    assert np.isin(a, big.numpy()).all()
    assert np.load(tmp_path / "a" / "small.npy").shape == (2, 7)                    # small results whole
    total = sum(f.stat().st_size for f in (tmp_path / "a").iterdir())
    assert total <= 64 << 10
