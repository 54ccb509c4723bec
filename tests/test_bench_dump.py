"""CPU: bench.py's --dump-outputs writer on an output of the headline's size (32 x 3 x 768 x 512): every level's codes whole,
the reconstructions as a seeded sample of DUMP_SAMPLE values (the same positions on every call), float32, 64 MB at most."""
import numpy as np
import torch

import bench


def _dump(directory, codes, pixels):
    bench.dump_outputs(str(directory), codes, pixels)
    return {p.name: np.load(p) for p in sorted(directory.iterdir())}


def test_dump_samples_a_large_reconstruction_at_fixed_positions(tmp_path):
    n, h, w = 32, 768, 512
    codes = [torch.randint(0, k, (n, 2, h // s, w // s), generator=torch.Generator().manual_seed(k))
             for k, s in ((8192, 16), (2048, 32), (512, 64))]
    pixels = torch.arange(n * 3 * h * w, dtype=torch.float64).reshape(n, 3, h, w)     # a value names its position
    a = _dump(tmp_path / "a", codes, pixels)
    b = _dump(tmp_path / "b", codes, pixels)
    assert sorted(a) == ["codes0.npy", "codes1.npy", "codes2.npy", "pixels.npy"]
    assert all(v.dtype == np.float32 for v in a.values()) and sum(v.nbytes for v in a.values()) <= 64 << 20
    for lv, c in enumerate(codes):
        assert np.array_equal(a[f"codes{lv}.npy"], c.numpy().astype(np.float32))
    s = a["pixels.npy"]
    assert s.shape == (bench.DUMP_SAMPLE,) and np.array_equal(s, b["pixels.npy"])
    pos = s.astype(np.int64)                                    # (exact: the positions a float32 holds are multiples of 1, 2 or 4)
    assert pos.min() >= 0 and pos.max() < pixels.numel() and (np.diff(pos) >= 0).all()
    assert np.unique(pos // (3 * h * w)).size == n              # every image is sampled


def test_dump_keeps_a_small_reconstruction_whole(tmp_path):
    codes = [torch.zeros((1, 2, 3, 4), dtype=torch.int64)]
    pixels = torch.rand((1, 3, 16, 16), generator=torch.Generator().manual_seed(0))
    a = _dump(tmp_path, codes, pixels)
    assert np.array_equal(a["pixels.npy"], pixels.reshape(-1).numpy())
