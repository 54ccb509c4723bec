"""CPU: the float64 reference of the training input transform (tests/_augment_ref.py) against ATen.

torchvision is not a dependency of this project; F.interpolate(mode="bilinear", antialias=True, align_corners=False) on the
crop is what torchvision's RandomResizedCrop calls for tensors, and ATen's CPU kernel takes float64, so the resampler is
pinned to it at 1e-12."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _augment_ref as R

# (box h, box w) -> (H, W): whole-image-like, up on both axes, 2.7x down on one axis and up on the other, one-pixel boxes,
# odd reductions, same size
CASES = [((61, 83), (32, 48)), ((20, 30), (32, 48)), ((87, 40), (32, 48)), ((25, 130), (32, 48)), ((1, 83), (32, 48)),
         ((61, 1), (32, 48)), ((61, 83), (61, 83)), ((61, 83), (130, 70)), ((57, 79), (31, 45)), ((96, 80), (64, 64))]


@pytest.mark.parametrize("box,size", CASES)
def test_resampler_matches_aten(box, size):
    g = torch.Generator().manual_seed(box[0] * 1000 + box[1])
    crop = torch.rand((3,) + box, generator=g, dtype=torch.float64)
    want = F.interpolate(crop[None], size, mode="bilinear", antialias=True, align_corners=False)[0].numpy()
    got = R.resample(crop.numpy(), size)
    err = float(np.abs(got - want).max())
    assert err <= 1e-12, f"box {box} -> {size}: max |diff| {err:.3e}"


def test_same_size_is_the_identity():
    crop = np.random.default_rng(0).random((3, 17, 23))
    assert np.array_equal(R.resample(crop, (17, 23)), crop)


def test_pipeline_off_is_clamp_and_normalise():
    x = np.random.default_rng(1).random((2, 3, 9, 11)) * 1.6 - 0.3
    got = R.pipeline(x, (9, 11), R.identity_params(2, (9, 11)))
    assert np.array_equal(got, (np.clip(x, 0.0, 1.0) - 0.5) / 0.5)
    p = R.identity_params(2, (9, 11))
    p[:, R.HFLIP] = 1
    p[1, R.VFLIP] = 1
    got = R.pipeline(x, (9, 11), p)
    want = (np.clip(x, 0.0, 1.0) - 0.5) / 0.5
    assert np.array_equal(got[0], want[0][:, :, ::-1]) and np.array_equal(got[1], want[1][:, ::-1, ::-1])
