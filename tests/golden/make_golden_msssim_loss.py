#!/usr/bin/env python3
"""Capture F17 (tests/golden/f17_msssim_loss.npz): the MS-SSIM TRAINING loss of the REAL reference
(mcquic/loss/__init__.py:47-55 -> mcquic/validate/metrics.py `MsSSIM(data_range=2.0, sizeAverage=True)` on restored + 1,
image + 1), imported unmodified from the reference tree the way make_golden.py does for F7, run on CPU autograd in float32
and in float64.  Runs only where the reference tree is; the output is data (seeds, hashes, losses, gradient samples).

    python tests/golden/make_golden_msssim_loss.py

Inputs: `image, target = metrics_ref.make_u8_pair(seed, n, h, w)`, both mapped to u8 / 127.5 - 1 (float32), and
`restored = target + N(0, 0.01)` drawn from np.random.default_rng(seed) (float32).  Stored per case i:
    loss32_i, loss64_i     the reference's loss in float32 / float64
    crop32_i, crop64_i     d loss / d restored of image 0, channel 0, rows 0..47, columns 0..127
    proj64_i [4]           the float64 gradient projected on four directions N(0, 1) of np.random.default_rng(seed + 1000)
    rel32_i                || g32 - g64 || / || g64 ||: the reference's own float32 gradient error
    sha_i                  sha256 of the float32 restored and image bytes
"""
import hashlib
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import metrics_ref as M         # noqa: E402  (generators only; expected values come from the reference)
from oracle import ref_harness              # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
F17_CASES = [(1, 2, 176, 208), (2, 4, 256, 256), (3, 1, 161, 333)]       # (seed, n, h, w), 3 channels
CROP_ROWS, CROP_COLS, NPROJ = 48, 128, 4


def inputs(seed: int, n: int, h: int, w: int):
    """(restored, image) float32 [n, 3, h, w] of case `seed` (shared with the tests)."""
    image_u8, target_u8 = M.make_u8_pair(seed, n, h, w)
    image = image_u8.float() / 127.5 - 1
    target = target_u8.float() / 127.5 - 1
    noise = torch.from_numpy(np.random.default_rng(seed).normal(0.0, 0.01, tuple(image.shape)).astype(np.float32))
    return target + noise, image


def directions(seed: int, shape):
    rng = np.random.default_rng(seed + 1000)
    return [rng.standard_normal(shape) for _ in range(NPROJ)]


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


def main():
    spec = importlib.util.spec_from_file_location("ref_metrics", os.path.join(ref_harness.REF, "mcquic/validate/metrics.py"))
    RM = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(RM)
    f17 = {"cases": np.array(F17_CASES, dtype=np.int64)}
    for i, (seed, n, h, w) in enumerate(F17_CASES):
        restored, image = inputs(seed, n, h, w)
        grads = {}
        for tag, dt in (("32", torch.float32), ("64", torch.float64)):
            ssim = RM.MsSSIM(data_range=2.0, sizeAverage=True).to(dt)         # mcquic/loss/__init__.py:50
            r = restored.detach().to(dt).clone().requires_grad_()
            loss = ssim(r + 1, image.to(dt) + 1)                              # mcquic/loss/__init__.py:53
            loss.backward()
            f17[f"loss{tag}_{i}"] = np.array([loss.item()], dtype=np.float64)
            grads[tag] = r.grad.double().numpy()
            f17[f"crop{tag}_{i}"] = r.grad[0, 0, :CROP_ROWS, :CROP_COLS].numpy().astype(np.float32 if tag == "32" else np.float64)
        g64, g32 = grads["64"], grads["32"]
        f17[f"proj64_{i}"] = np.array([float((d * g64).sum()) for d in directions(seed, g64.shape)], dtype=np.float64)
        f17[f"rel32_{i}"] = np.array([np.linalg.norm(g32 - g64) / np.linalg.norm(g64)], dtype=np.float64)
        f17[f"sha_{i}"] = np.frombuffer(bytes.fromhex(sha(restored) + sha(image)), dtype=np.uint8)
        print(f"case {i}: loss32 {f17[f'loss32_{i}'][0]:.9g} loss64 {f17[f'loss64_{i}'][0]:.12g} rel32 {f17[f'rel32_{i}'][0]:.3e}")
    path = os.path.join(OUT, "f17_msssim_loss.npz")
    np.savez_compressed(path, **f17)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
