"""CPU: the MS-SSIM training loss (mcquic_amd.loss; reference mcquic/loss/__init__.py:47-55) -- a float64 autograd restatement
built from oracle/metrics_ref.py against F17 (tests/golden/f17_msssim_loss.npz, captured from the reference's own
validate/metrics.py in float32 and float64), the torch fallback of `loss.MsSSIM`, the formatters and `step_loss`'s arithmetic.
The restatement is what tests/test_gpu_msssim_loss.py measures the HIP kernels against."""
import hashlib
import os

import numpy as np
import pytest
import torch

from oracle import metrics_ref as M

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CROP_ROWS, CROP_COLS, NPROJ = 48, 128, 4


def f17():
    return np.load(os.path.join(G, "f17_msssim_loss.npz"))


def f17_inputs(seed: int, n: int, h: int, w: int):
    """(restored, image) float32 of an F17 case (tests/golden/make_golden_msssim_loss.py)."""
    image_u8, target_u8 = M.make_u8_pair(seed, n, h, w)
    image = image_u8.float() / 127.5 - 1
    target = target_u8.float() / 127.5 - 1
    noise = torch.from_numpy(np.random.default_rng(seed).normal(0.0, 0.01, tuple(image.shape)).astype(np.float32))
    return target + noise, image


def f17_directions(seed: int, shape):
    rng = np.random.default_rng(seed + 1000)
    return [rng.standard_normal(shape) for _ in range(NPROJ)]


def ms_ssim_loss64(restored: torch.Tensor, image: torch.Tensor, offset: float = 1.0, data_range: float = 2.0):
    """float64 restatement: (1 - MS-SSIM(restored + offset, image + offset) over the batch, v [5, N, C] before the relu)."""
    x, y = restored.double() + offset, image.double() + offset
    win = M.gauss_window().double()
    weights = torch.tensor(M.MS_WEIGHTS).double()                        # float32 weights, as the reference module holds them
    vs = []
    for lv in range(5):
        s, cs = M.ssim_and_cs(x, y, win, data_range=data_range)
        vs.append(cs if lv < 4 else s)
        if lv < 4:
            x, y = M._halve(x), M._halve(y)
    v = torch.stack(vs)                                                  # [5, N, C]
    value = torch.prod(torch.relu(v) ** weights.view(-1, 1, 1), dim=0).mean()
    return 1.0 - value, v


def grads64(restored: torch.Tensor, image: torch.Tensor, wrt_image: bool = False):
    """(loss, v, d loss / d restored [, d loss / d image]) in float64."""
    r = restored.detach().double().requires_grad_()
    i = image.detach().double().requires_grad_(wrt_image)
    loss, v = ms_ssim_loss64(r, i)
    loss.backward()
    return loss.detach(), v.detach(), r.grad, (i.grad if wrt_image else None)


def _sha(t):
    return hashlib.sha256(t.contiguous().numpy().tobytes()).hexdigest()


def test_restatement_reproduces_f17():
    z = f17()
    for i, (seed, n, h, w) in enumerate(z["cases"].tolist()):
        restored, image = f17_inputs(seed, n, h, w)
        assert bytes(z[f"sha_{i}"]).hex() == _sha(restored) + _sha(image), "F17 inputs are not reproduced"
        loss, v, g, _ = grads64(restored, image)
        assert abs(float(loss) - float(z[f"loss64_{i}"][0])) <= 1e-12
        crop = g[0, 0, :CROP_ROWS, :CROP_COLS].numpy()
        want = z[f"crop64_{i}"]
        np.testing.assert_allclose(crop, want, rtol=0, atol=1e-12 * float(np.abs(want).max()))
        proj = np.array([float((d * g.numpy()).sum()) for d in f17_directions(seed, tuple(g.shape))])
        np.testing.assert_allclose(proj, z[f"proj64_{i}"], rtol=1e-9, atol=0)
        assert v.shape == (5, n, 3) and bool((v > 0).all())


def test_cpu_fallback_matches_reference_float32():
    from mcquic_amd import loss as L
    z = f17()
    for i, (seed, n, h, w) in enumerate(z["cases"].tolist()):
        restored, image = f17_inputs(seed, n, h, w)
        got = L.MsSSIM()(restored, image)
        assert got.dim() == 0 and got.dtype == torch.float32
        assert abs(float(got) - float(z[f"loss32_{i}"][0])) <= 1e-6
        assert abs(float(got) - float(z[f"loss64_{i}"][0])) <= 2e-6
        r = restored.clone().requires_grad_()
        L.MsSSIM()(r, image).backward()
        np.testing.assert_allclose(r.grad[0, 0, :CROP_ROWS, :CROP_COLS].numpy(), z[f"crop32_{i}"], rtol=0,
                                   atol=1e-3 * float(np.abs(z[f"crop32_{i}"]).max()))


def test_formatters_and_step_loss_follow_the_reference():
    from mcquic_amd import loss as L
    seed, n, h, w = 1, 2, 176, 208
    restored, image = f17_inputs(seed, n, h, w)
    ms, ps = L.MsSSIM(), L.PSNR()
    d = ms(restored, image)
    assert torch.equal(ms.formatDistortion(d), -10 * (d / 1.0).log10())              # Decibel(1.0)
    m = ps(restored, image)
    assert torch.equal(m, torch.nn.functional.mse_loss(restored, image))
    assert torch.equal(ps.formatDistortion(m), -10 * (m / 4.0).log10())               # Decibel(2.0)
    fn = L.step_loss()
    got = fn((restored, None, None, None), image)
    assert torch.equal(got, 0.5 * d + 0.5 * torch.nn.functional.mse_loss(restored, image))   # trainer.py:276 without LPIPS
    got2 = L.step_loss(L.PSNR(), 0.25, 0.75)((restored,), image)
    assert torch.equal(got2, 0.25 * m + 0.75 * m)


def test_small_sides_are_refused():
    from mcquic_amd import loss as L
    x = torch.zeros(1, 3, 160, 200)
    with pytest.raises(ValueError):
        L.MsSSIM()(x, x)
