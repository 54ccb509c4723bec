"""Training losses of the reference (mcquic/loss/__init__.py): the `Distortion` / `Rate` bases, the `MsSSIM` and `PSNR`
distortions with their formatters, the `BasicRate` codebook regulariser, and `step_loss`, the reference trainer's objective for
`parallel.GraphedTrainStep` and eager loops.

On a HIP device in float32 the MS-SSIM distortion runs on this library's kernels (csrc/msssim_loss.hip, forward and backward:
no ATen launch and no memset node inside a captured step); elsewhere it is the reference's torch formula, as
`autograd.mse_loss` falls back to `F.mse_loss`.  `BasicRate` likewise: csrc/codebook_cos.hip on a HIP device in float32 (no
[k, k] plane, no ATen launch), the reference's formula elsewhere.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from . import ops
from .autograd import CodebookCosineFn, MsSsimFn, mse_loss

__all__ = ["BasicRate", "Decibel", "Distortion", "MsSSIM", "PSNR", "Rate", "ms_ssim_loss", "step_loss"]

_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)         # mcquic/validate/metrics.py:19


class Decibel(nn.Module):
    """mcquic/validate/utils.py Decibel: -10 log10(x / upperBound^2)."""

    def __init__(self, upperBound: float):
        super().__init__()
        self._upperBound = upperBound ** 2

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return -10 * (x / self._upperBound).log10()


class Distortion(nn.Module):
    """mcquic/loss/__init__.py:9-15: a distortion term with the formatter its value is logged through."""

    def __init__(self, formatter: nn.Module):
        super().__init__()
        self._formatter = formatter

    def formatDistortion(self, loss):
        return self._formatter(loss)


class Rate(nn.Module):
    """mcquic/loss/__init__.py:18-24: a rate term with its formatter."""

    def __init__(self, formatter: nn.Module):
        super().__init__()
        self._formatter = formatter

    def formatRate(self, loss):
        return self._formatter(loss)


def _gauss_window(device, size: int = 11, sigma: float = 1.5) -> torch.Tensor:
    coords = torch.arange(size, device=device).float()
    coords -= size // 2
    g = torch.exp(-(coords ** 2) / (2 * sigma ** 2))
    g /= g.sum()
    return g.view(1, 1, 1, size)


def _torch_ms_ssim(X: torch.Tensor, Y: torch.Tensor, data_range: float) -> torch.Tensor:
    """metrics.py:69-104, 142-193 (win 11 / sigma 1.5, K = (0.01, 0.03), sizeAverage) in torch: the fallback off the HIP path."""
    if X.dim() != 4 or X.shape != Y.shape:
        raise ValueError(f"expected two [N, C, H, W] batches of one shape, got {tuple(X.shape)} and {tuple(Y.shape)}")
    if min(X.shape[-2:]) <= 160:
        raise ValueError(f"MS-SSIM needs image sides larger than 160 pixels, got {X.shape[-2]}x{X.shape[-1]}")
    C = X.shape[1]
    win = _gauss_window(X.device).to(X.dtype).repeat(C, 1, 1, 1)

    def blur(x):
        out = F.conv2d(x, win.transpose(2, 3), groups=C)
        return F.conv2d(out, win, groups=C)

    c1, c2 = (0.01 * data_range) ** 2, (0.03 * data_range) ** 2
    weights = torch.tensor(_WEIGHTS, dtype=X.dtype, device=X.device)
    mcs = []
    for i in range(5):
        mu1, mu2 = blur(X), blur(Y)
        mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
        s1 = blur(X * X) - mu1_sq
        s2 = blur(Y * Y) - mu2_sq
        s12 = blur(X * Y) - mu1_mu2
        cs_map = (2 * s12 + c2) / (s1 + s2 + c2)
        ssim_map = ((2 * mu1_mu2 + c1) / (mu1_sq + mu2_sq + c1)) * cs_map
        if i < 4:
            mcs.append(torch.relu(cs_map.flatten(2).mean(-1)))
            padding = [s % 2 for s in X.shape[2:]]
            X = F.avg_pool2d(X, kernel_size=2, padding=padding)
            Y = F.avg_pool2d(Y, kernel_size=2, padding=padding)
    ssim = torch.relu(ssim_map.flatten(2).mean(-1))
    stack = torch.stack(mcs + [ssim], dim=1)
    return torch.prod(stack ** weights.view(1, -1, 1), dim=1).mean()


def ms_ssim_loss(restored: torch.Tensor, image: torch.Tensor, offset: float = 1.0, data_range: float = 2.0) -> torch.Tensor:
    """1 - MS-SSIM(restored + offset, image + offset) over the batch, a 0-dim tensor (differentiable in both inputs)."""
    if restored.is_cuda and restored.dtype == torch.float32 and image.dtype == torch.float32:
        return MsSsimFn.apply(restored, image, offset, data_range)
    return 1.0 - _torch_ms_ssim(restored + offset, image + offset, data_range)


class MsSSIM(nn.Module):
    """mcquic/loss/__init__.py:47-55: `1 - ms_ssim(restored + 1, image + 1)` with data range 2.0 and the batch mean; the
    formatter is Decibel(1.0), -10 log10(loss)."""

    def __init__(self):
        super().__init__()
        self._formatter = Decibel(1.0)

    def formatDistortion(self, loss):
        return self._formatter(loss)

    def forward(self, restored, image, *_):
        return ms_ssim_loss(restored, image)


class PSNR(nn.Module):
    """mcquic/loss/__init__.py:57-63: mean squared error (this library's reduction on the HIP path); Decibel(2.0)."""

    def __init__(self):
        super().__init__()
        self._formatter = Decibel(2.0)

    def formatDistortion(self, loss):
        return self._formatter(loss)

    def forward(self, restored, image, *_):
        return mse_loss(restored, image)


class _WeightedSumFn(torch.autograd.Function):
    """alpha * a + beta * b of two 0-dim losses with this library's element-wise kernel (no ATen launch in a captured step)."""

    @staticmethod
    def forward(ctx, a, b, alpha, beta):
        ctx.alpha, ctx.beta = float(alpha), float(beta)
        return ops.axpby(a.contiguous(), b.contiguous(), ctx.alpha, ctx.beta)

    @staticmethod
    def backward(ctx, dout):
        dout = dout.contiguous().float()
        da = ops.axpby(dout, dout, ctx.alpha, 0.0) if ctx.needs_input_grad[0] else None
        db = ops.axpby(dout, dout, ctx.beta, 0.0) if ctx.needs_input_grad[1] else None
        return da, db, None, None


def _weighted_sum(a: torch.Tensor, b: torch.Tensor, alpha: float, beta: float) -> torch.Tensor:
    if a.is_cuda and a.dtype == torch.float32 and b.dtype == torch.float32 and a.shape == b.shape:
        return _WeightedSumFn.apply(a, b, alpha, beta)
    return alpha * a + beta * b


def _torch_cosine(codebook: torch.Tensor) -> torch.Tensor:
    """mcquic/loss/__init__.py:32-41 as written, for one level's [m, k, d]: the fallback off the HIP path."""
    losses = []
    for c in codebook:
        pairwise = c @ c.T
        norm = (c ** 2).sum(-1)
        cos = pairwise / (norm[:, None] * norm).sqrt()
        losses.append(cos.triu(1).clamp(0.0, 2).sum())
    return sum(losses)


_ZEROS = {}


class BasicRate(Rate):
    """mcquic/loss/__init__.py:27-44: gamma times the sum, over every level's codebook [m, k, d] and every group, of the pairwise
    cosines of its codewords above the diagonal, clamped to [0, 2] -- the term that pushes the codewords of a codebook apart.
    `codebooks` is the list over levels that `model.Codebooks` returns; `logits` is not read (the reference's signature).

    On a HIP device in float32 with d <= 256 a level is one `CodebookCosineFn` node (csrc/codebook_cos.hip: the [k, k] plane is
    never written, 256 MiB per group at k = 8192) and the levels are summed and scaled with this library's element-wise kernel;
    elsewhere it is the reference's torch formula.
    The one deliberate shortcut: with gamma == 0 the result is a 0-dim zero that launches nothing and gives the codebooks no
    gradient, where the reference computes 0 * loss -- NaN for a codebook with a zero codeword."""

    def __init__(self, gamma: float = 0.0):
        super().__init__(nn.Identity())
        self._gamma = gamma

    @staticmethod
    def _cosineLoss(codebook: torch.Tensor) -> torch.Tensor:
        if codebook.is_cuda and codebook.dtype == torch.float32 and codebook.dim() == 3 and 1 <= codebook.shape[-1] <= 256 \
                and codebook.numel():
            return CodebookCosineFn.apply(codebook)
        return _torch_cosine(codebook)

    def forward(self, logits, codebooks, *_):
        codebooks = list(codebooks)
        if self._gamma == 0 or not codebooks:
            key = (codebooks[0].device, codebooks[0].dtype) if codebooks else (torch.device("cpu"), torch.float32)
            zero = _ZEROS.get(key)
            if zero is None:                                            # (made once per device: a fill is a launch)
                zero = _ZEROS[key] = torch.zeros((), dtype=key[1], device=key[0])
            return zero
        total = None
        for codebook in codebooks:
            term = self._cosineLoss(codebook)
            total = term if total is None else _weighted_sum(total, term, 1.0, 1.0)
        if total.is_cuda and total.dtype == torch.float32:
            return _weighted_sum(total, total.detach(), self._gamma, 0.0)       # (gamma * total: one node input, one launch back)
        return self._gamma * total


class _MsSsimMseFn(torch.autograd.Function):
    """w_d * (1 - MS-SSIM(a + 1, b + 1)) + w_m * mean((a - b)^2) as ONE node: both terms read a, and two nodes would leave the
    sum of their gradients on a to the autograd engine -- an ATen add inside a captured step.  Library kernels only."""

    @staticmethod
    def forward(ctx, a, b, wd, wm):
        a, b = a.contiguous(), b.contiguous()
        ms, values, saved = ops.ms_ssim_loss(a, b)
        ctx.save_for_backward(a, b, values, saved)
        ctx.wd, ctx.wm = float(wd), float(wm)
        return ops.axpby(ms, ops.mse(a, b), ctx.wd, ctx.wm)

    @staticmethod
    def backward(ctx, dout):
        a, b, values, saved = ctx.saved_tensors
        want_a, want_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (want_a or want_b):
            return None, None, None, None
        dout = dout.contiguous().float()
        dms, dmse = ops.axpby(dout, dout, ctx.wd, 0.0), ops.axpby(dout, dout, ctx.wm, 0.0)
        da1, db1 = ops.ms_ssim_loss_bwd(a, b, values, saved, dms, want_db=want_b)
        da2, db2 = ops.mse_bwd(a, b, dmse, want_db=want_b)
        return (ops.add(da1, da2) if want_a else None), (ops.add(db1, db2) if want_b else None), None, None


def step_loss(distortion: nn.Module | None = None, distortion_weight: float = 0.5, mse_weight: float = 0.5,
              rate: nn.Module | None = None, model: nn.Module | None = None):
    """`loss_fn(out, x)` for `parallel.GraphedTrainStep` and eager loops: the reference trainer's objective
    `0.5 * recon + 0.5 * mse(xHat, x)` (mcquic/train/trainer.py:273-276, mcquic/modules/compound.py:35-42) with
    `recon = distortion(xHat, x)`, MsSSIM() by default.  `out` is the Compressor's training output (xHat first).
    The reference's third term, 2 * LPIPS, is NOT included: it needs ImageNet VGG16 weights this package does not ship.
    `rate` (a `Rate`, e.g. BasicRate(gamma); needs `model`, whose `.Codebooks` it reads at every call): the objective plus
    `rate(out[3], model.Codebooks)`.  Each codebook then receives two gradients, the quantizer's and the regulariser's, which the
    autograd engine sums; under `GraphedTrainStep` both must lie in one graph, so such a `loss_fn` carries
    `single_segment = True` and is taken with `segments=1` only.  Without `rate` nothing changes."""
    distortion = MsSSIM() if distortion is None else distortion
    fused = type(distortion) is MsSSIM
    if rate is not None and model is None:
        raise ValueError("step_loss: `rate` reads the codebooks of the model being trained: pass `model=` as well")

    def objective(out, x):
        xHat = out[0] if isinstance(out, (tuple, list)) else out
        if fused and xHat.is_cuda and xHat.dtype == torch.float32 and x.dtype == torch.float32 and xHat.shape == x.shape:
            return _MsSsimMseFn.apply(xHat, x, distortion_weight, mse_weight)
        return _weighted_sum(distortion(xHat, x), mse_loss(xHat, x), distortion_weight, mse_weight)

    if rate is None:
        return objective

    def loss_fn(out, x):
        logits = out[3] if isinstance(out, (tuple, list)) and len(out) > 3 else None
        return _weighted_sum(objective(out, x), rate(logits, model.Codebooks), 1.0, 1.0)

    loss_fn.single_segment = True
    return loss_fn
