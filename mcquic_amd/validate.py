"""Validation-side helpers around the Compressor (reference: mcquic/validate/validator.py:40-97,
mcquic/validate/metrics.py:264-274, mcquic/validate/handlers.py).  Caller-level code: statistics only.

`speed` is the reference's throughput protocol verbatim (random 10x3x768x512 batch, one warm-up, 50 `compress` then 50
`decompress` calls timed with events on the current stream, Mpps = 50*10*768*512/1000/ms) -- byte streams included,
exactly what the README's 25.45 / 22.03 Mpps (RTX 3090) were measured with.  `validate` restores a batch and returns
per-image PSNR and MS-SSIM (on the de-transformed uint8 images, HIP kernels of csrc/metrics.hip) and bits per pixel;
with torch.distributed initialised the rows of all ranks are gathered (parallel.gather_image_stats), images being
sharded by the caller (parallel.shard_range).  `ideal_bpp` is the handlers' entropy estimate over code histograms.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import torch

from . import ops, parallel


@torch.inference_mode()
def speed(model, iters: int = 50, batch: int = 10, height: int = 768, width: int = 512) -> Tuple[float, float]:
    device = next(model.parameters()).device
    tensor = torch.rand(batch, 3, height, width).to(device)
    startEvent = torch.cuda.Event(enable_timing=True)
    endEvent = torch.cuda.Event(enable_timing=True)
    codes, binaries, headers = model.compress(tensor)          # warm up
    model.decompress(binaries, headers)
    startEvent.record()
    for _ in range(iters):
        codes, binaries, headers = model.compress(tensor)
    endEvent.record()
    torch.cuda.synchronize()
    encoderMs = startEvent.elapsed_time(endEvent)
    startEvent.record()
    for _ in range(iters):
        model.decompress(binaries, headers)
    endEvent.record()
    torch.cuda.synchronize()
    decoderMs = startEvent.elapsed_time(endEvent)
    mpx = iters * batch * height * width / 1000
    return mpx / encoderMs, mpx / decoderMs


def psnr(x_u8: torch.Tensor, y_u8: torch.Tensor) -> torch.Tensor:
    """Per-image PSNR of uint8 batches, float64, upper bound 255 (metrics.py:264-274).  The squared-error sum is taken
    exactly in integers on the device, so the float64 mean squared error equals the reference's bit for bit."""
    mse = ops.sqdiff_sum(x_u8, y_u8).double() / float(x_u8[0].numel())
    return 10.0 * (255.0 ** 2 / (mse + 1e-4)).log10()


def ms_ssim_db(x_u8: torch.Tensor, y_u8: torch.Tensor) -> torch.Tensor:
    """Per-image MS-SSIM in dB as the reference's handler reports it (handlers.py:14-27: Decibel(1.0) of the MsSSIM
    module's 1 - ms_ssim, i.e. -10 log10(1 - value)); float32 like the reference."""
    return -10.0 * (1.0 - ops.ms_ssim(x_u8, y_u8)).log10()


def ideal_bpp(histograms: Sequence[torch.Tensor], total_pixels: int) -> float:
    """Entropy-coded size estimate of a validation run (handlers.py:110-187 `IdealBPP.Result`): for every level and group
    the empirical entropy of the accumulated code histogram [m, k] (e.g. parallel.code_histograms summed over the run)
    times the number of codes of that group, summed, per image pixel."""
    total = 0.0
    for usage in histograms:
        usage = usage.float()
        count = usage.sum(-1)
        prob = usage / count[:, None]
        ent = prob.log2()
        ent[ent == float("-inf")] = 0
        total += float((-(prob * ent).sum(-1) * count).sum())
    return total / float(total_pixels)


@torch.inference_mode()
def validate(model, images: torch.Tensor, group=None, msssim: bool = True, gather: bool = True, bits: str = "coded") -> torch.Tensor:
    """images: this rank's shard, fp32 [n, 3, h, w] in [-1, 1].  Returns float64 rows [psnr_db, ms_ssim_db, bpp] for ALL
    images (rank order) -- the [psnr, ms_ssim, bits] statistics of the reference's validator (validator.py:40-58).
    `msssim=False` fills the MS-SSIM column with NaN (the metric is undefined for sides <= 160 pixels); `gather=False`
    returns this rank's rows only.  `bits`: "coded" takes bpp from the byte streams of `compress` (codes to the host, the rANS coder,
    and back through `decompress`); "estimated" runs `encode` / `decode` and takes bpp from `codeBits`, what the coder's tables charge
    for the codes (lower than the coded figure by the streams' flush and renormalisation words only) -- nothing leaves the device
    but the result rows; "exact" runs `encode` / `decode` too and takes bpp from the sizes of the streams the device coder makes
    (`EntropyCoder.compressDevice(...).sizes()`): the figure of "coded" exactly, with nothing coded on the host."""
    if bits not in ("coded", "estimated", "exact"):
        raise ValueError(f"validate: bits must be 'coded', 'estimated' or 'exact', got {bits!r}")
    if images.shape[0] == 0:                                  # an empty shard still takes part in the gather
        rows = torch.empty((0, 3), dtype=torch.float64, device=images.device)
        return parallel.gather_image_stats(rows, group) if gather else rows
    if bits != "coded":
        return _validate_on_device(model, images, group, msssim, gather, bits)
    codes, binaries, headers = model.compress(images)
    restored = model.decompress(binaries, headers)
    a, b = ops.detransform(images.contiguous()), ops.detransform(restored.contiguous())
    p = psnr(a, b)
    s = ms_ssim_db(a, b).double() if msssim else torch.full_like(p, float("nan"))
    pixels = images.shape[-2] * images.shape[-1]
    bpp = torch.tensor([sum(len(s_) for s_ in bi) * 8 / pixels for bi in binaries], dtype=torch.float64, device=images.device)
    rows = torch.stack([p, s, bpp], 1)
    return parallel.gather_image_stats(rows, group) if gather else rows


@torch.inference_mode()
def rate_sweep(model, x: torch.Tensor, lambdas: Sequence[float], bits: str = "estimated", msssim: bool = True, aq=None) -> torch.Tensor:
    """One model over a range of rates: for every lambda of `lambdas` the rows of `validate(model, x, bits=bits)` with the images
    encoded by `model.encode(x, rd_lambda=lambda)`, averaged over the batch.  Returns float64 [len(lambdas), 4]: the existing columns
    [psnr_db, ms_ssim_db, bpp] plus `rd_lambda`.  `bits`: "estimated" or "exact", as for `validate` (the streams of "coded" are those
    of "exact").  `aq`: adaptive quantisation as for `Compressor.encode`, the same for every lambda.  This rank's images only."""
    if bits not in ("estimated", "exact"):
        raise ValueError(f"rate_sweep: bits must be 'estimated' or 'exact', got {bits!r}")
    lams = [model._quantizer.rateLambdas(lam) for lam in lambdas]             # all checked before any device work
    aq = model._aqArgs(aq)
    rows = []
    for lam, per_level in zip(lambdas, lams):
        r = _validate_on_device(model, x, None, msssim, False, bits, rd_lambda=per_level, aq=aq).mean(0)
        # (a per-level list shows as its first entry)
        rows.append(torch.cat([r, r.new_tensor([float(lam) if not isinstance(lam, (list, tuple)) else per_level[0]])]))
    return torch.stack(rows) if rows else torch.empty((0, 4), dtype=torch.float64, device=x.device)


def _validate_on_device(model, images: torch.Tensor, group, msssim: bool, gather: bool, bits: str, rd_lambda=None, aq=None) -> torch.Tensor:
    """`validate` with the size of the codes taken on the device: from the coder's tables ("estimated") or from the device coder's
    streams ("exact": bytes * 8 / pixels in float64, the one division of the coded path).  The restored images are those of the coded path
    (the coder is lossless: `decompress` decodes to these codes), cropped from the padded reconstruction as `decompress` crops."""
    if aq is not None:
        codes = model.encode(images, rd_lambda=rd_lambda, aq=aq)
    else:
        codes = model.encode(images) if rd_lambda is None else model.encode(images, rd_lambda=rd_lambda)
    restored = model.decode(codes)
    h, w = images.shape[-2], images.shape[-1]
    top, left = (restored.shape[-2] - h) // 2, (restored.shape[-1] - w) // 2
    restored = restored[..., top:top + h, left:left + w]
    a, b = ops.detransform(images.contiguous()), ops.detransform(restored.contiguous())
    p = psnr(a, b)
    s = ms_ssim_db(a, b).double() if msssim else torch.full_like(p, float("nan"))
    if bits == "exact":
        streams = model._quantizer._entropyCoder.compressDevice(codes)
        bpp = (streams.sizes().sum(-1) * 8).double() / float(h * w)
        streams.check()                                       # an out-of-range code raises, as `compress` does on the coded path
    else:
        bpp = model.codeBits(codes).sum(-1) / float(h * w)
    rows = torch.stack([p, s, bpp], 1)
    return parallel.gather_image_stats(rows, group) if gather else rows
