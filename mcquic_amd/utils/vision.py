"""The reference's batch transforms (mcquic/utils/vision.py:85-129, 150-197; torchvision's RandomResizedCrop) on the device.

Every module here is a setting of ONE pipeline -- crop box resample, gamma, colour gains, clamp, flips, normalise -- that runs
as two HIP launches (csrc/augment.hip): `ops.augment_draw` writes the per-image decisions into a device table from the
module's own {seed, offset} generator state, `ops.augment` applies the table.  A stage a module does not name is the identity
in its table.  The jitter and the flips are the operations the reference intends: its in-place forms act on copies
(`x[mask].mul_(...)`, `tensor[mask].copy_(...)`) and change nothing.

    forward(x, params=None)    x: [N, 3, Hs, Ws] uint8 (read as v / 255) or float32, contiguous, on the HIP device.
                               params: a table [N, 16] to apply instead of drawing one (ops.AUG_* columns).
    last_params                the device table of the last call (no synchronisation).
    state_dict()               holds `rng` = {seed, offset}: restoring it resumes the stream of decisions.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch
from torch import nn

from .. import ops

__all__ = ["Augment", "RandomPlanckianJitter", "RandomGamma", "RandomHorizontalFlip", "RandomVerticalFlip", "RandomResizedCrop"]


def _range(v, name: str):
    lo, hi = (float(t) for t in v)
    if not 0.0 < lo <= hi:
        raise ValueError(f"`{name}` must be a positive, ordered range, got {tuple(v)}")
    return lo, hi


class Augment(nn.Module):
    """The pipeline with every stage optional.  `size` None: the source's own size (no resampling); `crop` = (scale, ratio) or
    None; `gamma`: RandomGamma; `coeffs` [T, 2] with `p_gain`: RandomPlanckianJitter; `p_hflip` / `p_vflip`; `output`: what
    follows the gains (ops.AUG_OUT_NORMALIZED: clamp and Normalize(0.5, 0.5); _CLAMPED: the clamp; _RAW: neither)."""

    def __init__(self, size: Optional[Sequence[int]] = None, crop=None, gamma: bool = False, coeffs: Optional[torch.Tensor] = None,
                 p_gain: float = 0.0, p_hflip: float = 0.0, p_vflip: float = 0.0, output: int = ops.AUG_OUT_NORMALIZED,
                 seed: Optional[int] = None):
        super().__init__()
        self.size = None if size is None else (int(size[0]), int(size[1]))
        self.crop = None if crop is None else (_range(crop[0], "scale"), _range(crop[1], "ratio"))
        self.gamma = bool(gamma)
        if coeffs is not None:
            coeffs = torch.as_tensor(coeffs, dtype=torch.float32).detach().clone()
            if coeffs.dim() != 2 or coeffs.shape[1] != 2 or coeffs.shape[0] < 1:
                raise ValueError(f"`coeffs` must be a [T, 2] table of (channel 0, channel 2) gains, got {tuple(coeffs.shape)}")
        self.register_buffer("coeffs", coeffs)
        for name, p in (("p_gain", p_gain), ("p_hflip", p_hflip), ("p_vflip", p_vflip)):
            if not 0.0 <= float(p) <= 1.0:
                raise ValueError(f"`{name}` is a probability, got {p}")
        self.p_gain, self.p_hflip, self.p_vflip = float(p_gain), float(p_hflip), float(p_vflip)
        self.output = int(output)
        seed = torch.initial_seed() if seed is None else int(seed)
        self.register_buffer("rng", torch.tensor([seed & 0x7fffffffffffffff, 0], dtype=torch.int64))
        self.last_params = None

    def settings(self) -> dict:
        """The constructor arguments that describe the stages (what data.transforms.TrainingInput merges two halves from)."""
        return dict(size=self.size, crop=self.crop, gamma=self.gamma, coeffs=self.coeffs, p_gain=self.p_gain, p_hflip=self.p_hflip,
                    p_vflip=self.p_vflip, output=self.output)

    def out_size(self, x: torch.Tensor):
        return self.size if self.size is not None else (int(x.shape[-2]), int(x.shape[-1]))

    def draw(self, x: torch.Tensor) -> torch.Tensor:
        """One draw launch: the table for a batch like `x` (advances the generator)."""
        if not x.is_cuda:
            raise RuntimeError(f"mcquic_amd: the input transform runs on a HIP device (got {x.device}); the HIP kernels have no CPU fallback")
        for name in ("rng", "coeffs"):                        # (buffers follow .to(device); a module left on the CPU follows its input)
            b = getattr(self, name)
            if b is not None and b.device != x.device:
                setattr(self, name, b.to(x.device))
        return ops.augment_draw(self.rng, x.shape[0], x.shape[-2:], crop=self.crop, gamma=self.gamma, coeffs=self.coeffs,
                                p_gain=self.p_gain if self.coeffs is not None else 0.0, p_hflip=self.p_hflip, p_vflip=self.p_vflip,
                                output=self.output)

    def forward(self, x: torch.Tensor, params: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        if not torch.is_tensor(x) or not x.is_cuda:
            raise RuntimeError(f"mcquic_amd: the input transform runs on a HIP device (got {getattr(x, 'device', type(x))}); "
                               "the HIP kernels have no CPU fallback")
        if x.dim() != 4:
            raise ValueError(f"expected a [N, 3, Hs, Ws] batch, got {tuple(x.shape)}")
        if params is None:
            params = self.draw(x)
        self.last_params = params
        return ops.augment(x, self.out_size(x), params, out=out)

    def extra_repr(self) -> str:
        return ", ".join(f"{k}={v}" for k, v in self.settings().items() if k != "coeffs")


class RandomPlanckianJitter(Augment):
    """With probability `p` per image one row of `coeffs` [T, 2]: channel 0 times coeffs[t, 0], channel 2 times coeffs[t, 1];
    then every image is clamped to [0, 1] (vision.py:85-104).  The table is the caller's: none is built in."""

    def __init__(self, coeffs: torch.Tensor, p: float = 0.5, seed: Optional[int] = None):
        if coeffs is None:
            raise ValueError("RandomPlanckianJitter needs its [T, 2] table of gains: there is no built-in default")
        super().__init__(coeffs=coeffs, p_gain=p, output=ops.AUG_OUT_CLAMPED, seed=seed)


class RandomGamma(Augment):
    """Per image one of four, uniformly: the two sRGB curves, x^g with g ~ U(0.05, 2.0), identity (vision.py:108-129)."""

    def __init__(self, seed: Optional[int] = None):
        super().__init__(gamma=True, output=ops.AUG_OUT_RAW, seed=seed)


class RandomHorizontalFlip(Augment):
    def __init__(self, p: float = 0.5, seed: Optional[int] = None):
        super().__init__(p_hflip=p, output=ops.AUG_OUT_RAW, seed=seed)


class RandomVerticalFlip(Augment):
    def __init__(self, p: float = 0.5, seed: Optional[int] = None):
        super().__init__(p_vflip=p, output=ops.AUG_OUT_RAW, seed=seed)


class RandomResizedCrop(Augment):
    """torchvision's rule per image (ten attempts, then the central crop), the box resampled to `size` with the antialiased
    bilinear filter torchvision applies to tensors."""

    def __init__(self, size, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), seed: Optional[int] = None):
        super().__init__(size=size, crop=(scale, ratio), output=ops.AUG_OUT_RAW, seed=seed)
