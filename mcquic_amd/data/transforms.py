"""The reference's input transforms (mcquic/data/transforms.py) over the two launches of csrc/augment.hip.

    getTrainingPreprocess(size)                 the loader's half: RandomResizedCrop(size, (0.75, 1), (0.95, 1.05)) + RandomGamma
    getTrainingTransform(gen, planckian)        the trainer's half: colour gain, flips, Normalize(0.5, 0.5)
    TrainingInput(size, scale, ratio, ...)      both halves fused: one draw launch, one apply launch per batch
    getEvalTransform()                          AlignedCrop(256) + Normalize(0.5, 0.5), one launch

Each half is a `utils.vision.Augment`; `TrainingInput.from_halves(pre, post)` fuses two of them.  The fused pass gives what the
halves give one after the other under the same decisions, bit for bit: the second half resamples nothing (box = its whole input
at the same size: weights 1 and 0) and the value between them is the same float32 either way."""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from .. import ops
from ..utils.vision import Augment

__all__ = ["AlignedCrop", "EvalTransform", "TrainingInput", "getEvalTransform", "getTrainingPreprocess", "getTrainingTransform"]


def getTrainingPreprocess(size=(512, 512), seed: Optional[int] = None) -> Augment:
    """transforms.py:14-21 -- per sample in the reference's loader; per image of the batch here.  Values leave as they are
    (no clamp, no normalisation): the second half brings both."""
    return Augment(size=size, crop=((0.75, 1.0), (0.95, 1.05)), gamma=True, output=ops.AUG_OUT_RAW, seed=seed)


def getTrainingTransform(gen: bool = False, planckian: Optional[torch.Tensor] = None, seed: Optional[int] = None) -> Augment:
    """transforms.py:37-43.  `planckian`: the [T, 2] gain table of RandomPlanckianJitter(p=1.0), or None to leave the gain out --
    what the reference computes in effect (its jitter multiplies a copy), as its flips do nothing either: with `gen=True` and
    no table this is clamp(x, 0, 1) then (x - 0.5) / 0.5 exactly."""
    p_flip = 0.0 if gen else 0.5
    return Augment(coeffs=planckian, p_gain=1.0 if planckian is not None else 0.0, p_hflip=p_flip, p_vflip=p_flip,
                   output=ops.AUG_OUT_NORMALIZED, seed=seed)


class TrainingInput(Augment):
    """Preprocess + transform in two launches: a raw batch [N, 3, Hs, Ws] (uint8 or float32 in [0, 1]) in, the model's input
    [N, 3, H, W] float32 in [-1, 1] out.  `parallel.GraphedTrainStep(..., transform=TrainingInput(...))` captures both launches at
    the head of the step; `state_dict()` / `load_state_dict()` carry the generator's {seed, offset}."""

    def __init__(self, size=(512, 512), scale=(0.75, 1.0), ratio=(0.95, 1.05), gamma: bool = True, planckian: Optional[torch.Tensor] = None,
                 p_planckian: float = 1.0, p_hflip: float = 0.5, p_vflip: float = 0.5, gen: bool = False, seed: Optional[int] = None):
        super().__init__(size=size, crop=(scale, ratio), gamma=gamma, coeffs=planckian, p_gain=p_planckian if planckian is not None else 0.0,
                         p_hflip=0.0 if gen else p_hflip, p_vflip=0.0 if gen else p_vflip, output=ops.AUG_OUT_NORMALIZED, seed=seed)

    @classmethod
    def from_halves(cls, preprocess: Augment, transform: Augment, seed: Optional[int] = None) -> "TrainingInput":
        """The fused form of `transform(preprocess(x))`: the first half's crop, size and gamma, the second half's gain, flips and
        output range."""
        a, b = preprocess.settings(), transform.settings()
        if b["crop"] is not None or b["size"] is not None or b["gamma"]:
            raise ValueError("TrainingInput.from_halves: the second half must not crop, resize or draw a gamma (those come first in the pipeline)")
        if a["coeffs"] is not None or a["p_hflip"] or a["p_vflip"] or a["output"] != ops.AUG_OUT_RAW:
            raise ValueError("TrainingInput.from_halves: the first half must leave gain, flips, clamp and normalisation to the second")
        self = cls.__new__(cls)
        Augment.__init__(self, size=a["size"], crop=a["crop"], gamma=a["gamma"], coeffs=b["coeffs"], p_gain=b["p_gain"],
                         p_hflip=b["p_hflip"], p_vflip=b["p_vflip"], output=b["output"], seed=seed)
        return self


class AlignedCrop(nn.Module):
    """The centre crop to multiples of `base` per side (transforms.py:57-78), as a view."""

    def __init__(self, base: int = 128):
        super().__init__()
        self._base = int(base)

    def box(self, h: int, w: int):
        """(top, left, height, width) of the crop inside an h x w image."""
        ch, cw = h // self._base * self._base, w // self._base * self._base
        if ch == 0 or cw == 0:
            raise ValueError(f"AlignedCrop({self._base}): a {h}x{w} image has no {self._base}-aligned crop")
        return (h - ch) // 2, (w - cw) // 2, ch, cw

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        top, left, h, w = self.box(x.shape[-2], x.shape[-1])
        return x[..., top: top + h, left: left + w]


class EvalTransform(nn.Module):
    """ConvertImageDtype(float32), AlignedCrop(base), Normalize(0.5, 0.5) (transforms.py:49-54) as ONE launch: the crop is the
    box of a fixed table, resampled at its own size (weights 1 and 0: the pixels themselves)."""

    def __init__(self, base: int = 256):
        super().__init__()
        self.crop = AlignedCrop(base)
        self._tables = {}

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if not torch.is_tensor(x) or not x.is_cuda:
            raise RuntimeError(f"mcquic_amd: the input transform runs on a HIP device (got {getattr(x, 'device', type(x))}); "
                               "the HIP kernels have no CPU fallback")
        if x.dim() == 3:
            x = x[None]
        n, _, hs, ws = x.shape
        top, left, h, w = self.crop.box(hs, ws)
        key = (n, hs, ws, x.device)
        params = self._tables.get(key)
        if params is None:
            params = ops.augment_identity_params(n, (hs, ws))
            params[:, ops.AUG_TOP], params[:, ops.AUG_LEFT], params[:, ops.AUG_H], params[:, ops.AUG_W] = top, left, h, w
            params = self._tables[key] = params.to(x.device)
        return ops.augment(x, (h, w), params)


def getEvalTransform() -> EvalTransform:
    return EvalTransform(256)
