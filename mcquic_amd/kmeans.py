"""Data-dependent codebooks: k-means (Lloyd iterations) on the device over what the quantizer's levels actually receive.

    from mcquic_amd import kmeans
    report = kmeans.fit_codebooks(model, batches, iters=8, seed=0)      # before the first training step

`UMGMQuantizer` draws its codebooks from N(0, 2 / (5 d)), unrelated to what the encoder emits, and training spends its first
steps with most codewords dead (`CodeUsage`; the random drop, `reAssignCodebook` and the frequency EMA exist to repair that).
The reference wanted the same fix -- its `CountingCodes` hook collects codes "to use k-means to find new centers" and raises
NotImplementedError (mcquic/train/hooks.py:123-153).

One iteration = the existing MFMA assignment (`ops.vq_assign`) + csrc/vq_kmeans.hip: a per-codeword segmented sum without
atomics, the centroid update with the inertia, and the reseeding of empty clusters from data vectors.  Everything stays on the
device; nothing is read back inside an iteration, and the same seed gives the same bits.

Multi-rank use is not built in.  The pattern is the `CodebookReassign` hook's: rank 0 fits, then every rank calls
`model.syncCodebook()`.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence

import torch

from . import ops
from .modules.quantizer import UMGMQuantizer, _multiCodebookQuantization


class LevelReport(NamedTuple):
    """Per level: `inertia` float64 [iters, m] (within-cluster sum of squares of every iteration's assignment, against the
    codewords it was made with) and `empty` int64 [iters, m] (codewords no vector was assigned to), device tensors."""
    inertia: torch.Tensor
    empty: torch.Tensor


def _assign_accumulate(quantization: _multiCodebookQuantization, x: torch.Tensor, acc: ops.KMeansAcc) -> None:
    codes = ops.vq_assign(x, quantization._cache[0].get(quantization._codebook))
    ops.vq_kmeans_accumulate(x, codes, acc)


@torch.no_grad()
def lloyd_step(quantization: _multiCodebookQuantization, x: torch.Tensor, acc: Optional[ops.KMeansAcc] = None):
    """One Lloyd iteration of a level's codebook on ONE batch of its inputs `x` [n, m*d, h, w]: assign (the level's packed-operand
    cache and `ops.vq_assign`), accumulate, update; the new codebook goes through `_store`, so the packed operand is rebuilt.
    `acc`: accumulators to reuse (zeroed here).  Returns (inertia float64 [m], empty int64 [m]) on the device."""
    cb = quantization._codebook
    m, k, d = cb.shape
    acc = ops.KMeansAcc(m, k, d, x.device) if acc is None else acc.zero_()
    _assign_accumulate(quantization, x, acc)
    fresh = cb.detach().clone()
    inertia, empty = ops.vq_kmeans_update(fresh, acc)
    quantization._store(fresh)
    return inertia, empty


@torch.no_grad()
def fit_codebooks(model, batches: Sequence[torch.Tensor], iters: int = 8, seed: int = 0, levels: Optional[Sequence[int]] = None,
                  init: str = "data", reseed_empty: bool = True) -> List[Optional[LevelReport]]:
    """Fit the codebooks of `model` (a `Compressor`) to the latents of `batches` ([n, 3, H, W] float32 device tensors in [-1, 1]),
    on the inference path, level by level in cascade order -- level l's inputs depend on the codebooks before it.

    Per level: `init="data"` seeds every codeword from a latent vector of the first batch (`init="current"` starts from the codebook
    as it is); then `iters` times: over all batches assign + accumulate, one update, and (`reseed_empty`) the codewords that
    received nothing are reseeded from latent vectors of the last batch.  `levels`: the levels to fit (default: all); the others
    keep their codebooks.  `seed` starts a generator of this call's own ({seed, 0}, advanced on the device per seeding launch):
    the same seed gives the same codebooks bit for bit, and the training generator (`ops.seed_rng`) is left alone.

    The encoder runs ONCE per batch: what is cached per batch is the small tensor entering the current level (1/16 of the image
    side and below) and that level's quantizer input, not the image features; a level's heads run twice per batch (once for the
    quantizer input, once more under the fitted codebook for the residual the next level takes).

    Returns one entry per level: a `LevelReport` for a fitted level, None for a skipped one.  No host read-back happens inside."""
    quantizer = getattr(model, "_quantizer", None)
    if not isinstance(quantizer, UMGMQuantizer):
        raise NotImplementedError(f"fit_codebooks fits the per-level codebooks of a UMGMQuantizer (Compressor); "
                                  f"{type(quantizer).__name__} shares its codebook between levels and is out of scope")
    if init not in ("data", "current"):
        raise ValueError(f"init must be 'data' or 'current', got {init!r}")
    if iters < 1 or len(batches) < 1:
        raise ValueError("fit_codebooks needs at least one iteration and one batch")
    nlevels = len(quantizer._encoders)
    chosen = sorted(set(range(nlevels) if levels is None else (int(l) for l in levels)))
    if chosen and not 0 <= chosen[0] <= chosen[-1] < nlevels:
        raise ValueError(f"levels must lie in [0, {nlevels}), got {list(levels)}")
    for x in batches:
        model._check(x)
        if not x.is_cuda:
            raise RuntimeError(f"mcquic_amd: `batches` must live on a HIP device (got {x.device}); the HIP kernels have no CPU fallback")
    dev = batches[0].device
    rng = torch.tensor([int(seed) & 0x7fffffffffffffff, 0], dtype=torch.int64).to(dev)
    report: List[Optional[LevelReport]] = [None] * nlevels
    if not chosen:
        return report
    state = [model._encode_latent(x) for x in batches]                      # what enters the current level, per batch
    for lv in range(chosen[-1] + 1):
        encoder = quantizer._encoders[lv]
        if lv in chosen:
            quantization = encoder._quantizer
            m, k, d = quantization._codebook.shape
            inputs = [encoder._encode(y)[2] for y in state]
            if init == "data":
                fresh = quantization._codebook.detach().clone()
                ops.vq_kmeans_seed(inputs[0], fresh, rng)
                rng[1:].add_(1)
                quantization._store(fresh)
            acc = ops.KMeansAcc(m, k, d, dev)
            inertia = torch.empty((iters, m), dtype=torch.float64, device=dev)
            empty = torch.empty((iters, m), dtype=torch.int64, device=dev)
            for it in range(iters):
                if it:
                    acc.zero_()
                for x in inputs:
                    _assign_accumulate(quantization, x, acc)
                fresh = quantization._codebook.detach().clone()
                inertia[it], empty[it] = ops.vq_kmeans_update(fresh, acc)
                if reseed_empty:
                    ops.vq_kmeans_seed(inputs[-1], fresh, rng, acc.counts)
                    rng[1:].add_(1)
                quantization._store(fresh)
            report[lv] = LevelReport(inertia, empty)
        if lv < chosen[-1]:
            state = [encoder._encode(y)[0] for y in state]
    return report
