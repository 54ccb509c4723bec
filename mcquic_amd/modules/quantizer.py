"""Cascaded multi-codebook quantizer on HIP kernels (reference: mcquic/modules/quantizer.py).

`UMGMQuantizer.encode / decode` keep the reference's level cascade (:411-428) and module tree
(`_encoders.{l}.{_latentStageEncoder,_quantizationHead,_latentHead,_quantizer,_dequantizer}`,
`_decoders.{l}.{_dequantizationHead,_sideHead,_restoreHead,_dequantizer}`; the codebook is one
Parameter visible under three names, as in the reference).  The distance + argmin never materialises
the [n, m, h, w, k] tensor (ops.vq_assign), and the residual `z - dequant(code)` of the next level is
the epilogue of latentHead's last conv.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, List, Optional, Union

import torch
from torch import nn

from .. import ops
from .entropyCoder import INVALID_PMF, EntropyCoder, VariousMCoder

EPS = 1e-6
_TORCH_RAND = __import__("os").environ.get("MCQUIC_AMD_TORCH_RAND", "0") == "1"      # A/B switch: draw the uniforms with torch.rand


class _CodebookCache:
    """Packed (MFMA operand order) view of a codebook Parameter, rebuilt when the Parameter changes."""

    def __init__(self):
        self._packed: Optional[ops.PackedCodebook] = None
        self._key = None

    def invalidate(self):
        self._packed, self._key = None, None

    def get(self, codebook: torch.Tensor) -> ops.PackedCodebook:
        key = (ops.tensor_version(codebook), codebook.data_ptr())
        if self._packed is None or key != self._key:
            self._packed = ops.PackedCodebook(codebook)
            self._key = key
        return self._packed


def rateLambdas(rd_lambda, levels: int) -> tuple:
    """`rd_lambda` of encode / compress as one float per level: a float >= 0 for all levels, or a sequence of `levels` of them.
    The kernels take lambda as a float32, so every value is rounded to float32 HERE and that rounding is what is checked, cached on
    and returned (1e39 is finite as a double and inf as a float: refused).  Negative, NaN, infinite, non-numeric or of another
    length: ValueError (raised before any device work)."""
    if isinstance(rd_lambda, (list, tuple)):
        values = list(rd_lambda)
        if len(values) != levels:
            raise ValueError(f"rd_lambda: one value per level needs {levels} values, got {len(values)}")
    elif torch.is_tensor(rd_lambda) and rd_lambda.dim() > 0:
        raise ValueError("rd_lambda: a float, or a list / tuple of one float per level (not a tensor: reading it would synchronise)")
    else:
        values = [rd_lambda] * levels
    try:
        values = [float(v) for v in values]
    except (TypeError, ValueError):
        raise ValueError(f"rd_lambda: expected numbers, got {rd_lambda!r}") from None
    return tuple(ops.lambda_f32(v) for v in values)


class _RatePackCache:
    """One level's penalised packs (ops.pack_codebook_rate), valid under one (codebook version, table stamp) and keyed on lambda.  A
    pack is never rewritten in place and the cache owns it only while it is listed here: whoever launches on one beyond the call that
    asked for it -- a captured graph -- must hold it itself (`Compressor._encodeRate` stores the packs with the capture)."""
    KEEP = 4                                   # lambdas per level (a bisection walks through many; the last few stay)

    def __init__(self):
        self._state = None
        self._packs = {}

    def get(self, codebook: torch.Tensor, cdf: torch.Tensor, stamp, lam: float) -> ops.PackedCodebook:
        state = (ops.tensor_version(codebook), codebook.data_ptr(), stamp)
        if state != self._state:
            self._state, self._packs = state, {}
        pack = self._packs.pop(lam, None)
        if pack is None:
            pack = ops.pack_codebook_rate(codebook, cdf, lam)
            while len(self._packs) >= self.KEEP:
                self._packs.pop(next(iter(self._packs)))
        self._packs[lam] = pack                # (most recently used last)
        return pack

    def peek(self, codebook: torch.Tensor, stamp, lam: float) -> Optional[ops.PackedCodebook]:
        """The cached pack if it is current, building nothing (for a caller whose stream is capturing)."""
        if self._state != (ops.tensor_version(codebook), codebook.data_ptr(), stamp):
            return None
        return self._packs.get(lam)


class LowerBound(nn.Module):
    def __init__(self, bound: float):
        super().__init__()
        self.register_buffer("bound", torch.Tensor([float(bound)]))


class _multiCodebookQuantization(nn.Module):
    """reference: quantizer.py:99-239.  Parameters: `_codebook` [m, k, d] (shared), `_temperature` [m, 1, 1, 1],
    buffer `_bound.bound`."""

    def __init__(self, codebook: nn.Parameter, cache: _CodebookCache, freqEMA: Optional[nn.Parameter] = None):
        super().__init__()
        self._m, self._k, self._d = codebook.shape
        self._codebook = codebook
        self._temperature = nn.Parameter(torch.ones((self._m, 1, 1, 1)))
        if freqEMA is not None:        # ResidualBackwardQuantizer hands the level's EMA over (quantizer.py:607): a shared
            self._freqEMA = freqEMA    # Parameter, visible in the state_dict under this module as well (`_freqEMA`)
        self._bound = LowerBound(EPS)
        self._cache = [cache]          # list: keep the cache out of nn.Module's attribute registration

    @torch.no_grad()
    def reAssignCodebook(self, freq: torch.Tensor, priority: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Dead codewords (normalised frequency < 1e-6) are overwritten by the most used ones: the i-th dead codeword in
        index order receives the i-th most frequent codeword of its group; when more than k // 2 of a group are dead only
        a random k // 2 of them are refilled (reference behaviour: mcquic/modules/quantizer.py:111-136, driven by the
        CodebookReassign hook, mcquic/train/hooks.py:100-121).  Returns the flattened [m * k] mask of codewords that moved
        by more than 1e-4 in squared distance.

        One batched device-side pass over all m groups -- two sorts, a cumulative count and a gather -- with no host
        read-back (the reference loops over groups and syncs twice per group).  `priority` [m, k]: the dead codewords with
        the smallest priorities are the ones refilled when there are too many (default: fresh uniform draws; the parity
        test passes the ranks of the reference's `torch.randperm` draw)."""
        old = self._codebook.detach()
        dev = old.device
        freq = freq.detach().to(dev, torch.float32)
        m, k, d = old.shape
        half = k // 2
        dead = freq < EPS                                                       # [m, k]
        if priority is None:
            priority = torch.rand((m, k), device=dev)
        # rank of every codeword when the dead ones are lined up by priority (live ones pushed behind them)
        lineup = torch.where(dead, priority.to(dev, torch.float32), torch.full_like(freq, float("inf"))).argsort(dim=-1, stable=True)
        place = torch.empty_like(lineup).scatter_(-1, lineup, torch.arange(k, device=dev).expand(m, k))
        refill = dead & (place < half)                                          # at most k // 2 per group
        # popularity order: live codewords by frequency, then the refilled dead ones (0), then the skipped dead ones (-1);
        # a group with few dead codewords keeps its measured frequencies untouched, like the reference
        crowded = dead.sum(-1, keepdim=True) > half
        score = torch.where(crowded & dead, torch.where(refill, torch.zeros_like(freq), -torch.ones_like(freq)), freq)
        donors = score.argsort(dim=-1, descending=True, stable=True)                # [m, k] codeword indices, most used first
        slot = (refill.cumsum(-1) - 1).clamp_(min=0)                            # i for the i-th refilled codeword of a group
        source = donors.gather(-1, slot)                                        # donor index per codeword position
        moved = old.gather(1, source[..., None].expand(m, k, d))
        fresh = torch.where(refill[..., None], moved, old)
        changed = ((fresh - old) ** 2).sum(-1) > 1e-4
        self._store(fresh)
        return changed.flatten()

    @torch.no_grad()
    def syncCodebook(self):
        """Every rank takes rank 0's codebook (reference: quantizer.py:138-142): one broadcast of a detached copy, written
        back in place so the Parameter object (and the optimizer state keyed on it) stays the same."""
        import torch.distributed as dist
        from ..parallel import _staged
        buf = _staged(self._codebook.detach().clone())
        dist.broadcast(buf, 0)
        self._store(buf.to(self._codebook.device))

    def _store(self, value: torch.Tensor):
        """In-place update of the shared codebook Parameter that the packed-operand cache notices: `copy_` on the Parameter
        itself bumps its version counter (`.data.copy_` does not), and the cache is dropped explicitly as well, for
        parameters created under torch.inference_mode(), which carry no version counter."""
        self._codebook.copy_(value)
        self._cache[0].invalidate()

    def encode(self, x: torch.Tensor, how=None) -> torch.Tensor:
        """[n, m*d, h, w] -> int64 [n, m, h, w] = argmin_k ((x2 + c2) - 2 x.c), first index on ties (:144-179).  `how`, the level's
        assignment operand: None = this codebook's own cached pack; an `ops.PackedCodebook` = this codebook packed by the caller --
        `ops.pack_codebook_rate`'s, whose norms carry lambda * bits: the same kernel then returns the entropy-constrained assignment
        argmin_k (distance + lambda * bits_k); a pair (bits section, lambda buffer) = argmin_k fma(lambda_v, bits_k, distance) with one
        lambda per latent vector (`ops.vq_assign_rate_map`) on the own pack: the level's `ops.pack_bits` section, `lam` [n] or
        [n, h, w] of `ops.rate_map_levels`."""
        if isinstance(how, tuple):
            return ops.vq_assign_rate_map(x, self._cache[0].get(self._codebook), *how)
        return ops.vq_assign(x, self._cache[0].get(self._codebook) if how is None else how)

    def forward(self, x: torch.Tensor, freqEMA: torch.Tensor, uniforms=None, step=None, codebook=None):
        """Training-mode forward (:181-239), forward values only (no autograd graph yet).
        `codebook`: an alias of `self._codebook` to differentiate through (a quantizer whose codebook is shared by several levels
        hands every level its own alias so that their gradients are summed by one node, autograd.fork).

        logit = (-dist / sqrt(k)) * max(temperature, eps); random drop against the level's frequency EMA;
        gumbelSoftmax(hard=True); code = argmax(logit).  The straight-through sample y_hard - y_soft + y_soft is
        zero except at its arg-max, so it is carried as (index, hot value) instead of a dense [n, m, h, w, k]
        tensor.  `uniforms` = (u_drop, u_gumbel), the reference's two `torch.rand_like(logit)` draws; without them the
        draws are made inside the kernels that use them, from a generator snapshot (2 x 134 MB per training step that are
        never written or read; MCQUIC_AMD_TORCH_RAND=1 draws the tensors with torch.rand instead, the round-3 form).
        `step` = this level's share of the cascade's prologue launch (ops.VqStep.level: drop exponent, generator snapshot,
        code-count buffer); a stand-alone call makes its own.  Returns ((index, hot), code, logit)."""
        cb = self._cache[0].get(self._codebook)
        n, _, h, w = x.shape
        if uniforms is None and (_TORCH_RAND or not x.is_cuda):
            shape = (n, self._m, h, w, self._k)
            uniforms = (torch.rand(shape, device=x.device), torch.rand(shape, device=x.device))
        if step is None:
            # exponent of _randomDrop (:196-198) and the generator snapshot, made on the device (no host sync in the step)
            step = ops.vq_step_prologue([freqEMA], EPS, want_rng=uniforms is None).level(0)
        exponent, rng, counts = step
        if uniforms is None:
            uniforms = (None, None)
        else:
            rng = None
        if torch.is_grad_enabled():
            from ..autograd import SoftQuantizeFn
            deq, code, logit, sdeq = SoftQuantizeFn.apply(x, self._codebook if codebook is None else codebook, self._temperature, freqEMA.detach(), uniforms[0], uniforms[1],
                                                          exponent, cb, float(EPS), rng, counts)
            ops.set_silu_twin(deq, sdeq)
            return deq, code, logit           # the sample is represented by its (differentiable) dequantisation
        logit = ops.vq_logits(x, cb, self._temperature, float(EPS))
        code, index, hot = ops.vq_gumbel_sample(logit, uniforms[0], uniforms[1], freqEMA, exponent, rng, counts)
        return (index, hot), code, logit


class _multiCodebookDeQuantization(nn.Module):
    """reference: quantizer.py:242-274."""

    def __init__(self, codebook: nn.Parameter, cache: _CodebookCache):
        super().__init__()
        self._m, self._k, self._d = codebook.shape
        self._codebook = codebook
        self._cache = [cache]

    def forward(self, sample) -> torch.Tensor:
        """bmm(sample, codebook) (:262-274) for the (index, hot value) form of the straight-through sample."""
        if torch.is_tensor(sample):           # training graph: SoftQuantizeFn already produced sample @ codebook
            return sample
        index, hot = sample
        return ops.vq_dequant_soft(index, hot, self._cache[0].get(self._codebook))

    def decode(self, code: torch.Tensor, dual_silu: bool = False) -> torch.Tensor:
        """int64 [n, m, h, w] -> [n, m*d, h, w] (:249-259)."""
        return ops.vq_gather(code, self._cache[0].get(self._codebook), dual_silu=dual_silu)


class _quantizerEncoder(nn.Module):
    """reference: quantizer.py:277-328."""

    def __init__(self, quantizer, dequantizer, latentStageEncoder, quantizationHead, latentHead):
        super().__init__()
        self._quantizer = quantizer
        self._dequantizer = dequantizer
        self._latentStageEncoder = latentStageEncoder
        self._quantizationHead = quantizationHead
        self._latentHead = latentHead

    @property
    def Codebook(self):
        return self._quantizer._codebook

    def syncCodebook(self):
        self._quantizer.syncCodebook()

    def reAssignCodebook(self, freq: torch.Tensor) -> torch.Tensor:
        return self._quantizer.reAssignCodebook(freq)

    def encode(self, x: torch.Tensor, how=None):
        residual, code, _ = self._encode(x, how)
        return residual, code

    def _encode(self, x: torch.Tensor, how=None):
        """(residual for the next level or None, code, the tensor `_quantizer.encode` received).  `how`: see
        `_multiCodebookQuantization.encode` (the residual is taken from the plain codebook's row of the code whatever it is)."""
        from ..nn import blocks
        z = self._latentStageEncoder(x)
        head = self._latentHead
        if head is None:
            qin = self._quantizationHead(z)
            return None, self._quantizer.encode(qin, how), qin
        if blocks.lockstep_ok([self._quantizationHead, head], [z, z]):
            # latentHead(z) does not depend on the codes until its closing conv: everything before that runs in lockstep with
            # quantizationHead (same layer shapes on the same z: one multi-problem launch per layer, four problems in the
            # AttentionBlocks)
            last = len(head) - 1
            q, t = blocks.lockstep_infer([self._quantizationHead, head], [z, z], layers=last)
            qin = self._quantizationHead[last](q)
            code = self._quantizer.encode(qin, how)
        else:
            qin = self._quantizationHead(z)
            code = self._quantizer.encode(qin, how)
            t = z
            for i in range(len(head) - 1):
                t = head[i](t)
        deq = self._dequantizer.decode(code)
        # z' - dequant(code): the subtraction is the epilogue of latentHead's closing conv3x3 (:318)
        return head[len(head) - 1](t, res=deq, res_scale=-1.0, dual_silu=True), code, qin


    def _forward(self, x: torch.Tensor, freqEMA: torch.Tensor, uniforms=None, step=None):
        """Training-mode level (:295-305): returns (sample, residual for the next level, code, logit)."""
        z = self._latentStageEncoder(x)
        if self._latentHead is None:
            q, code, logit = self._quantizer(self._quantizationHead(z), freqEMA, uniforms, step)
            return q, None, code, logit
        head = self._latentHead
        if torch.is_grad_enabled():
            # latentHead(z) does not depend on the codes: it runs in lockstep with quantizationHead -- same layer shapes,
            # one multi-problem launch per layer for both (autograd.LockstepFn; 15 + 15 convolutions, launch-bound on the
            # 16x16 ... 4x4 maps of a training crop, become 10 launches each way)
            from .. import autograd as AG
            hz, qin = AG.lockstep([head, self._quantizationHead], [z, z])
            q, code, logit = self._quantizer(qin, freqEMA, uniforms, step)
            # z' - dequant (:303); the sample's second use (the decoder) goes through the same node, so that its two gradients
            # meet in one launch of ours
            residual, q = AG.sub_pass(hz, self._dequantizer(q))
            return q, residual, code, logit
        q, code, logit = self._quantizer(self._quantizationHead(z), freqEMA, uniforms, step)
        deq = self._dequantizer(q)
        t = z
        for i in range(len(head) - 1):
            t = head[i](t)
        return q, head[len(head) - 1](t, res=deq, res_scale=-1.0, dual_silu=True), code, logit

    def forward(self, x: torch.Tensor, freqEMA: torch.Tensor, uniforms=None, step=None):
        return self._forward(x, freqEMA, uniforms, step)


class _quantizerDecoder(nn.Module):
    """reference: quantizer.py:330-365."""

    def __init__(self, dequantizer, dequantizationHead, sideHead, restoreHead):
        super().__init__()
        self._dequantizer = dequantizer
        self._dequantizationHead = dequantizationHead
        self._sideHead = sideHead
        self._restoreHead = restoreHead

    def decode(self, code: torch.Tensor, formerLevel: Optional[torch.Tensor]):
        from ..nn import blocks
        deq = self._dequantizer.decode(code, dual_silu=True)
        if self._sideHead is None:
            return self._restoreHead(self._dequantizationHead(deq))
        if blocks.lockstep_ok([self._dequantizationHead, self._sideHead], [deq, formerLevel]):
            q, side = blocks.lockstep_infer([self._dequantizationHead, self._sideHead], [deq, formerLevel])    # independent until their sum
        else:
            q, side = self._dequantizationHead(deq), self._sideHead(formerLevel)
        return self._restoreHead(ops.add(q, side, dual_silu=True))                # q + sideHead(formerLevel) (:354)


    def forward(self, q, formerLevel: Optional[torch.Tensor]):
        """Training-mode level (:359-365): like decode, from the straight-through sample."""
        if self._sideHead is not None and torch.is_grad_enabled():
            from .. import autograd as AG                      # sideHead and dequantizationHead in lockstep (see _quantizerEncoder._forward)
            x, side = AG.lockstep([self._dequantizationHead, self._sideHead], [self._dequantizer(q), formerLevel])
            return self._restoreHead(AG.add(x, side, dual_silu=True))
        from ..nn import blocks
        x = blocks.run_stack(self._dequantizationHead, self._dequantizer(q))
        if self._sideHead is not None:
            if torch.is_grad_enabled():
                from .. import autograd as AG
                x = AG.add(x, self._sideHead(formerLevel), dual_silu=True)
            else:
                x = ops.add(x, self._sideHead(formerLevel), dual_silu=True)
        return self._restoreHead(x)


class BaseQuantizer(nn.Module):
    """reference: quantizer.py:32-78."""

    def __init__(self, m: int, k: List[int]):
        super().__init__()
        self._entropyCoder = EntropyCoder(m, k)
        self._m = m
        self._k = k

    @property
    def CDFs(self):
        return self._entropyCoder.CDFs

    @property
    def NormalizedFreq(self):
        return self._entropyCoder.NormalizedFreq

    def _stepPrologue(self, x: torch.Tensor, uniforms):
        """The per-step bookkeeping of all levels in ONE launch (ops.vq_step_prologue): every level's drop exponent and generator
        snapshot, and the zeroed code-count buffer of the entropy coder that the sampling kernels add into.  HIP devices only:
        the training forward has no CPU / PyTorch path (a level run on its own makes its own prologue launch, equally on the device)."""
        if not x.is_cuda:
            raise NotImplementedError(f"mcquic_amd: the training forward of {type(self).__name__} runs on a HIP device only (input on "
                                      f"{x.device}); there is no CPU / PyTorch fallback -- move the model and the batch to cuda")
        coder = self._entropyCoder
        want_rng = uniforms is None and not _TORCH_RAND
        return ops.vq_step_prologue(list(coder._freqEMA), EPS, want_rng, coder.countBuffer(x.device))

    def _checkCoder(self, coder: str) -> bool:
        """True for the device coder (csrc/rans_dev.hip), False for the host coder (csrc/rans.cpp), the default; same bytes either way."""
        if coder not in ("host", "device"):
            raise ValueError(f"coder must be 'host' or 'device', got {coder!r}")
        if coder == "device" and not hasattr(self._entropyCoder, "compressDevice"):
            raise NotImplementedError(f"{type(self._entropyCoder).__name__} writes raw codes, not rANS streams: it has no device coder")
        return coder == "device"

    def rateLambdas(self, rd_lambda) -> tuple:
        """`rd_lambda` checked and spread over the levels (`rateLambdas`); quantizers without 16-bit tables refuse."""
        if not isinstance(self._entropyCoder, EntropyCoder):
            raise NotImplementedError(f"{type(self).__name__} has no rate-constrained encoding: its {type(self._entropyCoder).__name__} "
                                      "writes raw codes and keeps no 16-bit tables to take the penalties from")
        return rateLambdas(rd_lambda, len(self._k))

    def _checkLanes(self, lanes) -> dict:
        """The coder's `lanes` keyword for a request of the lane-interleaved layout, {} for the plain one (None / False): the plain
        calls stay as they were.  Coders that write raw codes have no rANS streams to interleave."""
        if lanes is None or lanes is False:
            return {}
        if not isinstance(self._entropyCoder, EntropyCoder):
            raise NotImplementedError(f"{type(self._entropyCoder).__name__} writes raw codes, not rANS streams: it has no lanes layout")
        return {"lanes": lanes}

    def compress(self, x: torch.Tensor, coder: str = "host", rd_lambda=None, rd_map=None, lanes=None):
        device = self._checkCoder(coder)
        layout = self._checkLanes(lanes)
        rate = {}
        if rd_lambda is not None or rd_map is not None:
            self.rateLambdas(1.0 if rd_lambda is None else rd_lambda)          # (quantizers without tables refuse here)
            rate = dict(rd_lambda=rd_lambda, rd_map=rd_map)
        codes = self.encode(x, **rate)
        if device:
            streams = self._entropyCoder.compressDevice(codes, **layout)
            return codes, streams.tobytes(), streams.codeSizes
        binaries, codeSize = self._entropyCoder.compress(codes, **layout)
        return codes, binaries, codeSize

    def decompress(self, binaries, codeSize, coder: str = "host", lanes: bool = False) -> torch.Tensor:
        layout = self._checkLanes(lanes)
        if self._checkCoder(coder):
            return self.decode(self._entropyCoder.decompressDevice(binaries, codeSize, **layout))
        return self.decode(self._entropyCoder.decompress(binaries, codeSize, **layout))


class UMGMQuantizer(BaseQuantizer):
    """reference: quantizer.py:368-467."""
    _components = ["latentStageEncoder", "quantizationHead", "latentHead", "dequantizationHead", "sideHead", "restoreHead"]

    def __init__(self, channel: int, m: int, k: Union[int, List[int]], permutationRate: float,
                 components: Dict[str, Callable[[], nn.Module]]):
        if isinstance(k, int):
            k = [k]
        super().__init__(m, k)
        lse, qh, lh, dqh, sh, rh = [components[key] for key in self._components]
        encoders, decoders = [], []
        for i, ki in enumerate(k):
            last = i == len(k) - 1
            # SmallInit, N(0, 2 / (5 d)) (quantizer.py:394-398)
            codebook = nn.Parameter(nn.init.normal_(torch.empty(m, ki, channel // m), std=math.sqrt(2 / (5 * channel / m))))
            cache = _CodebookCache()
            quantizer = _multiCodebookQuantization(codebook, cache)
            dequantizer = _multiCodebookDeQuantization(codebook, cache)
            encoders.append(_quantizerEncoder(quantizer, dequantizer, lse(), qh(), None if last else lh()))
            decoders.append(_quantizerDecoder(dequantizer, dqh(), None if last else sh(), rh()))
        self._encoders = nn.ModuleList(encoders)
        self._decoders = nn.ModuleList(decoders)

    @property
    def Codebooks(self):
        return list(encoder.Codebook for encoder in self._encoders)

    def encode(self, x: torch.Tensor, rd_lambda=None, packs=None, rd_map=None, scales_dev=None) -> List[torch.Tensor]:
        """`rd_lambda`: None = the plain nearest-codeword cascade; a float >= 0, or one per level, = every level picks
        argmin_k (distance + lambda * bits_k), bits_k = what the coder's 16-bit table of that level charges for code k
        (`ratePacks`).  Same decoder, same streams.  `packs`: the result of `ratePacks`, made by a caller that must not build
        them here (a graph capture).
        `rd_map`: rate control per image or per region -- a float32 device tensor, [n] (one lambda per image) or [n, h0, w0] (one per
        level-0 code cell; the levels below take the mean of their 2 x 2 cells, `ops.rate_map_levels`).  `rd_lambda` is then the
        per-level scale (None = 1), lambda = fl32(scale_l * map_l) an operand of the assignment kernel, not a constant of a pack: the
        map's values are never read on the host, any map and any scale run the same launches on the plain packs and the tables'
        `rateBitsPacks`.  A negative, NaN or infinite map value counts as 0 and shows in `rateMapError()`.  `scales_dev`: the scales
        again as a device tensor the kernel reads instead (for a capture whose replays take new scales).  A caller that captures this
        call into a graph of its own keeps `rateBitsPacks()`'s list with that graph, as it keeps `ratePacks` for the scalar path: the
        graph launches on those sections, and the cache here lets go of them when the tables change."""
        return self._cascade(x, self._levelOperands(x, rd_lambda, packs, rd_map, scales_dev))

    def _levelOperands(self, y: torch.Tensor, rd_lambda=None, packs=None, rd_map=None, scales_dev=None) -> list:
        """`encode`'s arguments as one assignment operand per level (`_multiCodebookQuantization.encode`'s `how`) for the latent `y`:
        None (plain), the penalised pack (the scalar knob) or (bits section, lambda buffer) (the map).  For a map everything is checked
        on the host first, then ONE launch (`ops.rate_map_levels`).  The error word is a fresh tensor on every call -- inside a capture it
        belongs to that graph's pool, so no replay ever writes a word that a later call has replaced -- and becomes what
        `rateMapError()` returns."""
        if rd_map is not None:
            if packs is not None:
                raise ValueError("rd_map: `packs` belong to the scalar rd_lambda path")
            scales = self.rateLambdas(1.0 if rd_lambda is None else rd_lambda)
            self.checkRateMap(rd_map, int(y.shape[0]), (int(y.shape[-2]) + 1) // 2, (int(y.shape[-1]) + 1) // 2, y.device)
            bits = self.rateBitsPacks()
            lams, self.__dict__["_rateMapErr"] = ops.rate_map_levels(rd_map, scales, scales_dev=scales_dev)
            return list(zip(bits, lams))
        if packs is not None:
            return packs
        return [None] * len(self._encoders) if rd_lambda is None else self.ratePacks(self.rateLambdas(rd_lambda))

    def _cascade(self, x: torch.Tensor, hows, each=None) -> List[torch.Tensor]:
        """The level cascade, the one copy: level l assigns by `hows[l]` and hands its residual down.  `each(level, code, qin)`: called as
        soon as a level's launches are enqueued, qin = what its `_quantizer.encode` received."""
        codes = []
        for lv, (encoder, how) in enumerate(zip(self._encoders, hows)):
            x, code, qin = encoder._encode(x, how)
            codes.append(code)
            if each is not None:
                each(lv, code, qin)
        return codes

    def _rateTables(self):
        """(the coder's current `deviceCDFs(normalize=False)`, their stamp); their status is read once per stamp (one small copy to the
        host): a row `compress` would refuse raises its ValueError."""
        coder = self._entropyCoder
        tables = coder.deviceCDFs(False)
        stamp = coder.deviceCDFBuiltStamp(False)
        if self.__dict__.get("_rateChecked") != stamp:
            if bool(coder.deviceCDFStatus(False).any()):
                raise ValueError(INVALID_PMF)
            self.__dict__["_rateChecked"] = stamp
        return tables, stamp

    @torch.no_grad()
    def ratePacks(self, lams) -> List[ops.PackedCodebook]:
        """One penalised pack per level for the lambdas of `rateLambdas`: penalties from `deviceCDFs(normalize=False)`, the tables
        `compress` codes with.  Cached per level on (codebook version, the tables' stamp, lambda): two small launches per level when
        one of them changed, none otherwise.  When the tables were rebuilt their status is read once (one small copy to the host);
        a row `compress` would refuse raises its ValueError here.  While the current stream is capturing nothing is built: the
        packs must be cached and current (made by an earlier call outside the capture), else RuntimeError.  The cache keeps a few
        lambdas per level; a caller that launches on a pack later than this call returns must keep the pack itself."""
        coder = self._entropyCoder
        caches = self.__dict__.get("_rateCaches")
        if caches is None:
            caches = self.__dict__["_rateCaches"] = [_RatePackCache() for _ in self._encoders]
        if self._entropyCoder._freqEMA[0].is_cuda and torch.cuda.is_current_stream_capturing():
            # inside a caller's capture nothing may be built or read back: only packs that are cached and current are handed out
            stamp = coder.deviceCDFStamp()
            packs = [cache.peek(encoder.Codebook, stamp, lam) for cache, encoder, lam in zip(caches, self._encoders, lams)]
            if stamp != coder.deviceCDFBuiltStamp(False) or any(p is None for p in packs):
                raise RuntimeError("rd_lambda inside a stream capture needs its packs made beforehand: call encode(x, rd_lambda=...) with "
                                   "these lambdas once outside the capture (and again after the codebooks or the tables change)")
            return packs
        tables, stamp = self._rateTables()
        return [cache.get(encoder.Codebook, table, stamp, lam)
                for cache, encoder, table, lam in zip(caches, self._encoders, tables, lams)]

    @staticmethod
    def checkRateMap(rd_map, n: int, h0: int, w0: int, device) -> None:
        """ValueError, before any launch, unless `rd_map` is a float32 tensor on `device`, [n] or [n, h0, w0] with h0 x w0 the level-0
        code grid (half the latent's size, with ceil)."""
        if not torch.is_tensor(rd_map):
            raise ValueError(f"rd_map: expected a float32 tensor, got {type(rd_map).__name__}")
        if rd_map.dtype != torch.float32:
            raise ValueError(f"rd_map: must be float32, got {rd_map.dtype}")
        if rd_map.device != device:
            raise ValueError(f"rd_map: lives on {rd_map.device}, the images on {device}")
        if tuple(rd_map.shape) not in ((n,), (n, h0, w0)):
            raise ValueError(f"rd_map: expected [{n}] (per image) or [{n}, {h0}, {w0}] (the level-0 code grid), got {tuple(rd_map.shape)}")

    @torch.no_grad()
    def rateBitsPacks(self) -> List[torch.Tensor]:
        """One `ops.pack_bits` section per level from `deviceCDFs(normalize=False)`, cached on the tables' stamp alone (they depend on
        neither lambda nor the codebooks): one small launch per level when the tables changed, none otherwise.  The tables' status is
        read once per stamp, as in `ratePacks`, with its ValueError.  While the current stream is capturing nothing is built: the
        sections must be cached and current, else RuntimeError."""
        coder = self._entropyCoder
        cached = self.__dict__.get("_rateBits")                                     # (stamp, [sections])
        if coder._freqEMA[0].is_cuda and torch.cuda.is_current_stream_capturing():
            stamp = coder.deviceCDFStamp()
            # (cached[0] is the stamp of tables that were built and checked outside a capture; `codeBits` inside this capture may have
            #  re-issued the table launch since, which clears the built stamp but not what the sections were made from)
            if cached is None or cached[0] != stamp:
                raise RuntimeError("rd_map inside a stream capture needs its bits sections made beforehand: call encode(x, rd_map=...) once "
                                   "outside the capture (and again after the tables change)")
            return cached[1]
        tables, stamp = self._rateTables()
        if cached is None or cached[0] != stamp:
            cached = self.__dict__["_rateBits"] = (stamp, [ops.pack_bits(t) for t in tables])
        return cached[1]

    def rateMapError(self) -> torch.Tensor:
        """int32 [n] on the device, from the last `encode(..., rd_map=...)` issued here: 1 where an image's map held a negative, NaN or
        infinite value (taken as 0).  Nothing is read here.  Every call writes a word of its own; the word of a call that a caller
        captured is that graph's, rewritten by each replay, and is what this returns until another call is issued
        (`Compressor.rateMapError` also follows the replays of `enableGraphs`)."""
        err = self.__dict__.get("_rateMapErr")
        if err is None:
            raise RuntimeError("rateMapError: no encode with `rd_map` has run yet")
        return err

    def rateState(self):
        """What a penalised encode depends on besides the lambdas and the weights of the layers: every level's codebook (version,
        address) and the tables' stamp.  Nothing is launched or read."""
        return (tuple((ops.tensor_version(e.Codebook), e.Codebook.data_ptr()) for e in self._encoders), self._entropyCoder.deviceCDFStamp())

    def quantizerInputs(self, y: torch.Tensor) -> List[torch.Tensor]:
        """What each level's `_quantizer.encode` receives on the inference path under the current codebooks: `encode`'s cascade
        (the very same launches, lockstep paths included) with the quantization heads' outputs kept -- the data a level's codebook
        is fitted to (mcquic_amd.kmeans)."""
        inputs = []
        self._cascade(y, self._levelOperands(y), lambda lv, code, qin: inputs.append(qin))
        return inputs

    def compress(self, x: torch.Tensor, coder: str = "host", rd_lambda=None, rd_map=None, lanes=None):
        """`encode` + the entropy coder (mcquic/modules/entropyCoder.py:108-126) with the coder taken level by level: a level's codes
        leave for the host (a copy in stream order, then a host thread) as soon as they are enqueued, while the GPU computes the levels below it --
        level 0 holds three quarters of the symbols and is ready first.  Same codes, same bytes as encode() + coder.compress().
        `rd_lambda`, `rd_map`: as for `encode` (the same overlap with either).  `lanes`: the lane-interleaved layout
        (`EntropyCoder.compress`), which takes the all-levels path as the device coder does."""
        from .entropyCoder import CODER_OVERLAP
        if self._checkLanes(lanes):
            return super().compress(x, coder, rd_lambda, rd_map, lanes=lanes)
        if self._checkCoder(coder) or not (CODER_OVERLAP and x.is_cuda):     # (the device coder takes all levels in one launch)
            return super().compress(x, coder, rd_lambda, rd_map)
        hows = self._levelOperands(x, rd_lambda, rd_map=rd_map)
        job = self._entropyCoder.beginCompress(len(self._encoders))
        codes = self._cascade(x, hows, lambda lv, code, qin: job.submit(lv, code))
        binaries, codeSize = job.finish()
        return codes, binaries, codeSize

    def decompress(self, binaries, codeSize, coder: str = "host", lanes: bool = False) -> torch.Tensor:
        """The coder's streams -> `decode` (entropyCoder.py:141-154) with the levels decoded on a host thread in the order the decoder
        cascade consumes them -- the last (smallest) level first: its kernels are enqueued while the larger levels are still being
        decoded.  `lanes`: True for lane-interleaved streams (the all-levels path)."""
        from .entropyCoder import CODER_OVERLAP
        if self._checkLanes(lanes):
            return super().decompress(binaries, codeSize, coder, lanes=lanes)
        if self._checkCoder(coder) or not (CODER_OVERLAP and self._entropyCoder._freqEMA[0].is_cuda):
            return super().decompress(binaries, codeSize, coder)
        job = self._entropyCoder.beginDecompress(binaries, codeSize)
        formerLevel = None
        for lv in reversed(range(len(self._decoders))):
            formerLevel = self._decoders[lv].decode(job.level(lv), formerLevel)
        return formerLevel

    def decode(self, codes: List[torch.Tensor]) -> Optional[torch.Tensor]:
        if len(codes) != len(self._decoders):
            raise RuntimeError(f"expected {len(self._decoders)} code levels, got {len(codes)}")
        self._entropyCoder._checkShape(codes)
        formerLevel = None
        for decoder, code in zip(self._decoders[::-1], codes[::-1]):
            formerLevel = decoder.decode(code, formerLevel)
        return formerLevel

    def forward(self, x: torch.Tensor, uniforms=None):
        """Training-mode forward (:443-467), forward values only: per level soft-assign with the level's frequency EMA
        (the reference snapshot passes `permutationRate` where this tensor belongs, :399 -- repaired here), decoders in
        reverse, then the code-frequency EMA update with its all-reduce (entropyCoder.py:28-44).
        `uniforms`: optional list of (u_drop, u_gumbel) per level.  Returns (yHat, codes, logits)."""
        quantizeds, codes, logits = [], [], []
        st = self._stepPrologue(x, uniforms)
        for lv, encoder in enumerate(self._encoders):
            quantized, x, code, logit = encoder(x, self._entropyCoder._freqEMA[lv], None if uniforms is None else uniforms[lv],
                                                None if st is None else st.level(lv))
            quantizeds.append(quantized)
            codes.append(code)
            logits.append(logit)
        formerLevel = None
        for decoder, quantized in zip(self._decoders[::-1], quantizeds[::-1]):
            formerLevel = decoder(quantized, formerLevel)
        self._entropyCoder(codes, counts=None if st is None else st.counts)
        return formerLevel, codes, logits

    def reAssignCodebook(self) -> torch.Tensor:
        """reference: quantizer.py:430-436."""
        freqs = self.NormalizedFreq
        reassigned = [encoder.reAssignCodebook(freq) for encoder, freq in zip(self._encoders, freqs)]
        return torch.cat(reassigned).float().mean()

    def syncCodebook(self):
        """reference: quantizer.py:438-441."""
        import torch.distributed as dist
        dist.barrier()
        for encoder in self._encoders:
            encoder.syncCodebook()



class VariousMQuantizer(BaseQuantizer):
    """reference: quantizer.py:88-93 (group count per level, statistics in a VariousMCoder)."""

    def __init__(self, m: List[int], k: List[int]):
        nn.Module.__init__(self)
        self._entropyCoder = VariousMCoder(m, k)
        self._m = m
        self._k = k


class _plainHeadEncoder(_quantizerEncoder):
    """`_quantizerEncoder` whose `quantizationHead` / `latentHead` are nn.Identity() (NeonQuantizer, quantizer.py:490-491): the codes
    come straight from the latent-stage encoder's output, and EVERY level -- the last one too -- returns z - dequant(code)
    (quantizer.py:310-318 with `latentHead` never None)."""

    def encode(self, x: torch.Tensor):
        z = self._latentStageEncoder(x)
        code = self._quantizer.encode(z)
        return ops.axpby(z, self._dequantizer.decode(code), 1.0, -1.0), code

    def forward(self, *a, **kw):
        raise NotImplementedError("NeonQuantizer's training forward raises in the reference snapshot too (it hands the float 0.5 to "
                                  "_multiCodebookQuantization where the frequency EMA tensor belongs, quantizer.py:493,194-200)")


class _plainHeadDecoder(_quantizerDecoder):
    """`_quantizerDecoder` with nn.Identity() `dequantizationHead` / `sideHead` (quantizer.py:497-498): q + formerLevel, restoreHead."""

    def decode(self, code: torch.Tensor, formerLevel: Optional[torch.Tensor]):
        q = self._dequantizer.decode(code)
        return self._restoreHead(q if self._sideHead is None else ops.add(q, formerLevel))

    def forward(self, *a, **kw):
        raise NotImplementedError("NeonQuantizer's training forward raises in the reference snapshot too (quantizer.py:493)")


class NeonQuantizer(VariousMQuantizer):
    """reference: quantizer.py:469-573 -- the one quantizer class of that file no model or config of the snapshot instantiates: a
    32-channel cascade like UMGMQuantizer's with a group count PER LEVEL (`m[i]` codebooks of 32 / m[i] dimensions, k[i] codewords),
    identity heads, and a latent-stage encoder / restore head per level (ResidualBlock, AttentionBlock, strided / shuffle block, a
    bias-free 1x1 convolution).  Same module tree and state_dict keys; inference only (encode / decode / compress / decompress,
    Codebooks, reAssignCodebook): the reference's own training forward raises (see `_plainHeadEncoder.forward`)."""

    def __init__(self, m: List[int], k: List[int]):
        if not isinstance(k, list):
            raise AttributeError
        from ..nn import AttentionBlock, ResidualBlock, ResidualBlockShuffle, ResidualBlockWithStride, conv1x1
        super().__init__(m, k)
        encoders, decoders = [], []
        for i, (ki, mi) in enumerate(zip(k, m)):
            codebook = nn.Parameter(nn.init.normal_(torch.empty(mi, ki, 32 // mi), std=math.sqrt(2 / (5 * 32 / float(mi)))))
            cache = _CodebookCache()
            quantizer = _multiCodebookQuantization(codebook, cache)
            dequantizer = _multiCodebookDeQuantization(codebook, cache)
            lse = nn.Sequential(ResidualBlock(32, 32), AttentionBlock(32), ResidualBlockWithStride(32, 32), conv1x1(32, 32, bias=False))
            restore = nn.Sequential(conv1x1(32, 32, bias=False), ResidualBlockShuffle(32, 32), AttentionBlock(32), ResidualBlock(32, 32))
            encoders.append(_plainHeadEncoder(quantizer, dequantizer, lse, nn.Identity(), nn.Identity()))
            decoders.append(_plainHeadDecoder(dequantizer, nn.Identity(), nn.Identity() if i < len(k) - 1 else None, restore))
        self._encoders = nn.ModuleList(encoders)
        self._decoders = nn.ModuleList(decoders)

    @property
    def Codebooks(self):
        return list(encoder.Codebook for encoder in self._encoders)

    def encode(self, x: torch.Tensor) -> List[torch.Tensor]:
        codes = []
        for encoder in self._encoders:
            x, code = encoder.encode(x)
            codes.append(code)
        return codes

    def decode(self, codes: List[torch.Tensor]) -> Optional[torch.Tensor]:
        if len(codes) != len(self._decoders):
            raise RuntimeError(f"expected {len(self._decoders)} code levels, got {len(codes)}")
        formerLevel = None
        for decoder, code in zip(self._decoders[::-1], codes[::-1]):
            formerLevel = decoder.decode(code, formerLevel)
        return formerLevel

    def reAssignCodebook(self) -> torch.Tensor:
        reassigned = [encoder.reAssignCodebook(freq) for encoder, freq in zip(self._encoders, self.NormalizedFreq)]
        return torch.cat(reassigned).float().mean()

    def syncCodebook(self):
        import torch.distributed as dist
        dist.barrier()
        for encoder in self._encoders:
            encoder.syncCodebook()

    def forward(self, x: torch.Tensor):
        raise NotImplementedError("NeonQuantizer's training forward raises in the reference snapshot too (it hands the float 0.5 to "
                                  "_multiCodebookQuantization where the frequency EMA tensor belongs, quantizer.py:493,194-200)")


class ResidualBackwardQuantizer(VariousMQuantizer):
    """The quantizer of `Neon` (reference: quantizer.py:577-765): ONE codebook [1, k, 8] shared by all levels; every level has
    a latent-stage encoder (down), a `backward` stack and a `restoreHead` (both up); codes are produced from the SMALLEST
    level up, each level quantizing what the coarser levels' `backward` stacks did not explain, and come out small -> large.
    Same module tree / state_dict keys as the reference (`_encoders`, `_decoders`, `_backwards`, `_quantizers`,
    `_dequantizers`); the layers are the HIP-backed ones of mcquic_amd.nn."""

    def __init__(self, k: int, size: List[int], denseNorm: bool = False):
        from ..nn import AttentionBlock, ResidualBlock, ResidualBlockShuffle, ResidualBlockWithStride, conv1x1
        channel = 8
        self.channel = channel
        super().__init__([1] * len(size), [k] * len(size))
        codebook = nn.Parameter(nn.init.trunc_normal_(torch.empty(1, k, channel), std=math.sqrt(2 / (5 * channel))))
        cache = _CodebookCache()
        encoders, backwards, decoders, quantizers, dequantizers = [], [], [], [], []
        lastSize = size[0] * 2
        for i, thisSize in enumerate(size):
            if thisSize == lastSize // 2:
                down = lambda: ResidualBlockWithStride(channel * 4, channel * 4, 2, 1, denseNorm)       # noqa: E731
                up = lambda: ResidualBlockShuffle(channel * 4, channel * 4, 2, 1, denseNorm)            # noqa: E731
            elif thisSize == lastSize:
                down = up = lambda: ResidualBlock(channel * 4, channel * 4, 1, denseNorm)               # noqa: E731
            else:
                raise ValueError("The given size sequence does not half or equal to from left to right.")
            lastSize = thisSize

            def upStack():
                return nn.Sequential(conv1x1(channel, channel * 4, bias=False), up(), AttentionBlock(channel * 4, 1, denseNorm),
                                     ResidualBlock(channel * 4, channel, 1, denseNorm))
            encoders.append(nn.Sequential(ResidualBlock(channel, channel * 4, 1, denseNorm), AttentionBlock(channel * 4, 1, denseNorm),
                                          down(), conv1x1(channel * 4, channel, bias=False)))
            backwards.append(upStack() if i < len(size) - 1 else nn.Identity())
            decoders.append(upStack())
            # NOTE (reference): quantizers run large -> small, `_freqEMA` is stored small -> large
            quantizers.append(_multiCodebookQuantization(codebook, cache, self._entropyCoder._freqEMA[-(i + 1)]))
            dequantizers.append(_multiCodebookDeQuantization(codebook, cache))
        self._encoders = nn.ModuleList(encoders)
        self._decoders = nn.ModuleList(decoders)
        self._backwards = nn.ModuleList(backwards)
        self._quantizers = nn.ModuleList(quantizers)
        self._dequantizers = nn.ModuleList(dequantizers)

    @property
    def Codebooks(self):
        return list(quantizer._codebook for quantizer in self._quantizers)

    def _latents(self, x: torch.Tensor) -> List[torch.Tensor]:
        latents = []
        grad = self.training and torch.is_grad_enabled()
        for i, encoder in enumerate(self._encoders):
            x = encoder(x)
            if grad and i + 1 < len(self._encoders):
                from .. import autograd as AG
                x, keep = AG.fork(x, 2)            # (a level's latent feeds the next level AND its own residual: one node sums the two gradients)
                latents.append(keep)
            else:
                latents.append(x)
        return latents

    def encode(self, x: torch.Tensor) -> List[torch.Tensor]:
        """quantizer.py:676-694."""
        latents = self._latents(x)
        codes, current = [], None
        for quantizer, dequantizer, backward, latent in zip(self._quantizers[::-1], self._dequantizers[::-1], self._backwards[::-1],
                                                            latents[::-1]):
            residual = latent if current is None else ops.axpby(latent, current, 1.0, -1.0)      # (latent - 0 is latent, bit for bit)
            code = quantizer.encode(residual)
            codes.append(code)
            current = backward(dequantizer.decode(code))
        return codes

    def decode(self, codes: List[torch.Tensor]) -> Optional[torch.Tensor]:
        """quantizer.py:696-704."""
        if len(codes) != len(self._decoders):
            raise RuntimeError(f"expected {len(self._decoders)} code levels, got {len(codes)}")
        self._entropyCoder._checkShape(codes)
        formerLevel = None
        for decoder, dequantizer, code in zip(self._decoders[::-1], self._dequantizers[::-1], codes):
            quantized = dequantizer.decode(code)
            formerLevel = decoder(quantized if formerLevel is None else ops.add(quantized, formerLevel))
        return formerLevel

    def residual_backward(self, code: torch.Tensor, level: int) -> torch.Tensor:
        """quantizer.py:671-674."""
        return self._backwards[-level](self._dequantizers[-level].decode(code))

    def residual_forward(self, code: torch.Tensor, formerLevel: Optional[torch.Tensor], level: int) -> torch.Tensor:
        """quantizer.py:706-713."""
        if formerLevel is None and level > 0:
            raise RuntimeError("For reconstruction after level-0, you should provide not None formerLevel as input.")
        if formerLevel is not None and level == 0:
            raise RuntimeError("For reconstruction at level-0, you should provide None formerLevel as input.")
        decoder, dequantizer = self._decoders[-(level + 1)], self._dequantizers[-(level + 1)]
        quantized = dequantizer.decode(code)
        return decoder(ops.add(quantized, formerLevel)) if formerLevel is not None else decoder(quantized)

    def reAssignCodebook(self) -> torch.Tensor:
        """quantizer.py:715-721."""
        reassigned = [quantizer.reAssignCodebook(freq) for quantizer, freq in zip(self._quantizers, self.NormalizedFreq)]
        return torch.cat(reassigned).float().mean()

    def syncCodebook(self):
        """quantizer.py:723-726."""
        import torch.distributed as dist
        dist.barrier()
        for quantizer in self._quantizers:
            quantizer.syncCodebook()

    def forward(self, x: torch.Tensor, uniforms=None):
        """Training-mode forward (quantizer.py:727-765): (yHat, codes, logits), codes / logits small -> large;
        `uniforms[j]` = (u_drop, u_gumbel) of the j-th quantization (smallest level first)."""
        from .. import autograd as AG
        grad = torch.is_grad_enabled()
        latents = self._latents(x)
        quantizeds, codes, logits = [], [], []
        current = None
        st = self._stepPrologue(x, uniforms)          # (the j-th quantization reads `_entropyCoder._freqEMA[j]`, see __init__)
        # ONE codebook under every level: each level differentiates through its own alias and one node sums the gradients
        cbs = AG.fork(self._quantizers[0]._codebook, len(self._quantizers)) if grad else [None] * len(self._quantizers)
        for j, (quantizer, dequantizer, backward, latent) in enumerate(zip(self._quantizers[::-1], self._dequantizers[::-1],
                                                                           self._backwards[::-1], latents[::-1])):
            if current is None:
                residual = latent
            else:
                residual = AG.sub(latent, current) if grad else ops.axpby(latent, current, 1.0, -1.0)
            sample, code, logit = quantizer(residual, quantizer._freqEMA, None if uniforms is None else uniforms[j],
                                            None if st is None else st.level(j), cbs[j])
            quantized = dequantizer(sample)
            # (two consumers: the decoder side and the `backward` stack -- or, behind the last level's identity, the next residual)
            quantized, forBackward = AG.fork(quantized, 2) if grad else (quantized, quantized)
            quantizeds.append(quantized)
            codes.append(code)
            logits.append(logit)
            current = backward(forBackward)
        formerLevel = None
        for decoder, quantized in zip(self._decoders[::-1], quantizeds):
            if formerLevel is None:
                formerLevel = decoder(quantized)                                  # (0 + quantized is quantized, bit for bit)
            else:
                formerLevel = decoder(AG.add(formerLevel, quantized) if grad else ops.add(formerLevel, quantized))
        self._entropyCoder(codes, counts=None if st is None else st.counts)
        return formerLevel, codes, logits
