"""`Compressor` with the reference's API surface on HIP kernels (reference: mcquic/modules/compressor.py).

    Compressor(channel, m, k, permutationRate=0.0)         # compressor.py:121
    .encode(x) -> List[LongTensor [n, m, h_l, w_l]]        # :79-88
    .decode(codes) -> Tensor [n, 3, H, W]                  # :114-117
    .compress(x) / .decompress(binaries, headers)          # :67-77 / :90-112 (rANS streams, csrc/rans.cpp)
    .Codebooks / .NormalizedFreq / .CDFs / .CodeUsage / .QuantizationParameter

The module tree and every state_dict key are the reference's (718 entries for the qp=2 shape), so a
reference checkpoint's `model` dict loads with `load_state_dict(strict=True)`.
"""
from __future__ import annotations

import operator
from typing import List, Tuple

import torch
import torch.nn.functional as F
from torch import nn

from ..nn import AttentionBlock, ResidualBlock, ResidualBlockShuffle, ResidualBlockWithStride, conv3x3, pixelShuffle3x3
from ..utils.specification import FileHeader, ImageSize
from .quantizer import BaseQuantizer, ResidualBackwardQuantizer, UMGMQuantizer

from ..utils.specification import VERSION as __version__   # the reference snapshot's mcquic.__version__ (FileHeader)


_VERSION_OF = operator.attrgetter("_version")
_DATA_PTR_OF = operator.methodcaller("data_ptr")


def _forget_captures_hook(module, incompatible_keys):
    """load_state_dict post-hook of BaseCompressor: new weights, so captured hipGraphs (which replay packed copies) are stale."""
    module._forgetCaptures()


class _GraphedCall:
    """One captured hipGraph of `fn` for fixed input shapes: replay costs one launch instead of ~165 Python-side
    kernel launches (at batch 1 the eager path is host-bound: ~25 us of Python per launch against ~10 us kernels).
    Inputs are copied into the graph's static buffers, outputs are cloned out of them.  `owns`: device buffers the captured
    launches read besides the model's own -- they live exactly as long as this capture; `token`: what they were made under."""

    def __init__(self, fn, inputs, owns=None, token=None):
        self.owns, self.token = owns, token
        self.static_in = [t.clone() for t in inputs]
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):                      # warm-up off the capture: weight packing, allocator pools
            for _ in range(2):
                fn(*self.static_in)
        cur.wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.static_out = fn(*self.static_in)

    def __call__(self, inputs):
        for dst, src in zip(self.static_in, inputs):
            dst.copy_(src)
        self.graph.replay()
        out = self.static_out
        return [t.clone() for t in out] if isinstance(out, (list, tuple)) else out.clone()


class AlignedPadding(nn.Module):
    """Reflect-pad H, W up to multiples of `base` (reference: mcquic/data/transforms.py:81-99).
    A no-op for 768x512.  Data movement only (torch's reflect pad on the device)."""

    def __init__(self, base: int = 128):
        super().__init__()
        self._base = base

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        h, w = x.shape[-2], x.shape[-1]
        wPadding = ((w // self._base + 1) * self._base - w) % self._base
        hPadding = ((h // self._base + 1) * self._base - h) % self._base
        if wPadding == 0 and hPadding == 0:
            return x
        padLeft = wPadding // 2
        padTop = hPadding // 2
        return F.pad(x, (padLeft, wPadding - padLeft, padTop, hPadding - padTop), "reflect")


class BaseCompressor(nn.Module):
    def __init__(self, encoder: nn.Module, quantizer: BaseQuantizer, decoder: nn.Module):
        super().__init__()
        self._encoder = encoder
        self._decoder = decoder
        self._quantizer = quantizer
        self._qp = "-1"
        self._padding = AlignedPadding()
        self._graphs = None          # {(kind, shapes, device): _GraphedCall} once enableGraphs(True)
        self._graphStamp = None      # fingerprint of the weights the captures were taken under
        self.register_load_state_dict_post_hook(_forget_captures_hook)      # (module-level function: a lambda here made the model unpicklable)

    def enableGraphs(self, enabled: bool = True):
        """Replay `encode` / `decode` as captured hipGraphs (one per input shape).  For latency-bound small batches.
        A capture bakes in the addresses of the packed weights / codebooks it ran on, so every captured call first
        compares a fingerprint of all parameters and buffers (version counters + storage addresses, ~0.15 ms) with the one
        the captures were taken under: an optimizer step, `load_state_dict`, `reAssignCodebook`, `.to(...)`, `p.data = ...`
        or any other in-place update drops all captures before anything is replayed.  Two things the fingerprint cannot
        see: `p.data.copy_(...)` (no version bump, same address) and a Parameter OBJECT swapped for another one
        (`module.weight = nn.Parameter(...)`): call `enableGraphs()` again after either."""
        self._graphs = {} if enabled else None
        self._graphStamp = None
        return self

    def _weightStamp(self):
        from .. import ops
        tensors = self.__dict__.get("_stampTensors")
        if tensors is None:                      # (walking the module tree costs ~3 ms: done once, redone after _apply)
            tensors = self.__dict__["_stampTensors"] = list(self.parameters()) + list(self.buffers())
        ptrs = tuple(map(_DATA_PTR_OF, tensors))   # `p.data = other` / set_() move the storage without touching the counter
        try:
            return tuple(map(_VERSION_OF, tensors)), ptrs
        except RuntimeError:                     # tensors created under torch.inference_mode() carry no counter
            return tuple(ops.tensor_version(t) for t in tensors), ptrs

    def _forgetCaptures(self):
        self.__dict__.pop("_stampTensors", None)
        if self._graphs is not None:
            self._graphs.clear()

    def _apply(self, fn, *args, **kwargs):
        """`.to()` / `.cuda()` / `.float()` replace storages (and buffer objects): forget the captures and the tensor list."""
        self._forgetCaptures()
        return super()._apply(fn, *args, **kwargs)

    def _dropStaleCaptures(self):
        from .. import ops
        stamp = (self._weightStamp(), ops.winograd_enabled())     # (the opt-in switch re-packs every convolution: as good as new weights)
        if stamp != self._graphStamp:            # weights changed since the captures: their packed operands are stale
            self._graphs.clear()
            self._graphStamp = stamp

    RATE_CAPTURES = 8                # penalised-encode captures kept at a time (least recently used goes first, with its packs)

    def _graphed(self, kind: str, fn, inputs, variant: tuple = (), token=None, make=None):
        """`variant`: what else the capture bakes in besides the weights -- the lambdas of a rate-constrained encode -- so that a
        capture taken under one lambda never serves another, or the plain path.  Such a capture launches on penalised packs that are
        no part of the model: `make()` -> (fn, packs) builds them on a miss only, the capture OWNS them (`_GraphedCall.owns`: they
        cannot be freed or rewritten under it), and `token` -- the codebooks' and tables' stamp they were made under -- is compared
        on every call: a capture whose token is stale is dropped, never replayed.  At most RATE_CAPTURES of them are kept."""
        self._dropStaleCaptures()
        key = (kind, tuple(tuple(t.shape) for t in inputs), inputs[0].device) + tuple(variant)
        g = self._graphs.get(key)
        if make is None:
            if g is None:
                g = self._graphs[key] = _GraphedCall(fn, inputs)
            return g(inputs)
        if g is not None:
            del self._graphs[key]                # (re-inserted below: the dict's order is the order of last use)
            if g.token != token:
                g = None
        if g is None:
            owned = [k for k, c in self._graphs.items() if c.owns is not None]
            for k in owned[:max(0, len(owned) - (self.RATE_CAPTURES - 1))]:
                del self._graphs[k]
            fn, packs = make()
            g = _GraphedCall(fn, inputs, owns=packs, token=token)
        self._graphs[key] = g
        return g(inputs)

    @property
    def QuantizationParameter(self) -> str:
        return self._qp

    @QuantizationParameter.setter
    def QuantizationParameter(self, qp: str):
        self._qp = qp

    def forward(self, x: torch.Tensor, uniforms=None):
        """Training-mode forward (compressor.py:35-43): (xHat, yHat, codes, logits); None in eval mode like the
        reference.  With grad enabled the step runs through mcquic_amd.autograd (HIP kernels in both directions:
        xHat.backward(...) fills every parameter's .grad); under torch.no_grad() the fused inference kernels are used.
        `uniforms`: optional per-level (u_drop, u_gumbel) draws replacing the two `torch.rand_like(logit)` calls.
        The returned `logits` carry their graph like the reference's (autograd.SoftQuantizeFn: a gradient on them reaches
        latents, codebooks and temperatures; the shipped losses, mcquic/loss/__init__.py:47-62, never produce one)."""
        if not self.training:
            return None
        self._check(x)
        if torch.is_grad_enabled():
            self._repackStale()
            y = self._trainEncode(x)
            yHat, codes, logits = self._quantizer(y, uniforms)
            return self._decoder(yHat), yHat, codes, logits
        y = self._encode_latent(x, pad=False)
        yHat, codes, logits = self._quantizer(y, uniforms)
        xHat = self._decoder(yHat)
        return xHat, yHat, codes, logits

    def _trainEncode(self, x: torch.Tensor) -> torch.Tensor:
        """`self._encoder(x)` in the training graph -- no padding there (compressor.py:39); the stem conv also stores silu(.)
        for the block that follows (every encoder here continues with an activation)."""
        y = self._encoder[0](x, dual_silu=True)
        for i in range(1, len(self._encoder)):
            y = self._encoder[i](y)
        return y

    def _repackStale(self):
        """After an optimizer step every convolution's operand streams are stale: refresh them in grouped launches
        (nn.convs.Conv2d.repack_stale) before the step instead of one by one inside it."""
        convs = self.__dict__.get("_convList")
        if convs is None:
            from ..nn.convs import Conv2d
            convs = self.__dict__["_convList"] = [m for m in self.modules() if isinstance(m, Conv2d)]
        from ..nn.convs import Conv2d
        Conv2d.repack_stale(convs, self.__dict__.get("_packMasks"))     # (_packMasks: only while parallel.GraphedTrainStep captures)
        gdns = self.__dict__.get("_gdnList")
        if gdns is None:
            from ..nn.gdn import GenDivNorm
            gdns = self.__dict__["_gdnList"] = [m for m in self.modules() if isinstance(m, GenDivNorm)]
        if gdns:
            from .. import autograd as AG
            AG.refresh_gdn_operands(gdns)                               # the GDN layers' folded parameters and operand streams, grouped too

    def reAssignCodebook(self) -> torch.Tensor:
        return self._quantizer.reAssignCodebook()

    def syncCodebook(self):
        return self._quantizer.syncCodebook()

    @property
    def Codebooks(self):
        return self._quantizer.Codebooks

    @property
    def CDFs(self):
        return self._quantizer.CDFs

    @property
    def NormalizedFreq(self):
        return self._quantizer.NormalizedFreq

    def deviceCDFs(self, normalize: bool = False) -> List[torch.Tensor]:
        """The entropy coder's tables as uint32 tensors on the device (`EntropyCoder.deviceCDFs`)."""
        return self._quantizer._entropyCoder.deviceCDFs(normalize)

    def codeBits(self, codes: List[torch.Tensor], **kwargs) -> torch.Tensor:
        """double [n, levels]: what the coder's tables charge for `codes`, computed on the device (`EntropyCoder.codeBits`)."""
        return self._quantizer._entropyCoder.codeBits(codes, **kwargs)

    @property
    def CodeUsage(self):
        return torch.cat(list((freq > 1e-6).flatten() for freq in self._quantizer.NormalizedFreq)).float().mean()

    def _check(self, x: torch.Tensor):
        if x.dim() != 4 or x.shape[1] != 3:
            raise RuntimeError(f"expected an image batch [n, 3, h, w], got {tuple(x.shape)}")

    def _encode_latent(self, x: torch.Tensor, pad: bool = True) -> torch.Tensor:
        """`self._encoder(self._padding(x))`; the stem conv also emits silu(.) for the first ResidualBlock."""
        y = self._encoder[0](self._padding(x) if pad else x, dual_silu=True)
        for i in range(1, len(self._encoder)):
            y = self._encoder[i](y)
        return y

    AQ_CLIP = 2.0                    # the clip of a bare `aq` strength: w in [1/4, 4]

    def _aqArgs(self, aq):
        """`aq` of encode / compress / encode_to_rate checked before any device work: None, or (strength, clip) as the float32 values
        the kernel takes -- a bare float means clip = AQ_CLIP.  ValueError unless strength is finite and >= 0 and clip finite and > 0."""
        if aq is None:
            return None
        from .. import ops
        pair = tuple(aq) if isinstance(aq, (list, tuple)) else (aq, self.AQ_CLIP)
        try:
            if len(pair) != 2 or any(isinstance(v, bool) or torch.is_tensor(v) and v.dim() > 0 for v in pair):
                raise TypeError
            strength, clip = ops.lambda_f32(pair[0]), ops.lambda_f32(pair[1])
        except (TypeError, ValueError):
            raise ValueError(f"aq: a strength >= 0, or (strength, clip) with clip > 0, finite float32 values; got {aq!r}") from None
        if not (clip > 0.0):
            raise ValueError(f"aq: clip must be > 0, got {aq!r}")
        return strength, clip

    def _aqMap(self, x: torch.Tensor, aq: tuple, rd_map=None) -> torch.Tensor:
        """The effective map float32 [n, h0, w0] of a call with `aq` = (strength, clip) (checked): w, or w * rd_map -- two eager launches
        (`ops.activity_cells`, `ops.activity_weights`) in front of the encoder, nothing read on the host.  The activity error word of
        the call is kept for `activityError()`."""
        from .. import ops
        a, mask, self.__dict__["_aqErr"] = ops.activity_cells(x, self._padding._base)
        return ops.activity_weights(a, mask, aq[0], aq[1], roi=rd_map)

    def activityWeights(self, x: torch.Tensor, aq) -> torch.Tensor:
        """The adaptive-quantisation map of `x` alone: float32 [n, h0, w0] on the level-0 code grid, what `encode(x, aq=aq)` multiplies
        lambda by.  Per 16 x 16 cell of the aligned image a = log2(variance of the luma + 2^-14), the variance centred (two passes);
        w = 2^clamp(strength (a - mean a), -clip, +clip): above 1 (fewer bits) where texture masks the error, below 1 where the picture
        is flat, geometric mean 1 over an image while nothing clips.  `aq`: a strength >= 0, or (strength, clip); a bare strength takes
        clip = 2 (w in [1/4, 4]) -- a design choice that nothing here could tune: there is no trained checkpoint to tune it on."""
        aq = self._aqArgs(aq)
        if aq is None:
            raise ValueError("activityWeights: `aq` must be a strength or (strength, clip)")
        self._quantizer.rateLambdas(1.0)                     # (a quantizer without tables refuses here)
        self._check(x)
        if x.shape[0] == 0:
            raise ValueError("aq: an empty batch has no map")
        with torch.no_grad():
            return self._aqMap(x, aq)

    def activityError(self) -> torch.Tensor:
        """int32 [n] on the device, from the last call with `aq`: 1 where an image held a cell with a non-finite luma (that cell took
        w = 1).  Nothing is read on the host."""
        err = self.__dict__.get("_aqErr")
        if err is None:
            raise RuntimeError("activityError: no call with `aq` has run yet")
        return err

    def encode(self, x: torch.Tensor, rd_lambda=None, rd_map=None, aq=None) -> List[torch.Tensor]:
        """`rd_lambda`: None = nearest codeword; a float >= 0 (or one per level) = the entropy-constrained assignment
        argmin_k (distance + lambda * bits_k) under the coder's current tables (`UMGMQuantizer.encode`): one model, a continuous
        rate knob; `decode` / `decompress` and the stream format do not know about it.  Inside a caller's own stream capture
        (where plain `encode` works as it is) nothing can be built or read back: the packs of these lambdas must have been made by
        a call outside the capture under the current codebooks and tables, else RuntimeError -- and the caller keeps them alive
        with its graph (`packs = model._quantizer.ratePacks(model._quantizer.rateLambdas(lam))`).
        `rd_map`: rate control per image ([n]) or per level-0 code cell ([n, H / 16, W / 16] of the 128-aligned image), a float32
        device tensor; `rd_lambda` is then the per-level scale (`UMGMQuantizer.encode`).  The map is an operand: under `enableGraphs`
        one capture per image shape and map form serves every map and every scale; inside a caller's capture it works once a call
        outside it has made the tables' bits sections.
        `aq`: adaptive quantisation, None (off) or a strength >= 0 or (strength, clip) (`activityWeights`): the map w made from the image
        on the device becomes the effective map, w * rd_map with a map given, w alone without; `rd_lambda` stays the per-level scale.
        The two launches that make it run eagerly in front of the `rd_map` path, whose capture it shares (the key is the map's shape)."""
        aq = self._aqArgs(aq)
        lams, empty = self._rateArgs(x, rd_lambda, rd_map, aq)
        if empty:
            # an empty shard (fewer images than ranks, parallel.shard_range): PyTorch's layers hand back empty tensors of the
            # right geometry (the reference's behaviour); the kernels refuse empty launches, so the geometry comes from one blank image
            return [c[:0] for c in self.encode(x.new_zeros((1,) + tuple(x.shape[1:])), rd_lambda=lams)]
        if aq is not None:
            with torch.no_grad():
                rd_map = self._aqMap(x, aq, rd_map)
        if rd_map is not None:
            return self._encodeRateMap(x, lams, rd_map)
        if lams is not None:
            return self._encodeRate(x, lams)
        with torch.no_grad():
            if self._replays(x):
                return self._graphed("encode", lambda t: self._quantizer.encode(self._encode_latent(t)), [x.contiguous()])
            return self._quantizer.encode(self._encode_latent(x))

    def _rateArgs(self, x: torch.Tensor, rd_lambda, rd_map, aq=None):
        """The arguments of `encode` / `compress` checked, in this order, before any device work: `rd_lambda` (`rateLambdas`: quantizers
        without tables refuse first), the image batch, the map against its level-0 code grid.  Returns (lams, empty): lams = None for
        the plain path, the lambdas of the scalar knob, or with a map the per-level scales (None = 1); empty: a batch of no images (with
        a map that raises: it has no batch to belong to).  `aq` (already checked, `_aqArgs`) makes a map, so it counts as one."""
        lams = None
        if rd_lambda is not None or rd_map is not None or aq is not None:
            lams = self._quantizer.rateLambdas(1.0 if rd_lambda is None else rd_lambda)
        self._check(x)
        if rd_map is not None:
            self._quantizer.checkRateMap(rd_map, *self._rateGrid(x), x.device)
        if x.shape[0] == 0 and rd_map is not None:
            raise ValueError("rd_map: an empty batch has no map")
        if aq is not None:
            from .. import ops
            if x.shape[0] == 0:
                raise ValueError("aq: an empty batch has no map")
            ops.activity_grid(x.shape[-2], x.shape[-1], self._padding._base)      # (padding that reflect cannot make: refused here)
        return lams, x.shape[0] == 0

    def _replays(self, t: torch.Tensor) -> bool:
        """A call on `t` replays through the captures of `enableGraphs` (not inside a caller's own capture: that one records us eagerly)."""
        return self._graphs is not None and t.is_cuda and not torch.cuda.is_current_stream_capturing()

    def decode(self, codes: List[torch.Tensor]) -> torch.Tensor:
        if codes[0].shape[0] == 0:                            # (empty shard, see encode)
            return self.decode([c.new_zeros((1,) + tuple(c.shape[1:])) for c in codes])[:0]
        with torch.no_grad():
            if self._replays(codes[0]):
                return self._graphed("decode", lambda *c: self._decoder(self._quantizer.decode(list(c))), [c.contiguous() for c in codes])
            return self._decoder(self._quantizer.decode(codes))

    def _encodeRate(self, x: torch.Tensor, lams: tuple) -> List[torch.Tensor]:
        """`encode` with the penalised packs of `lams` (already checked).  Under `enableGraphs` the packs are made BEFORE the capture
        and the capture keeps them (`_graphed`): its key names the lambdas, its token the codebooks and tables they were made from,
        so a replay never reads a buffer that was freed, rewritten or made for other tables.  A lambda never seen before costs a
        capture; the least recently used go beyond `RATE_CAPTURES`."""
        with torch.no_grad():
            def make():
                packs = self._quantizer.ratePacks(lams)
                return (lambda t: self._quantizer.encode(self._encode_latent(t), packs=packs)), packs
            if self._replays(x):
                return self._graphed("encode", None, [x.contiguous()], (lams,), token=self._quantizer.rateState(), make=make)
            return make()[0](x)

    def _rateGrid(self, x: torch.Tensor):
        """(n, h0, w0): the level-0 code grid of the image batch `x` -- the aligned image halved four times."""
        base = self._padding._base
        h, w = -(-int(x.shape[-2]) // base) * base, -(-int(x.shape[-1]) // base) * base
        for _ in range(4):
            h, w = (h + 1) // 2, (w + 1) // 2
        return int(x.shape[0]), h, w

    def _encodeRateMap(self, x: torch.Tensor, scales: tuple, rd_map: torch.Tensor) -> List[torch.Tensor]:
        """`encode` with `rd_map` (scales already checked).  Under `enableGraphs` the map and the scales are INPUTS of the capture: its
        key names the image shape and the map's shape, not their values, and it holds no lambda-dependent buffer -- only the tables'
        bits sections, which it keeps, and whose stamp is compared on every call (a capture under older tables is taken again)."""
        with torch.no_grad():
            if not self._replays(x):
                return self._quantizer.encode(self._encode_latent(x), rd_lambda=scales, rd_map=rd_map)
            self._dropStaleCaptures()
            inputs = [x.contiguous(), rd_map.contiguous()]
            key = ("encode", tuple(tuple(t.shape) for t in inputs), x.device, "rd_map")
            token = self._quantizer._entropyCoder.deviceCDFStamp()
            g = self._graphs.get(key)
            if g is None or g.token != token:
                bits = self._quantizer.rateBitsPacks()
                ones = (1.0,) * len(scales)          # (the kernel reads the scales from the capture's third input)
                pinned = torch.tensor(scales, dtype=torch.float32).pin_memory()
                g = self._graphs[key] = _GraphedCall(lambda t, mp, sc: self._quantizer.encode(self._encode_latent(t), rd_lambda=ones, rd_map=mp,
                                                                                          scales_dev=sc), inputs + [pinned.to(x.device)], token=token)
                # what the captured launches read and write besides the inputs lives as long as the capture: the tables' bits sections,
                # and the error word of the captured call (allocated inside the capture, so in the graph's own pool)
                g.bits, g.error = bits, self._quantizer.rateMapError()
                g.scales, g.pinned = scales, pinned
            elif g.scales != scales:                 # new scales go into the static input from a pinned buffer, and only when they change
                g.pinned.copy_(torch.tensor(scales, dtype=torch.float32))
                g.static_in[2].copy_(g.pinned)
                g.scales = scales
            codes = g(inputs)                        # (zip stops at the two inputs given: the scales are already in place)
            self._quantizer.__dict__["_rateMapErr"] = g.error      # the capture's own word, just rewritten by THIS replay (nothing allocated)
            return codes

    def rateMapError(self) -> torch.Tensor:
        """int32 [n] on the device, from the last `encode` / `compress` / `encode_to_rate` call with a map, replays under `enableGraphs`
        included: 1 where an image's map held a negative, NaN or infinite value (which counted as 0).  Nothing is read on the host."""
        return self._quantizer.rateMapError()

    def encode_to_rate(self, x: torch.Tensor, target_bpp, iters: int = 12, lambda_max: float = 64.0, per_image: bool = False,
                       trace: bool = False, aq=None, rd_map=None):
        """Codes of `x` that the coder's tables charge at most `target_bpp` bits per pixel for, by a search over ONE lambda for the
        whole batch: returns (codes, lam, bpp) with bpp = codeBits(codes).sum() / (n h w) <= target_bpp.  The image-side encoder runs
        once; each of the at most `iters` + 2 trials re-runs the quantizer cascade only and reads one number back (so the search runs
        outside any capture, eagerly).  lambda = 0 is tried first: if the plain codes already meet the target they are returned with
        lam = 0.  Then `lambda_max`: if even that misses, ValueError names the bpp it reached.  Then the bracket (0, lambda_max] is
        narrowed `iters` times -- a sixteenth of the upper end while the lower end is still 0 (the useful lambdas span decades and
        depend on the latents' scale), the geometric mean after -- and the smallest lambda visited that met the target is returned.
        Rate is not strictly monotone in lambda below level 0 (a level's residual depends on the level above), hence "visited".
        `aq`, `rd_map`: the search runs over a spatial map -- `aq` as for `encode` (the map w made from the image, once), `rd_map` the
        caller's own ([n] or [n, h0, w0]); the effective map is w * rd_map (w = 1 without `aq`).  The batch form then tries
        `encode(x, rd_lambda=lambda, rd_map=w * rd_map)` and what it returns reproduces through `encode(x, rd_lambda=lam, aq=aq,
        rd_map=rd_map)`; the per-image form makes every trial's map (w * rd_map) * lam[n] with one `ops.activity_weights` launch, `lam`
        the multiplier the search is over, and still reads nothing on the host.  With neither, the code path is the one without maps."""
        from .. import ops
        aq = self._aqArgs(aq)
        self._quantizer.rateLambdas(0.0)                     # (a quantizer without tables refuses here)
        self._check(x)
        cells = None
        if aq is not None or rd_map is not None:
            if rd_map is not None:
                self._quantizer.checkRateMap(rd_map, *self._rateGrid(x), x.device)
            if x.shape[0] == 0:
                raise ValueError("encode_to_rate: an empty batch has no rate")
            ops.activity_grid(x.shape[-2], x.shape[-1], self._padding._base)
            cells = (0.0, self.AQ_CLIP) if aq is None else aq          # (a map without `aq`: strength 0, w = 1)
        if per_image:
            return self._encodeToRatePerImage(x, target_bpp, int(iters), lambda_max, bool(trace), cells, rd_map)
        target, iters = float(target_bpp), int(iters)
        lambda_max = ops.lambda_f32(lambda_max)
        if not (target > 0.0) or not (lambda_max > 0.0) or iters < 0:
            raise ValueError(f"encode_to_rate: target_bpp and lambda_max must be positive and finite, iters >= 0 "
                             f"(got {target_bpp}, {lambda_max}, {iters})")
        if x.shape[0] == 0:
            raise ValueError("encode_to_rate: an empty batch has no rate")
        if x.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("encode_to_rate reads the rate back every trial: it cannot be captured")
        pixels = float(x.shape[0] * x.shape[-2] * x.shape[-1])
        with torch.no_grad():
            wmap = None if cells is None else self._aqMap(x, cells, rd_map)
            y = self._encode_latent(x)

            def trial(lam: float):
                if wmap is not None:
                    codes = self._quantizer.encode(y, rd_lambda=lam, rd_map=wmap)
                else:
                    codes = self._quantizer.encode(y) if lam == 0.0 else self._quantizer.encode(y, rd_lambda=lam)
                return codes, float(self.codeBits(codes).sum()) / pixels

            codes, bpp = trial(0.0)
            if bpp <= target:
                return codes, 0.0, bpp
            best = trial(lambda_max)
            if best[1] > target:
                raise ValueError(f"encode_to_rate: lambda_max = {lambda_max} reaches {best[1]:.6f} bpp, above the target {target}")
            lo, hi = 0.0, lambda_max
            for _ in range(iters):
                mid = ops.lambda_f32(hi / 16.0 if lo == 0.0 else (lo * hi) ** 0.5)      # (the float32 the kernel takes: what is returned is what ran)
                if not (lo < mid < hi):
                    break
                got = trial(mid)
                if got[1] <= target:
                    hi, best = mid, got
                else:
                    lo = mid
        return best[0], hi, best[1]

    def _encodeToRatePerImage(self, x: torch.Tensor, target_bpp, iters: int, lambda_max, trace: bool, aq=None, roi=None):
        """`encode_to_rate(per_image=True)`: every image is brought to ITS target by its own lambda, the search's state on the device.
        `target_bpp`: a float, or a device tensor [n].  The image-side encoder runs once; then `iters` + 2 lockstep trials of the
        quantizer cascade with rd_map = lambda[n], each followed by `codeBits` and one `ops.rate_search_step` launch; then the final
        cascade at the chosen lambdas.  Per image the rule is the batch search's: 0 first (met: done), `lambda_max` (missed: the image
        ends there), else the bracket -- a sixteenth of the upper end while the lower is 0, the geometric mean after, frozen when the
        float32 midpoint leaves the open bracket -- and the answer is the upper end.  Finished images ride along at their answer.
        Nothing is read on the host: with the bits sections made beforehand (any `encode(x, rd_map=...)` outside) the whole call
        captures into a caller's graph.  Returns (codes, lam float32 [n], bpp float64 [n]) on the device, bpp = the final run's
        codeBits summed over the levels / (H W); an unreachable target does not raise: the image ends at `lambda_max` and its bpp
        shows it.  `trace`: also (lams float32, bpps float64) [trials, n], what every trial ran at and reached.
        `aq` = (strength, clip) (checked), `roi`: the spatial form -- the cell activities are made once, every trial's map
        (w * roi) * lam[n] by one `ops.activity_weights` launch into one buffer, and the cascade runs with that map; the search's state,
        its step and the return values are the same, `lam` now the per-image multiplier of the map."""
        from .. import ops
        lambda_max = ops.lambda_f32(lambda_max)
        if not (lambda_max > 0.0) or iters < 0:
            raise ValueError(f"encode_to_rate: lambda_max must be positive and finite, iters >= 0 (got {lambda_max}, {iters})")
        n = int(x.shape[0])
        if n == 0:
            raise ValueError("encode_to_rate: an empty batch has no rate")
        if torch.is_tensor(target_bpp) and target_bpp.dim() > 0:
            if tuple(target_bpp.shape) != (n,) or target_bpp.device != x.device or not target_bpp.dtype.is_floating_point:
                raise ValueError(f"encode_to_rate: a target tensor must be floating point [{n}] on {x.device}, got "
                                 f"{target_bpp.dtype} {tuple(target_bpp.shape)} on {target_bpp.device}")
            target = None
        else:
            target = float(target_bpp)
            if not (target > 0.0) or target == float("inf"):
                raise ValueError(f"encode_to_rate: target_bpp must be positive and finite (got {target_bpp})")
        if not x.is_cuda:
            raise RuntimeError(f"mcquic_amd: encode_to_rate(per_image=True) runs on a HIP device only (input on {x.device})")
        dev, trials = x.device, iters + 2
        pixels = float(x.shape[-2] * x.shape[-1])
        with torch.no_grad():
            tgt = target_bpp.to(torch.float64).contiguous() if target is None else torch.full((n,), target, dtype=torch.float64, device=dev)
            lam = torch.zeros(n, dtype=torch.float32, device=dev)
            bracket = torch.empty((n, 2), dtype=torch.float32, device=dev)
            done = torch.empty(n, dtype=torch.int32, device=dev)
            tlam = torch.empty((trials + 1, n), dtype=torch.float32, device=dev)
            tbpp = torch.empty((trials + 1, n), dtype=torch.float64, device=dev)
            if aq is not None:
                a, mask, self.__dict__["_aqErr"] = ops.activity_cells(x, self._padding._base)
                trial_map = torch.empty_like(a)
            y = self._encode_latent(x)
            for t in range(trials + 1):                       # (the last one is the final run: recorded, nothing decided)
                if aq is None:
                    codes = self._quantizer.encode(y, rd_map=lam)
                else:
                    codes = self._quantizer.encode(y, rd_map=ops.activity_weights(a, mask, aq[0], aq[1], roi=roi, lam=lam, out=trial_map))
                ops.rate_search_step(self.codeBits(codes), tgt, lam, bracket, done, tlam, tbpp, pixels, lambda_max, t, trials)
        out = (codes, lam, tbpp[trials].clone())
        return out + (tlam[:trials], tbpp[:trials]) if trace else out

    def compress(self, x: torch.Tensor, coder: str = "host", rd_lambda=None, rd_map=None,
                 lanes=None, aq=None) -> Tuple[List[torch.Tensor], List[List[bytes]], List[FileHeader]]:
        """`coder`: "host" (the default) codes the streams with csrc/rans.cpp on host threads, "device" with csrc/rans_dev.hip where
        the codes are (`EntropyCoder.compressDevice`); the bytes and headers are the same.  `rd_lambda`, `rd_map`, `aq`: as for `encode`.
        `lanes`: None (the default) for the reference's streams; "auto" or a power of two <= 64 for the lane-interleaved layout
        (DESIGN.md section 3), whose streams `decompress(..., lanes=True)` reads -- the same bytes under either coder."""
        self._quantizer._checkCoder(coder)
        layout = self._quantizer._checkLanes(lanes)
        aq = self._aqArgs(aq)
        lams, empty = self._rateArgs(x, rd_lambda, rd_map, aq)
        if empty:                                             # (empty shard: no streams, no headers)
            return self.encode(x), [], []
        n, c, h, w = x.shape
        with torch.no_grad():
            if aq is not None:
                rd_map = self._aqMap(x, aq, rd_map)
            codes, binaries, codeSizes = self._quantizer.compress(self._encode_latent(x), coder, rd_lambda=lams, rd_map=rd_map, **layout)
        header = [FileHeader(__version__, self._qp, codeSize, ImageSize(height=h, width=w, channel=c)) for codeSize in codeSizes]
        return codes, binaries, header

    def _checkHeaderGeometry(self, headers: List[FileHeader]):
        """Untrusted `.mcq` headers: the code sizes must be the ones THIS image size produces (level 0 = the 128-aligned
        image at 1/16 resolution), before the coder allocates anything from them."""
        for header in headers:
            size, code = header.ImageSize, header.CodeSize
            if not (0 < int(size.height) <= (1 << 20) and 0 < int(size.width) <= (1 << 20)):
                raise RuntimeError("The header's image size is out of range.")
            base = self._padding._base
            ph, pw = -(-int(size.height) // base) * base, -(-int(size.width) // base) * base
            if len(code.heights) < 1 or int(code.heights[0]) * 16 != ph or int(code.widths[0]) * 16 != pw:
                raise RuntimeError(f"The header's code size {list(code.heights)} x {list(code.widths)} does not belong to a "
                                   f"{size.height} x {size.width} image.")

    def decompress(self, binaries: List[List[bytes]], headers: List[FileHeader], coder: str = "host", lanes: bool = False) -> torch.Tensor:
        """`coder`: "host" (the default) or "device" (`EntropyCoder.decompressDevice`), as for `compress`; the same image either way.
        `lanes`: True for the streams of `compress(..., lanes=...)`; streams of the other layout raise."""
        self._quantizer._checkCoder(coder)
        layout = self._quantizer._checkLanes(lanes)
        if type(self)._encode_latent is BaseCompressor._encode_latent:       # (Compressor's 16x stem; Neon's geometry differs)
            self._checkHeaderGeometry(headers)
        with torch.no_grad():
            restored = self._decoder(self._quantizer.decompress(binaries, [header.CodeSize for header in headers], coder, **layout))
        imageSize = headers[0].ImageSize
        H, W = restored.shape[-2], restored.shape[-1]
        h, w = imageSize.height, imageSize.width
        cropTop, cropLeft = (H - h) // 2, (W - w) // 2
        return restored[..., cropTop:cropTop + h, cropLeft:cropLeft + w]


class Compressor(BaseCompressor):
    def __init__(self, channel: int, m: int, k: List[int], permutationRate: float = 0.0):
        encoder = nn.Sequential(
            conv3x3(3, channel, 2),
            ResidualBlock(channel, channel),
            ResidualBlockWithStride(channel, channel),
            AttentionBlock(channel),
            ResidualBlock(channel, channel),
            ResidualBlockWithStride(channel, channel),
            ResidualBlock(channel, channel))
        decoder = nn.Sequential(
            ResidualBlock(channel, channel),
            ResidualBlockShuffle(channel, channel),
            AttentionBlock(channel),
            ResidualBlock(channel, channel),
            ResidualBlockShuffle(channel, channel),
            ResidualBlock(channel, channel),
            pixelShuffle3x3(channel, 3, 2))
        quantizer = UMGMQuantizer(channel, m, k, permutationRate, {
            "latentStageEncoder": lambda: nn.Sequential(
                ResidualBlockWithStride(channel, channel), ResidualBlock(channel, channel), AttentionBlock(channel)),
            "quantizationHead": lambda: nn.Sequential(
                ResidualBlock(channel, channel), AttentionBlock(channel), conv3x3(channel, channel)),
            "latentHead": lambda: nn.Sequential(
                ResidualBlock(channel, channel), AttentionBlock(channel), conv3x3(channel, channel)),
            "restoreHead": lambda: nn.Sequential(
                AttentionBlock(channel), ResidualBlock(channel, channel), ResidualBlockShuffle(channel, channel)),
            "dequantizationHead": lambda: nn.Sequential(
                AttentionBlock(channel), conv3x3(channel, channel), ResidualBlock(channel, channel)),
            "sideHead": lambda: nn.Sequential(
                AttentionBlock(channel), conv3x3(channel, channel), ResidualBlock(channel, channel)),
        })
        super().__init__(encoder, quantizer, decoder)



class Neon(BaseCompressor):
    """The stage-1 model of the reference's generative branch (mcquic/modules/compressor.py:181-241; what the snapshot's
    trainer builds, mcquic/train/ddp.py:79-83): a 3x-strided encoder / decoder around a `ResidualBackwardQuantizer`.
    Same constructor, module tree and state_dict keys; `checkpoint_wrapper` (fairscale activation checkpointing, a
    training-memory measure) is not applied.  `groups` / `denseNorm`: see nn/blocks.py (GroupNorm on csrc/norm.hip)."""

    def __init__(self, channel: int, k: int, size: List[int], denseNorm: bool = False, *_, **__):
        quantizer = ResidualBackwardQuantizer(k, size, denseNorm)
        q = quantizer.channel
        encoder = nn.Sequential(
            conv3x3(3, channel),
            AttentionBlock(channel, 32, denseNorm),
            ResidualBlock(channel, channel, 32, denseNorm),
            ResidualBlock(channel, channel, 32, denseNorm),
            ResidualBlockWithStride(channel, channel, 2, 32, denseNorm),
            ResidualBlock(channel, channel, 32, denseNorm),
            ResidualBlockWithStride(channel, channel, 2, 32, denseNorm),
            ResidualBlock(channel, channel, 32, denseNorm),
            ResidualBlockWithStride(channel, channel, 2, 32, denseNorm),
            AttentionBlock(channel, 32, denseNorm),
            ResidualBlock(channel, 2 * channel, 32, denseNorm),
            ResidualBlock(2 * channel, 2 * channel, 32, denseNorm),
            ResidualBlock(2 * channel, 2 * channel, 32, denseNorm),
            ResidualBlock(2 * channel, 2 * channel, 32, denseNorm),
            ResidualBlock(2 * channel, q, 1, denseNorm),
            AttentionBlock(q, 1, denseNorm))
        decoder = nn.Sequential(
            AttentionBlock(q, 1, denseNorm),
            ResidualBlock(q, 2 * channel, 1, denseNorm),
            ResidualBlock(2 * channel, 2 * channel, 32, denseNorm),
            ResidualBlock(2 * channel, 2 * channel, 32, denseNorm),
            ResidualBlock(2 * channel, 2 * channel, 32, denseNorm),
            ResidualBlock(2 * channel, channel, 32, denseNorm),
            AttentionBlock(channel, 32, denseNorm),
            ResidualBlock(channel, channel, 32, denseNorm),
            ResidualBlockShuffle(channel, channel, 2, 32, denseNorm),
            ResidualBlock(channel, channel, 32, denseNorm),
            ResidualBlockShuffle(channel, channel, 2, 32, denseNorm),
            ResidualBlock(channel, channel, 32, denseNorm),
            ResidualBlockShuffle(channel, channel, 2, 32, denseNorm),
            ResidualBlock(channel, channel, 32, denseNorm),
            ResidualBlock(channel, channel, 32, denseNorm),
            AttentionBlock(channel, 32, denseNorm),
            conv3x3(channel, 3))
        super().__init__(encoder, quantizer, decoder)

    def _encode_latent(self, x: torch.Tensor, pad: bool = True) -> torch.Tensor:
        return self._encoder(self._padding(x) if pad else x)

    def residual_backward(self, code: torch.Tensor, level: int) -> torch.Tensor:
        """[n, c, 2h, 2w] <- ([n, m, h, w], level)  (compressor.py:233-235)."""
        with torch.no_grad():
            return self._quantizer.residual_backward(code, level)

    def residual_forward(self, code: torch.Tensor, formerLevel, level: int) -> torch.Tensor:
        """compressor.py:237-239."""
        with torch.no_grad():
            return self._quantizer.residual_forward(code, formerLevel, level)
