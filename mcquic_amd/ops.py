"""Tensor-level wrappers over the C-ABI of libmcquic_hip.so.

PyTorch is used here only for device memory (torch.empty) and the current HIP stream; every op below
is a hand-written gfx950 kernel reached through ctypes.  CPU tensors are rejected -- there is no
fallback implementation.
"""
from __future__ import annotations

import ctypes
import math
import os
from typing import List, Optional, Sequence

import torch

from . import _lib
from ._lib import (CONV_DSILU_MUL, CONV_DUAL_SILU, CONV_MUL, CONV_GATE, CONV_GDN, CONV_IGDN, CONV_RESIDUAL, CONV_SHUFFLE2, CONV_SILU_IN,
                   CONV_SILU_OUT, CONV_SQUARE_IN, CONV_WINOGRAD, CONV_WINOGRAD2D, CONV_WINOGRAD2D16, CONV_GDN_BWD, CONV_IGDN_BWD, CONV_GATE_BWD, CONV_TAPS_LR, CONV_POST_GDN, CONV_POST_IGDN, CONV_POST_GATE, ConvDesc, check)
from ._lib import (AUG_COLUMNS, AUG_TOP, AUG_LEFT, AUG_H, AUG_W, AUG_GAMMA_MODE, AUG_GAMMA, AUG_GAIN0, AUG_GAIN2, AUG_HFLIP, AUG_VFLIP,     # noqa: F401
                   AUG_GAIN_ROW, AUG_FALLBACK, AUG_OUTPUT, AUG_GAMMA_SRGB_TO_LINEAR, AUG_GAMMA_LINEAR_TO_SRGB, AUG_GAMMA_POWER,
                   AUG_GAMMA_IDENTITY, AUG_OUT_NORMALIZED, AUG_OUT_CLAMPED, AUG_OUT_RAW)

# OPT-IN fast path, never the default and never the headline bench: large 3x3 stride-1 layers in the Winograd F(2, 3) form
# along x (mcq_pack_conv_weight_winograd_f32 + MCQ_CONV_WINOGRAD): 2/3 of the multiplications, float32 throughout, but not
# the reference's arithmetic -- results differ from the direct form in the last bits, so near-tie code indices may move.
_WINOGRAD = os.environ.get("MCQUIC_AMD_WINOGRAD", "0") in ("1", "2")
# ... and where Cout % 128 == 0, in both directions: F(2x2, 3x3), 4/9 of the multiplications (MCQUIC_AMD_WINOGRAD=2)
_WINOGRAD_2D = os.environ.get("MCQUIC_AMD_WINOGRAD", "0") == "2"
_WINOGRAD_MIN_PIXELS = int(os.environ.get("MCQUIC_AMD_WINOGRAD_MIN_PIXELS", str(128 * 1024)))   # N*H*W below this: direct form
# (the 2-D form still wins far below that: 32 x 48x32 maps 112 -> 86 us per launch, one 192x128 map at batch 1 -- 24 k pixels --
#  7.3 -> 6.0 ms per encode+decode with the maps above it; at 12 k pixels, 32 x 24x16, it loses, 41 -> 44 us)
_WINOGRAD_MIN_PIXELS_2D = int(os.environ.get("MCQUIC_AMD_WINOGRAD_MIN_PIXELS_2D", str(20 * 1024)))
# which instance runs the F(2x2, 3x3) layers: 16 = v_mfma_f32_16x16x4_f32, two waves per SIMD (csrc/conv_wino16.hip; layers with
# Cin % 16 == 0 and a SiLU / residual / twin / PixelShuffle epilogue), 32 = the one-wave-per-SIMD 32x32x2 instance of conv_mfma_kernel
# (csrc/conv_wino32.hip)
_W2D_KERNEL = int(os.environ.get("MCQUIC_AMD_W2D_KERNEL", "16"))
_W16_EPILOGUES = CONV_SILU_OUT | CONV_RESIDUAL | CONV_DUAL_SILU


def winograd_enabled() -> int:
    """0 = off (the default), 1 = F(2, 3) along x, 2 = F(2x2, 3x3) where the layer allows it."""
    return (2 if _WINOGRAD_2D else 1) if _WINOGRAD else 0


def set_winograd(enabled, min_pixels: Optional[int] = None) -> None:
    """Switch the opt-in Winograd path on / off for convolutions packed from now on (nn.Conv2d re-packs on the change):
    False / 0 = off, True / 1 = F(2, 3) along x, 2 = F(2x2, 3x3) for layers with Cout % 128 == 0 (the 1-D form elsewhere).
    `min_pixels`: layers with fewer than N*H*W input pixels keep the direct form (default 128 k)."""
    global _WINOGRAD, _WINOGRAD_2D, _WINOGRAD_MIN_PIXELS, _WINOGRAD_MIN_PIXELS_2D
    _WINOGRAD = bool(enabled)
    _WINOGRAD_2D = enabled is not True and int(enabled) >= 2
    if min_pixels is not None:
        _WINOGRAD_MIN_PIXELS = int(min_pixels)
        _WINOGRAD_MIN_PIXELS_2D = min(_WINOGRAD_MIN_PIXELS_2D, int(min_pixels)) if int(min_pixels) < 128 * 1024 else 20 * 1024

# A producer asked for `dual_silu` hangs silu(y) on its result under this attribute; a consumer asked for
# `silu_in` uses the twin instead of re-evaluating SiLU inside its k-loop (9 taps x 2 half-waves times per
# element).  The twin is stored with y's version counter and storage address: an in-place update of y by a caller
# (y.add_(...), y.copy_(...), y.set_(...)) invalidates it -- the consumer then evaluates SiLU itself -- and views /
# clones never carry it.  (Tensors made under torch.inference_mode() have no version counter and cannot be checked;
# nothing in this package updates activations in place.)
_TWIN = "_mcq_silu_twin"


def silu_twin(t: torch.Tensor) -> Optional[torch.Tensor]:
    rec = getattr(t, _TWIN, None)
    if rec is None:
        return None
    twin, version, ptr = rec
    if version != tensor_version(t) or ptr != t.data_ptr():
        delattr(t, _TWIN)                       # y changed since the producer wrote silu(y): stale
        return None
    return twin


def set_silu_twin(t: torch.Tensor, twin: torch.Tensor) -> None:
    setattr(t, _TWIN, (twin, tensor_version(t), t.data_ptr()))



def tensor_version(t: torch.Tensor) -> int:
    """`t._version` for cache keys; tensors created under torch.inference_mode() (the reference CLI builds its model
    there, mcquic/cli.py:60) do not track one -- they cannot be updated by an optimizer either, so the storage
    pointer alone identifies their contents."""
    try:
        return t._version
    except RuntimeError:
        return -1


# Host-side cost matters where launches are ~10 us of GPU work (batch 1, the training step's ~4700 launches): the raw
# stream handle and a device guard that does nothing when the tensor already lives on the current device replace
# torch.cuda.current_stream() / torch.cuda.device(), which cost ~4 us and ~3 us per call.
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream() -> int:
    """hipStream_t of the current device's current stream (call inside `_guard`)."""
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


class _guard:
    """`with _guard(t.device):` makes t's device current for the launch, like torch.cuda.device, but free when it already is."""
    __slots__ = ("idx", "prev")

    def __init__(self, device: torch.device):
        self.idx = device.index
        self.prev = -1

    def __enter__(self):
        if self.idx is not None and _cur_device is not None:
            cur = _cur_device()
            if cur != self.idx:
                torch.cuda.set_device(self.idx)
                self.prev = cur
        elif self.idx is not None:
            self.prev = torch.cuda.current_device()
            torch.cuda.set_device(self.idx)
        return self

    def __exit__(self, *exc):
        if self.prev >= 0:
            torch.cuda.set_device(self.prev)
        return False


def _dev(t: torch.Tensor, name: str, dtype=torch.float32) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"mcquic_amd: `{name}` must live on a HIP device (got {t.device}); "
                           "the HIP kernels have no CPU fallback")
    if t.dtype != dtype:
        raise TypeError(f"mcquic_amd: `{name}` must be {dtype} (got {t.dtype})")
    return t if t.is_contiguous() else t.contiguous()


def _dev16(t: torch.Tensor, name: str) -> torch.Tensor:
    """`_dev` for the operands of kernels written for 16-byte-aligned tensors (the 128-bit loads of add_kernel / add3_kernel, the
    64- / 128-bit side-tensor accesses of the convolution's pixel-pair and PixelShuffle epilogues, none of which look at the
    address): a contiguous view that starts elsewhere in its allocation (t.flatten()[1:], a slice of a flat gradient buffer) is
    copied to a fresh one.  torch's allocator hands out 512-byte-aligned blocks, so tensors that own their storage pass as they are."""
    t = _dev(t, name)
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _ptr(t: Optional[torch.Tensor]):
    """Device address for a `void*` parameter / struct field (ctypes converts the int; None = NULL)."""
    return None if t is None else t.data_ptr()


class PackedConv:
    """A conv weight re-laid for the MFMA operand stream (+ its bias), see mcq_pack_conv_weight_f32."""

    __slots__ = ("wp", "bias", "cout", "cin", "ksize", "wino", "wino2d", "wino16", "lr_taps")
    # lr_taps: the packed 3x3 filter is zero outside its lower-right 2 x 2 taps (the input-gradient stream of a stride-2 layer): launches
    # say so (MCQ_CONV_TAPS_LR) and walk 4 of the 9 taps

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor], copy_bias: bool = True, winograd: Optional[bool] = None):
        weight = _dev(weight.detach(), "weight")
        cout, cin, kh, kw = weight.shape
        if kh != kw or kh not in (1, 3):
            raise ValueError(f"unsupported kernel size {kh}x{kw}")
        lib = _lib.load()
        n = lib.mcq_packed_conv_weight_floats(cout, cin, kh)
        self.wp = torch.empty(n, dtype=torch.float32, device=weight.device)
        with _guard(weight.device):
            check(lib.mcq_pack_conv_weight_f32(_ptr(weight), cout, cin, kh, _ptr(self.wp), _stream()), "mcq_pack_conv_weight_f32")
        # (the copy decouples the pack from later in-place updates of the parameter; a caller that hands over a fresh tensor skips it)
        self.bias = None if bias is None else (_dev(bias.detach(), "bias").clone() if copy_bias else _dev(bias.detach(), "bias"))
        self.cout, self.cin, self.ksize = cout, cin, kh
        self.wino = self.wino2d = self.wino16 = None
        self.lr_taps = False
        level = (2 if _WINOGRAD_2D else 1) if _WINOGRAD else 0
        if winograd is not None:
            level = 1 if winograd is True else int(winograd)
        if level >= 1 and kh == 3 and cout % 64 == 0:
            self.wino = torch.empty(lib.mcq_packed_conv_winograd_floats(cout, cin), dtype=torch.float32, device=weight.device)
            with _guard(weight.device):
                check(lib.mcq_pack_conv_weight_winograd_f32(_ptr(weight), cout, cin, _ptr(self.wino), _stream()),
                      "mcq_pack_conv_weight_winograd_f32")
        if level >= 2 and kh == 3 and cout % 128 == 0 and cin % 8 == 0:
            self.wino2d = torch.empty(lib.mcq_packed_conv_winograd2d_floats(cout, cin), dtype=torch.float32, device=weight.device)
            with _guard(weight.device):
                check(lib.mcq_pack_conv_weight_winograd2d_f32(_ptr(weight), cout, cin, _ptr(self.wino2d), _stream()),
                      "mcq_pack_conv_weight_winograd2d_f32")
            if _W2D_KERNEL == 16 and cin % 16 == 0:
                self.wino16 = torch.empty(lib.mcq_packed_conv_winograd16_floats(cout, cin), dtype=torch.float32, device=weight.device)
                with _guard(weight.device):
                    check(lib.mcq_pack_conv_weight_winograd16_f32(_ptr(weight), cout, cin, _ptr(self.wino16), _stream()),
                          "mcq_pack_conv_weight_winograd16_f32")

    def repack_(self, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> bool:
        """Pack `weight` (+ `bias`) into THIS object's streams, in place: same addresses, no allocation -- what a captured
        hipGraph that reads them (parallel.GraphedTrainStep) and the allocator both prefer to a new object per weight version.
        False (nothing written) when the shapes differ or Winograd streams are involved: the caller then builds a new pack."""
        if self.wino is not None or self.wino2d is not None or self.wino16 is not None or _WINOGRAD:
            return False
        weight = _dev(weight.detach(), "weight")
        cout, cin, kh, kw = weight.shape
        lib = _lib.load()
        if kh != kw or (cout, cin, kh) != (self.cout, self.cin, self.ksize) or weight.device != self.wp.device or \
                self.wp.numel() != lib.mcq_packed_conv_weight_floats(cout, cin, kh) or (bias is None) != (self.bias is None):
            return False
        if bias is not None:
            bias = _dev(bias.detach(), "bias")
            if bias.data_ptr() != self.bias.data_ptr():       # (a pack that references the live parameter has nothing to copy)
                if bias.shape != self.bias.shape:
                    return False
                try:
                    self.bias.copy_(bias)
                except RuntimeError:                          # (a copy made under torch.inference_mode() cannot be updated outside it)
                    return False
        with _guard(weight.device):
            check(lib.mcq_pack_conv_weight_f32(_ptr(weight), cout, cin, kh, _ptr(self.wp), _stream()), "mcq_pack_conv_weight_f32")
        return True

    @classmethod
    def dgrad(cls, weight: torch.Tensor, stride: int, scale: float = 1.0, winograd: Optional[bool] = None) -> "PackedConv":
        """Operand stream of the layer's input-gradient convolution, packed straight from its OIHW weight in one launch
        (mcq_pack_conv_dgrad_weight_f32): stride 1 -> a [cin, cout, k, k] conv; stride 2 -> a [4 cin, cout, 3, 3] conv whose
        result goes through the PixelShuffle(2) store."""
        weight = _dev(weight.detach(), "weight")
        cout, cin, kh, kw = weight.shape
        lib = _lib.load()
        co_d, ci_d = ctypes.c_int32(0), ctypes.c_int32(0)
        if kh != kw or lib.mcq_dgrad_weight_shape(cout, cin, kh, stride, ctypes.byref(co_d), ctypes.byref(ci_d)) != 0:
            raise NotImplementedError(f"input gradient of a {kh}x{kw} stride-{stride} convolution is not on the path")
        self = cls.__new__(cls)
        self.wp = torch.empty(lib.mcq_packed_conv_weight_floats(co_d.value, ci_d.value, kh), dtype=torch.float32, device=weight.device)
        with _guard(weight.device):
            check(lib.mcq_pack_conv_dgrad_weight_f32(_ptr(weight), cout, cin, kh, stride, float(scale), _ptr(self.wp), _stream()),
                  "mcq_pack_conv_dgrad_weight_f32")
        self.bias = None
        self.cout, self.cin, self.ksize = co_d.value, ci_d.value, kh
        self.wino = self.wino2d = self.wino16 = None
        self.lr_taps = stride == 2 and kh == 3
        if (winograd if winograd is not None else _WINOGRAD) and kh == 3 and stride == 1 and scale == 1.0 and cin % 64 == 0:
            self.wino = torch.empty(lib.mcq_packed_conv_winograd_floats(cin, cout), dtype=torch.float32, device=weight.device)
            with _guard(weight.device):
                check(lib.mcq_pack_conv_dgrad_weight_winograd_f32(_ptr(weight), cout, cin, _ptr(self.wino), _stream()),
                      "mcq_pack_conv_dgrad_weight_winograd_f32")
        return self


# (round 6) the 1x1 layer BEHIND a 3x3 convolution inside that convolution's launch (MCQ_CONV_POST_*: GDN / IGDN after a strided /
# shuffle convolution, the AttentionBlock's gate after its side stack): A/B switch, 0 = always its own launch
# ("1" = all, "0" = none, or a comma list of gdn / igdn / gate)
# Round 6: 3x3 stride-1 launches that store no SiLU twin run the PIXEL-PAIR form of the unsplit 128 x 64 tile (tile bit 0x400, round 5:
# a third fewer activation loads, 64 / 128-bit epilogue accesses, the same bits -- tests/test_gpu_ops.py::test_conv_pixel_pair_tile_is_bit_equal)
# from 160 k output pixels up, i.e. where the launcher takes that tile for several rounds of the chip: -0.8 % on such launches, the
# 32-image step +0.17 % (258.76 -> 259.19 images/s over four alternating runs).  With a twin the form loses 1 %, on one-round launches
# the replay hides the gain, and a forced tile bit on small maps would take the 16 x 16 tile kernel away from them (measured: one
# image 5.67 -> 5.78 ms) -- hence the conditions.  MCQUIC_AMD_PAIR_RULE=0: the standing tile everywhere (A/B).
_PAIR_RULE = os.environ.get("MCQUIC_AMD_PAIR_RULE", "1") != "0"
_PAIR_MIN_PIXELS = int(os.environ.get("MCQUIC_AMD_PAIR_MIN_PIXELS", str(160 * 1024)))
_fp = os.environ.get("MCQUIC_AMD_FUSE_POST", "1")
_FUSE_POST = {"gdn", "igdn", "gate"} if _fp == "1" else set() if _fp == "0" else set(_fp.split(","))
# wave tiles (128 channels x 32 pixels) from which a launch is fused: the library's own rule is 2048 (two per SIMD); one image's large
# maps gain from 768 up (tools/bench_post.py --batch1), forced through tile 0x41
_POST_MIN_WAVES = int(os.environ.get("MCQUIC_AMD_POST_MIN_WAVES", "768"))


class PackedPost:
    """A [128, 128] 1x1 layer (+ bias) in the operand order of the MCQ_CONV_POST_* epilogues (mcq_pack_post1x1_weight_f32): its
    contraction runs over the producing wave's accumulator registers, in their order."""

    __slots__ = ("wp", "bias")

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor]):
        weight = _dev(weight.detach(), "weight")
        if tuple(weight.shape[:2]) != (128, 128) or weight.numel() != 128 * 128:
            raise ValueError("PackedPost: a [128, 128] 1x1 layer")
        lib = _lib.load()
        self.wp = torch.empty(lib.mcq_packed_post1x1_floats(), dtype=torch.float32, device=weight.device)
        with _guard(weight.device):
            check(lib.mcq_pack_post1x1_weight_f32(_ptr(weight), _ptr(self.wp), _stream()), "mcq_pack_post1x1_weight_f32")
        self.bias = None if bias is None else _dev(bias.detach(), "bias").clone()


def post_ok(x: torch.Tensor, w: "PackedConv", stride: int, kind: str, shuffle2: bool = False) -> int:
    """Does the 1x1 layer `kind` ("gdn" / "igdn" / "gate") behind the 3x3 convolution `w` of `x` run inside that convolution's launch?
    0 = no (the caller launches it on its own), else the `tile` to pass with the post_* option: 1 = the library's own choice (maps
    that fill the chip with unsplit 128-row tiles), 0x41 = forced (fewer tiles than that, still a measured gain)."""
    if kind not in _FUSE_POST or not x.is_cuda or w.ksize != 3 or _WINOGRAD or _band_rows(x, w, stride):
        return 0
    flag = {"gdn": CONV_POST_GDN, "igdn": CONV_POST_IGDN, "gate": CONV_POST_GATE}[kind] | (CONV_SHUFFLE2 if shuffle2 else 0)
    n, cin, h, wd = x.shape
    waves = int(_lib.load().mcq_conv2d_post_ok(n, cin, h, wd, w.cout, w.ksize, stride, flag))
    if waves < max(_POST_MIN_WAVES, 1):
        return 0
    return 1 if waves >= 2048 else 0x41


def pack_convs(weights: Sequence[torch.Tensor], biases: Optional[Sequence[Optional[torch.Tensor]]] = None, *, dgrad: bool = False,
               stride: int = 1, scale: float = 1.0, into: Optional[Sequence[Optional[PackedConv]]] = None,
               masks: Optional[Sequence[int]] = None) -> List[PackedConv]:
    """PackedConv (or PackedConv.dgrad) of several weights of ONE shape in ceil(n / 16) launches
    (mcq_pack_conv_weight_multi_f32).  The biases are referenced, not copied: this is the re-pack after an optimizer step,
    whose caller re-packs again whenever a parameter changes."""
    lib = _lib.load()
    ws = [_dev(w.detach(), "weight") for w in weights]
    if not ws:
        return []
    cout, cin, kh, kw = ws[0].shape
    if any(w.shape != ws[0].shape or w.device != ws[0].device for w in ws):
        raise ValueError("pack_convs: all weights must have one shape and one device")
    co, ci = cout, cin
    if dgrad:
        co_d, ci_d = ctypes.c_int32(0), ctypes.c_int32(0)
        if kh != kw or lib.mcq_dgrad_weight_shape(cout, cin, kh, stride, ctypes.byref(co_d), ctypes.byref(ci_d)) != 0:
            raise NotImplementedError(f"input gradient of a {kh}x{kw} stride-{stride} convolution is not on the path")
        co, ci = co_d.value, ci_d.value
    if kh != kw or kh not in (1, 3):
        raise ValueError(f"unsupported kernel size {kh}x{kw}")
    if co <= 16 and kh == 3:                                   # narrow layers carry a second copy: one by one
        if dgrad:
            return [PackedConv.dgrad(w, stride, scale) for w in ws]
        return [PackedConv(w, None if biases is None else biases[i], copy_bias=False) for i, w in enumerate(ws)]
    floats = lib.mcq_packed_conv_weight_floats(co, ci, kh)
    # `into`: the streams these weights were packed into before -- the re-pack after an optimizer step writes them in place
    # (same stream order as the launches that read them; no allocation, no new objects, addresses a captured graph can keep)
    reuse = into is not None and len(into) == len(ws) and all(
        pk is not None and pk.wp.numel() == floats and pk.wp.device == ws[0].device and pk.wino is None and pk.wino2d is None and pk.wino16 is None
        and (pk.cout, pk.cin, pk.ksize) == (co, ci, kh) for pk in into)
    slab = None if reuse else torch.empty((len(ws), floats), dtype=torch.float32, device=ws[0].device)
    dsts = [pk.wp for pk in into] if reuse else [slab[i] for i in range(len(ws))]
    cap = lib.mcq_pack_conv_weight_max_multi()
    with _guard(ws[0].device):
        for at in range(0, len(ws), cap):
            n = min(cap, len(ws) - at)
            src = (ctypes.c_void_p * n)(*[w.data_ptr() for w in ws[at:at + n]])
            dst = (ctypes.c_void_p * n)(*[d.data_ptr() for d in dsts[at:at + n]])
            if reuse and masks is not None:
                # (only ever for an in-place re-pack: the copies the mask leaves out keep what an earlier full pack wrote)
                mk = (ctypes.c_uint8 * n)(*[int(m) & 15 for m in masks[at:at + n]])
                check(lib.mcq_pack_conv_weight_multi_masked_f32(src, dst, mk, n, cout, cin, kh, 1 if dgrad else 0, stride, float(scale), _stream()),
                      "mcq_pack_conv_weight_multi_masked_f32")
            else:
                check(lib.mcq_pack_conv_weight_multi_f32(src, dst, n, cout, cin, kh, 1 if dgrad else 0, stride, float(scale), _stream()),
                      "mcq_pack_conv_weight_multi_f32")
    if reuse:
        for i, pk in enumerate(into):
            pk.bias = None if dgrad or biases is None or biases[i] is None else _dev(biases[i].detach(), "bias")
        return list(into)
    out = []
    for i in range(len(ws)):
        pk = PackedConv.__new__(PackedConv)
        pk.wp = slab[i]
        pk.bias = None if dgrad or biases is None or biases[i] is None else _dev(biases[i].detach(), "bias")
        pk.cout, pk.cin, pk.ksize = co, ci, kh
        pk.wino = pk.wino2d = pk.wino16 = None
        pk.lr_taps = bool(dgrad) and stride == 2 and kh == 3
        out.append(pk)
    return out


def section_trace(on: bool) -> None:
    """Start (clearing earlier records) / stop recording which copy of its operand stream every conv launch reads
    (mcq_conv_section_trace); `sections_used(pack)` reads a stream's record back.  parallel.GraphedTrainStep uses it so that the
    re-pack inside its captured step refreshes only the copies the captured launches read."""
    _lib.load().mcq_conv_section_trace(1 if on else 0)


def sections_used(pack: Optional[PackedConv]) -> int:
    """Mask of the copies of `pack.wp` read by conv launches since section_trace(True) (0 = none seen = treat as all)."""
    return 0 if pack is None else int(_lib.load().mcq_conv_sections_used(pack.wp.data_ptr()))


def _conv_desc(x: torch.Tensor, w: PackedConv, stride: int = 1, *, silu_in: bool = False, square_in: bool = False,
               silu_out: bool = False, res: Optional[torch.Tensor] = None, res_scale: float = 1.0,
               gdn_mul: Optional[torch.Tensor] = None, igdn_mul: Optional[torch.Tensor] = None,
               gate_mul: Optional[torch.Tensor] = None, gate_id: Optional[torch.Tensor] = None,
               mul: Optional[torch.Tensor] = None, dsilu_mul: Optional[torch.Tensor] = None, shuffle2: bool = False,
               dual_silu: bool = False, tile: int = 0, winograd: Optional[bool] = None,
               post_gdn: Optional["PackedPost"] = None, post_igdn: Optional["PackedPost"] = None, post_gate: Optional["PackedPost"] = None):
    """(mcq_conv_desc, y, y_silu or None, tensors the descriptor points at) for one fused conv launch."""
    if silu_in:
        twin = silu_twin(x)
        if twin is not None:
            x, silu_in = twin, False
    x = _dev16(x, "x")
    n, cin, h, wd = x.shape
    if cin != w.cin:
        raise ValueError(f"channel mismatch: x has {cin}, weight expects {w.cin}")
    pad = w.ksize // 2
    ho = (h + 2 * pad - w.ksize) // stride + 1
    wo = (wd + 2 * pad - w.ksize) // stride + 1
    flags = 0
    if silu_in:
        flags |= CONV_SILU_IN
    if square_in:
        flags |= CONV_SQUARE_IN
    if silu_out:
        flags |= CONV_SILU_OUT
    if shuffle2:
        flags |= CONV_SHUFFLE2
        y = torch.empty((n, w.cout // 4, 2 * ho, 2 * wo), dtype=torch.float32, device=x.device)
    else:
        y = torch.empty((n, w.cout, ho, wo), dtype=torch.float32, device=x.device)
    y2 = None
    if dual_silu:
        flags |= CONV_DUAL_SILU
        y2 = torch.empty_like(y)
    mul_in = mul
    mul = None
    if res is not None:
        flags |= CONV_RESIDUAL
        res = _dev16(res, "res")
        if res.shape != y.shape:
            raise ValueError(f"residual shape {tuple(res.shape)} != output shape {tuple(y.shape)}")
    for flag, t in ((CONV_GDN, gdn_mul), (CONV_IGDN, igdn_mul), (CONV_GATE, gate_mul), (CONV_MUL, mul_in), (CONV_DSILU_MUL, dsilu_mul)):
        if t is not None:
            if not (flag == CONV_GATE and post_gate is not None):     # (post_gate: the gate closes the FUSED 1x1 layer, MCQ_CONV_POST_GATE)
                flags |= flag
            mul = _dev16(t, "mul")
            if mul.shape != y.shape:
                raise ValueError(f"mul shape {tuple(mul.shape)} != output shape {tuple(y.shape)}")
    if gate_id is not None:
        gate_id = _dev16(gate_id, "gate_id")
        if gate_id.shape != y.shape:
            raise ValueError("gate identity shape mismatch")
    post = None
    for flag, pk in ((CONV_POST_GDN, post_gdn), (CONV_POST_IGDN, post_igdn), (CONV_POST_GATE, post_gate)):
        if pk is not None:
            if post is not None:
                raise ValueError("one fused 1x1 layer per launch")
            flags |= flag
            post = pk
    if post is not None:
        winograd = False                             # (the fused 1x1 layer lives in the direct kernel's epilogue)
    wp = w.wp
    auto_2d = winograd is None and _WINOGRAD and _WINOGRAD_2D and w.wino2d is not None and n * h * wd >= _WINOGRAD_MIN_PIXELS_2D
    if winograd or auto_2d or (winograd is None and _WINOGRAD and n * h * wd >= _WINOGRAD_MIN_PIXELS):
        ok = w.wino is not None and stride == 1 and not (flags & (CONV_SILU_IN | CONV_SQUARE_IN))
        two_d = w.wino2d is not None and (_WINOGRAD_2D if winograd is None or winograd is True else int(winograd) >= 2)
        if winograd is not None and winograd is not True and int(winograd) >= 2 and w.wino2d is None:
            raise ValueError("winograd=2 needs a 3x3 layer with Cout % 128 == 0 and Cin % 8 == 0, packed with winograd=2")
        if ok and two_d and _W2D_KERNEL == 16 and w.wino16 is not None and (
                (flags & ~_W16_EPILOGUES) == 0 or flags == CONV_SHUFFLE2):
            flags |= CONV_WINOGRAD2D16               # the two-waves-per-SIMD instance (epilogues it does not carry stay below)
            wp = w.wino16
        elif ok and two_d:
            flags |= CONV_WINOGRAD2D
            wp = w.wino2d
        elif ok:
            flags |= CONV_WINOGRAD
            wp = w.wino
        elif winograd:
            raise ValueError("winograd=True needs a 3x3 stride-1 layer with Cout % 64 == 0, packed with winograd=True, and no input prologue")
    if _TAPS_LR and getattr(w, "lr_taps", False) and stride == 1 and wp is w.wp and not (flags & (CONV_SILU_IN | CONV_SQUARE_IN)):
        flags |= CONV_TAPS_LR
    if (_PAIR_RULE and tile == 0 and w.ksize == 3 and stride == 1 and not dual_silu and dsilu_mul is None and post is None
            and n * ho * wo >= _PAIR_MIN_PIXELS):
        tile = 0x400                                 # (the pixel-pair form wherever the launcher takes the unsplit 128 x 64 tile: see _PAIR_RULE)
    d = ConvDesc(_ptr(x), _ptr(wp), _ptr(w.bias), _ptr(y), _ptr(y2), _ptr(res), _ptr(mul), _ptr(gate_id),
                 n, cin, h, wd, w.cout, w.ksize, stride, flags, float(res_scale), tile,
                 None if post is None else _ptr(post.wp), None if post is None else _ptr(post.bias))
    return d, y, y2, (x, res, mul, gate_id, post)


# ---- images whose activations do not fit one launch --------------------------------------------------------------------------
# The kernels address one image's [C, H, W] slab through 32-bit buffer offsets whose top bit is the out-of-range marker
# (MCQ_ETOOLARGE at 2 GiB): a 6000 x 4000 photo's stem output is 3000 x 2000 x 128 x 4 B = 3.07 GB.  The reference has no limit
# but memory (mcquic/modules/compressor.py:67-117), so such layers run band by band: rows [o0, o1) of the output from the input
# rows under them (+ the 3x3 halo), each band a contiguous copy that fits.  Every output pixel still sees its own taps in the
# kernel's (channel pair, tap) order, so a band's rows are the unsplit launch's rows bit for bit wherever both take the same
# tile / split (tests/test_gpu_model.py::test_row_band_fallback_equals_the_single_launch at a lowered limit).
_SLAB_LIMIT = int(os.environ.get("MCQUIC_AMD_SLAB_LIMIT", str(1 << 31)))
_TENSOR_OPTS = ("res", "gdn_mul", "igdn_mul", "gate_mul", "gate_id", "mul", "dsilu_mul")


def set_slab_limit(nbytes: Optional[int]) -> int:
    """Per-image activation bytes above which a convolution runs in row bands (default 2 GiB = the kernels' own limit); tests
    lower it.  Returns the previous value; None restores the default."""
    global _SLAB_LIMIT
    prev = _SLAB_LIMIT
    _SLAB_LIMIT = (1 << 31) if nbytes is None else int(nbytes)
    return prev


def _slab_bytes(cin: int, h: int, wd: int, cout: int, ho: int, wo: int) -> int:
    """What conv_validate / conv_launch bound (csrc/conv_launch.hip): the input slab plus the prefetch rings' over-read, the output
    slab with its last 128-row tile complete."""
    return max((cin + 32) * h * wd * 4, -(-cout // 128) * 128 * ho * wo * 4)


def _band_rows(x: torch.Tensor, w: PackedConv, stride: int) -> int:
    """0 when the layer fits one launch, else the output rows per band."""
    n, cin, h, wd = x.shape
    pad = w.ksize // 2
    ho, wo = (h + 2 * pad - w.ksize) // stride + 1, (wd + 2 * pad - w.ksize) // stride + 1
    if _slab_bytes(cin, h, wd, w.cout, ho, wo) < _SLAB_LIMIT:
        return 0
    per_row = max((cin + 32) * wd * 4 * stride, -(-w.cout // 128) * 128 * wo * 4)      # bytes one more output row costs
    rows = (_SLAB_LIMIT - 1) // per_row - 4                                            # (halo rows on both sides)
    if rows < 1:
        raise RuntimeError(f"mcquic_amd: one output row of a {cin}->{w.cout} layer on a {wd}-pixel-wide map exceeds the slab limit")
    return int(rows)


def _band_plan(h: int, ksize: int, stride: int, rows: int):
    """[(o0, o1, b0, b1, g0)] covering the output rows of a conv (kernel `ksize`, padding ksize // 2, `stride`) on an `h`-row map in
    bands of at most `rows` output rows: output rows [o0, o1) come from input rows [b0, b1) -- every tap of a kept row is inside
    the band or outside the image, where the conv pads -- and the band's local output row 0 is global output row g0 (b0 is a
    multiple of the stride, so the band's own conv computes rows g0, g0 + 1, ... and rows o0 - g0 .. o1 - g0 of it are kept)."""
    pad = ksize // 2
    ho = (h + 2 * pad - ksize) // stride + 1
    plan = []
    for o0 in range(0, ho, rows):
        o1 = min(ho, o0 + rows)
        b0 = max(0, stride * o0 - stride) if pad else stride * o0
        b1 = min(h, stride * (o1 - 1) + ksize - pad)
        plan.append((o0, o1, b0, b1, b0 // stride))
    return plan


def _conv2d_banded(x: torch.Tensor, w: PackedConv, stride: int, rows: int, fused: dict) -> torch.Tensor:
    if fused.get("silu_in"):
        twin = silu_twin(x)
        if twin is not None:
            x, fused = twin, dict(fused, silu_in=False)
    x = _dev(x, "x")
    n, cin, h, wd = x.shape
    k, pad = w.ksize, w.ksize // 2
    ho, wo = (h + 2 * pad - k) // stride + 1, (wd + 2 * pad - k) // stride + 1
    shuffle2, dual = bool(fused.get("shuffle2")), bool(fused.get("dual_silu"))
    up = 2 if shuffle2 else 1
    y = torch.empty((n, w.cout // 4, 2 * ho, 2 * wo) if shuffle2 else (n, w.cout, ho, wo), dtype=torch.float32, device=x.device)
    y2 = torch.empty_like(y) if dual else None
    sides = {kk: _dev(fused[kk], kk) for kk in _TENSOR_OPTS if fused.get(kk) is not None}
    if shuffle2 and sides:
        # (side inputs have the SHUFFLED output's 2 ho rows; the bands below are cut in pre-shuffle rows.  The kernels take no side
        #  tensor with the PixelShuffle store either -- conv_validate -- so nothing in the model asks for this)
        raise NotImplementedError("row bands: a PixelShuffle store together with output-shaped side tensors is not supported")
    plain = {kk: v for kk, v in fused.items() if kk not in _TENSOR_OPTS}
    for o0, o1, b0, b1, g0 in _band_plan(h, k, stride, rows):
        xb = x[:, :, b0:b1].contiguous()
        hl = (b1 - b0 + 2 * pad - k) // stride + 1
        local = {kk: v[:, :, g0:g0 + hl].contiguous() for kk, v in sides.items()}
        for kk, v in local.items():
            if v.shape[2] != hl:                                    # (the band computes rows past the map's end: pad the side input)
                local[kk] = torch.nn.functional.pad(v, (0, 0, 0, hl - v.shape[2]))
        yb = conv2d(xb, w, stride, **plain, **local)
        lo, hi = up * (o0 - g0), up * (o1 - g0)
        y[:, :, up * o0:up * o1] = yb[:, :, lo:hi]
        if dual:
            y2[:, :, up * o0:up * o1] = silu_twin(yb)[:, :, lo:hi]
    if dual:
        set_silu_twin(y, y2)
    return y


def conv2d(x: torch.Tensor, w: PackedConv, stride: int = 1, **fused) -> torch.Tensor:
    """y = epilogue(conv(prologue(x)) + bias); one kernel launch (mcq_conv2d_f32).  Options: silu_in, square_in, silu_out,
    res (+ res_scale), gdn_mul / igdn_mul / gate_mul (+ gate_id) / mul / dsilu_mul, shuffle2, dual_silu, tile.
    A layer whose per-image slab exceeds the kernels' 2 GiB addressing runs in row bands (same results, see above)."""
    rows = _band_rows(x, w, stride)
    if rows:
        return _conv2d_banded(x, w, stride, rows, fused)
    d, y, y2, keep = _conv_desc(x, w, stride, **fused)
    with _guard(y.device):
        check(_lib.load().mcq_conv2d_f32(ctypes.byref(d), _stream()), "mcq_conv2d_f32")
    if y2 is not None:
        set_silu_twin(y, y2)
    return y


def conv2d_gdn_bwd(x: torch.Tensor, w: PackedConv, dy: torch.Tensor, inverse: bool, tile: int = 0):
    """(dy f(s), dy x f'(s)) with s = beta + gamma @ x^2 recomputed by THIS launch (`w` = the layer's folded 1x1 operand stream):
    the element-wise part of the GDN / IGDN backward as the epilogue of the s-convolution (MCQ_CONV_GDN_BWD / _IGDN_BWD) instead of
    a launch of its own behind a stored s -- one launch and 2 x the tensor less HBM traffic per layer.  `tile` forces the tile height
    (the launcher keeps one pixel block per wave and no split for this epilogue)."""
    x, dy = _dev(x, "x"), _dev(dy, "dy")
    if w.ksize != 1 or x.shape != dy.shape or x.shape[1] != w.cin or w.cout != w.cin:
        raise ValueError("conv2d_gdn_bwd: a square 1x1 layer and dy of x's shape")
    n, c, h, wd = x.shape
    dxd, ds = torch.empty_like(x), torch.empty_like(x)
    d = ConvDesc(_ptr(x), _ptr(w.wp), _ptr(w.bias), _ptr(dxd), _ptr(ds), _ptr(dy), _ptr(x), None,
                 n, c, h, wd, w.cout, 1, 1, CONV_SQUARE_IN | (CONV_IGDN_BWD if inverse else CONV_GDN_BWD), 1.0, tile)
    with _guard(x.device):
        check(_lib.load().mcq_conv2d_f32(ctypes.byref(d), _stream()), "mcq_conv2d_f32")
    return dxd, ds


def conv2d_gate_bwd(bs, ws, as_, douts, tile: int = 0):
    """[(d a_i, d s_i)] of out_i = a_i * sigmoid(s_i) + x_i with s_i = conv1x1(b_i) RECOMPUTED by this launch (`ws[i]` = the gate's
    1x1 operand stream): d a = dout sigmoid(s), d s = dout a sigmoid(s) (1 - sigmoid(s)) leave from the epilogue
    (MCQ_CONV_GATE_BWD), so the forward stores no s and runs the gate as its 1x1 launch's epilogue (mcquic/nn/blocks.py:281-288).
    Several gates of one geometry (the paired heads' AttentionBlocks) share the launch.  `tile`: as for conv2d_gdn_bwd."""
    built = []
    for b, w, a, dout in zip(bs, ws, as_, douts):
        b, a, dout = _dev(b, "b"), _dev(a, "a"), _dev(dout, "dout")
        if w.ksize != 1 or b.shape[1] != w.cin or a.shape != dout.shape or a.shape[1] != w.cout or a.shape[0] != b.shape[0] or a.shape[2:] != b.shape[2:]:
            raise ValueError("conv2d_gate_bwd: a 1x1 layer, `a` and `dout` of its output's shape")
        n, c, h, wd = b.shape
        da, ds = torch.empty_like(a), torch.empty_like(a)
        d = ConvDesc(_ptr(b), _ptr(w.wp), _ptr(w.bias), _ptr(da), _ptr(ds), _ptr(dout), _ptr(a), None,
                     n, c, h, wd, w.cout, 1, 1, CONV_GATE_BWD, 1.0, tile)
        built.append((d, da, ds, (b, a, dout)))
    lib = _lib.load()
    cap = lib.mcq_conv2d_max_multi() if _MULTI else 1
    with _guard(built[0][1].device):
        for lo in range(0, len(built), cap):
            part = built[lo:lo + cap]
            if len(part) == 1:
                check(lib.mcq_conv2d_f32(ctypes.byref(part[0][0]), _stream()), "mcq_conv2d_f32")
            else:
                check(lib.mcq_conv2d_multi_f32((ConvDesc * len(part))(*[p[0] for p in part]), len(part), _stream()), "mcq_conv2d_multi_f32")
    return [(da, ds) for _, da, ds, _ in built]


_MULTI = os.environ.get("MCQUIC_AMD_MULTI_CONV", "1") != "0"      # A/B switch: 0 = one launch per convolution
_TAPS_LR = os.environ.get("MCQUIC_AMD_TAPS_LR", "1") != "0"        # A/B switch: 0 = stride-2 input-gradient launches walk all nine taps (5 of them zeros)


def conv2d_multi(xs, ws, stride: int = 1, per_problem=None, **shared):
    """Independent convolutions of ONE geometry and flag set in one launch (mcq_conv2d_multi_f32): xs[i] through ws[i] with
    the options of `shared` plus per_problem[i] (tensor-valued options such as res= / dsilu_mul=).  Returns [y_i]."""
    n = len(xs)
    per_problem = per_problem or [{}] * n
    lib = _lib.load()
    if n == 1 or not _MULTI or _band_rows(xs[0], ws[0], stride):
        return [conv2d(x, w, stride, **shared, **pp) for x, w, pp in zip(xs, ws, per_problem)]
    cap = lib.mcq_conv2d_max_multi()
    out = []
    for lo in range(0, n, cap):
        built = [_conv_desc(x, w, stride, **shared, **pp) for x, w, pp in zip(xs[lo:lo + cap], ws[lo:lo + cap], per_problem[lo:lo + cap])]
        k = len(built)
        table = (ConvDesc * k)(*[b[0] for b in built])
        with _guard(built[0][1].device):
            check(lib.mcq_conv2d_multi_f32(table, k, _stream()), "mcq_conv2d_multi_f32")
        for _, y, y2, _keep in built:
            if y2 is not None:
                set_silu_twin(y, y2)
            out.append(y)
    return out


def nonneg_reparam(p: torch.Tensor, bound: float, pedestal: float) -> torch.Tensor:
    """max(p, bound)^2 - pedestal (mcquic/nn/base.py:81-84), folded once per weight version."""
    p = _dev(p.detach(), "p")
    out = torch.empty_like(p)
    with _guard(p.device):
        check(_lib.load().mcq_nonneg_reparam_f32(_ptr(p), float(bound), float(pedestal), _ptr(out), p.numel(), _stream()),
              "mcq_nonneg_reparam_f32")
    return out


def nonneg_reparam_multi_(ps, outs, bounds, pedestals) -> None:
    """outs[i] = max(ps[i], bounds[i])^2 - pedestals[i] for many parameters in ceil(n / 64) launches (mcq_nonneg_reparam_multi_f32);
    `outs` are written in place (their addresses are what packed operand streams and captured graphs hold)."""
    lib = _lib.load()
    ps = [_dev(p.detach(), "p") for p in ps]
    for o, p in zip(outs, ps):
        if o.shape != p.shape or o.dtype != torch.float32 or not o.is_contiguous() or o.device != p.device:
            raise ValueError("nonneg_reparam_multi_: every output must be a contiguous float32 tensor of its parameter's shape")
    cap = lib.mcq_nonneg_reparam_max_multi()
    with _guard(ps[0].device):
        for lo in range(0, len(ps), cap):
            k = min(cap, len(ps) - lo)
            src = (ctypes.c_void_p * k)(*[p.data_ptr() for p in ps[lo:lo + k]])
            dst = (ctypes.c_void_p * k)(*[o.data_ptr() for o in outs[lo:lo + k]])
            ns = (ctypes.c_int64 * k)(*[p.numel() for p in ps[lo:lo + k]])
            bd = (ctypes.c_float * k)(*[float(b) for b in bounds[lo:lo + k]])
            pd = (ctypes.c_float * k)(*[float(b) for b in pedestals[lo:lo + k]])
            check(lib.mcq_nonneg_reparam_multi_f32(src, dst, ns, bd, pd, k, _stream()), "mcq_nonneg_reparam_multi_f32")


def nonneg_reparam_bwd(p: torch.Tensor, dfolded: torch.Tensor, bound: float) -> torch.Tensor:
    """Gradient of max(p, bound)^2 - pedestal w.r.t. p under LowerBound's rule (mcq_nonneg_reparam_bwd_f32)."""
    p, dfolded = _dev(p.detach(), "p"), _dev(dfolded, "dfolded")
    if p.shape != dfolded.shape:
        raise ValueError("nonneg_reparam_bwd: shape mismatch")
    out = torch.empty_like(p)
    with _guard(p.device):
        check(_lib.load().mcq_nonneg_reparam_bwd_f32(_ptr(p), _ptr(dfolded), float(bound), _ptr(out), p.numel(), _stream()),
              "mcq_nonneg_reparam_bwd_f32")
    return out


def nonneg_reparam_bwd2(p0: torch.Tensor, d0: torch.Tensor, bound0: float, p1: torch.Tensor, d1: torch.Tensor, bound1: float):
    """nonneg_reparam_bwd for two parameters (a GDN layer's beta and gamma) in one launch (mcq_nonneg_reparam_bwd2_f32)."""
    p0, d0, p1, d1 = _dev(p0.detach(), "p0"), _dev(d0, "d0"), _dev(p1.detach(), "p1"), _dev(d1, "d1")
    if p0.numel() != d0.numel() or p1.numel() != d1.numel():
        raise ValueError("nonneg_reparam_bwd2: shape mismatch")
    o0, o1 = torch.empty_like(p0), torch.empty_like(p1)
    with _guard(p0.device):
        check(_lib.load().mcq_nonneg_reparam_bwd2_f32(_ptr(p0), _ptr(d0), float(bound0), _ptr(o0), p0.numel(), _ptr(p1), _ptr(d1), float(bound1),
                                                      _ptr(o1), p1.numel(), _stream()), "mcq_nonneg_reparam_bwd2_f32")
    return o0, o1


class PackedCodebook:
    """Codebook [m, k, d] in MFMA operand order + codeword norms (mcq_vq_pack_codebook_f32).  `rate`: (cdf, lam) of
    `pack_codebook_rate`, whose launch then takes the plain one's place."""

    __slots__ = ("packed", "codebook", "m", "k", "d")

    def __init__(self, codebook: torch.Tensor, rate=None):
        cb = _dev(codebook.detach(), "codebook").clone()
        name, args = "mcq_vq_pack_codebook_f32", ()
        if rate is not None:
            if cb.dim() != 3:
                raise ValueError(f"pack_codebook_rate: codebook must be [m, k, d], got {tuple(cb.shape)}")
            m, k, d = cb.shape
            t = _dev(rate[0], "cdf", torch.uint32)
            if tuple(t.shape) != (m, k + 1) or t.device != cb.device:
                raise ValueError(f"pack_codebook_rate: a codebook [{m}, {k}, {d}] needs a table [{m}, {k + 1}] on {cb.device}, got {tuple(t.shape)} on {t.device}")
            name, args = "mcq_vq_pack_codebook_rate_f32", (_ptr(t), rate[1])
        m, k, d = cb.shape
        lib = _lib.load()
        self.packed = torch.empty(lib.mcq_packed_codebook_floats(m, k, d), dtype=torch.float32, device=cb.device)
        with _guard(cb.device):
            check(getattr(lib, name)(_ptr(cb), *args, m, k, d, _ptr(self.packed), _stream()), name)
        self.codebook, self.m, self.k, self.d = cb, m, k, d


def lambda_f32(lam: float) -> float:
    """`lam` rounded to float32, the type the pack kernel takes it in, as a Python float; ValueError unless that is finite and >= 0
    (1e39 is a finite double and an infinite float)."""
    v = ctypes.c_float(float(lam)).value
    if not (v >= 0.0) or math.isinf(v):
        raise ValueError(f"rd_lambda: every value must be a finite float32 >= 0, got {lam!r}")
    return v


def pack_codebook_rate(codebook: torch.Tensor, cdf: torch.Tensor, lam: float) -> PackedCodebook:
    """A `PackedCodebook` whose norm section carries the rate penalty `lam * bits_k` under `cdf` (uint32 [m, k + 1], one level of
    `pmf_to_quantized_cdf_dev`; bits_k = 16 - log2(cdf[k + 1] - cdf[k])): `vq_assign` on it returns argmin_k (distance + lam * bits_k)
    through the unchanged kernel (mcq_vq_pack_codebook_rate_f32).  `lam` = 0 gives `PackedCodebook(codebook)`'s buffer bit for bit;
    a `lam` that is negative, NaN or infinite as a float32 is a ValueError, raised before anything is allocated.  Usable wherever a `PackedCodebook` is; `vq_gather` reads the plain codebook."""
    return PackedCodebook(codebook, rate=(cdf, lambda_f32(lam)))


def _latent(x: torch.Tensor, cb: PackedCodebook):
    """(x on the device, n, h, w) of a latent [n, m*d, h, w] for the codebook `cb`."""
    x = _dev(x, "x")
    n, c, h, w = x.shape
    if c != cb.m * cb.d:
        raise ValueError(f"latent has {c} channels, codebook expects {cb.m}*{cb.d}")
    return x, n, h, w


def _assign(name: str, x: torch.Tensor, cb: PackedCodebook, n: int, h: int, w: int, *rate) -> torch.Tensor:
    """The codes and the workspace of an assignment launch, and the launch: `name` with `rate` between the pack and the codes."""
    codes = torch.empty((n, cb.m, h, w), dtype=torch.int64, device=x.device)
    lib = _lib.load()
    nbytes = lib.mcq_vq_assign_workspace_bytes(n, cb.m, cb.d, h, w, cb.k)       # > 0: a launch too small to fill the GPU ranges the codewords
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device) if nbytes else None
    with _guard(x.device):
        check(getattr(lib, name)(_ptr(x), _ptr(cb.packed), *rate, _ptr(codes), n, cb.m, cb.d, h, w, cb.k, _ptr(ws), _stream()), name)
    return codes


def vq_assign(x: torch.Tensor, cb: PackedCodebook) -> torch.Tensor:
    """int64 codes [n, m, h, w] = argmin_k distance (mcq_vq_assign_f32)."""
    x, n, h, w = _latent(x, cb)
    return _assign("mcq_vq_assign_ws_f32", x, cb, n, h, w)


def pack_bits(cdf: torch.Tensor) -> torch.Tensor:
    """The `bits` section of one level for `vq_assign_rate_map` from its table `cdf` uint32 [m, k + 1] on the device
    (mcq_vq_pack_bits_f32): float32 in the layout of a packed codebook's norms, fl32(16 - log2 width) per codeword, 0 in the padding,
    +inf for a slot of width 0.  It depends on the table alone -- not on lambda, not on the codebook."""
    t = _dev(cdf, "cdf", torch.uint32)
    if t.dim() != 2 or t.shape[1] < 2:
        raise ValueError(f"pack_bits: a table [m, k + 1], got {tuple(t.shape)}")
    m, k = int(t.shape[0]), int(t.shape[1]) - 1
    lib = _lib.load()
    out = torch.empty(lib.mcq_packed_bits_floats(m, k), dtype=torch.float32, device=t.device)
    with _guard(t.device):
        check(lib.mcq_vq_pack_bits_f32(_ptr(t), m, k, _ptr(out), _stream()), "mcq_vq_pack_bits_f32")
    return out


def vq_assign_rate_map(x: torch.Tensor, cb: PackedCodebook, bits: torch.Tensor, lam: torch.Tensor, strides=None) -> torch.Tensor:
    """int64 codes [n, m, h, w] = argmin_k fma(lambda_v, bits_k, distance), one lambda per latent vector (mcq_vq_assign_rate_map_f32) on
    the PLAIN pack `cb` and `pack_bits`' section.  `lam`: float32 on x's device, finite and >= 0 (`rate_map_levels` makes such buffers).
    `strides` None: lam is [n] (one lambda per image) or [n, h, w], any view with non-negative strides; else the element strides
    (image, row, column) into `lam`'s storage from its first element.  lambda 0 gives `vq_assign`'s code."""
    x, n, h, w = _latent(x, cb)
    lib = _lib.load()
    if not (torch.is_tensor(bits) and bits.is_cuda and bits.device == x.device and bits.dtype == torch.float32 and bits.is_contiguous()
            and bits.numel() == lib.mcq_packed_bits_floats(cb.m, cb.k)):
        raise ValueError(f"vq_assign_rate_map: `bits` must be pack_bits' section for m = {cb.m}, k = {cb.k} on {x.device}")
    if not (torch.is_tensor(lam) and lam.dtype == torch.float32 and lam.device == x.device):
        raise ValueError(f"vq_assign_rate_map: `lam` must be a float32 tensor on {x.device}")
    if strides is None:
        if tuple(lam.shape) == (n,):
            strides = (lam.stride(0), 0, 0)
        elif tuple(lam.shape) == (n, h, w):
            strides = tuple(lam.stride())
        else:
            raise ValueError(f"vq_assign_rate_map: `lam` must be [{n}] or [{n}, {h}, {w}], got {tuple(lam.shape)}")
    sn, sy, sx = (int(s) for s in strides)
    room = lam.untyped_storage().nbytes() // 4 - lam.storage_offset()
    if min(sn, sy, sx) < 0 or (n - 1) * sn + (h - 1) * sy + (w - 1) * sx >= room:
        raise ValueError(f"vq_assign_rate_map: strides {(sn, sy, sx)} are negative or leave `lam`'s storage")
    return _assign("mcq_vq_assign_rate_map_f32", x, cb, n, h, w, _ptr(bits), _ptr(lam), sn, sy, sx)


def rate_map_grids(h0: int, w0: int, levels: int):
    """The code grids below a level-0 grid: [(h_l, w_l)], halving with ceil."""
    grids = [(int(h0), int(w0))]
    for _ in range(1, levels):
        grids.append(((grids[-1][0] + 1) // 2, (grids[-1][1] + 1) // 2))
    return grids


def rate_map_levels(rd_map: torch.Tensor, scales, out=None, error: Optional[torch.Tensor] = None, scales_dev: Optional[torch.Tensor] = None):
    """Every level's lambda buffer from the caller's map in ONE launch (mcq_rate_map_levels_f32).  `rd_map`: float32 on the device, [n]
    (one lambda per image: every level is scale_l * map) or [n, h0, w0] on the level-0 code grid (level l = scale_l * the mean of the
    2 x 2 cells of level l - 1 that exist, taken on the unscaled map, grids halving with ceil); any view with non-negative strides.
    `scales`: one float per level, finite and >= 0 (`lambda_f32`); `scales_dev`: the same as a float32 device tensor, read by the kernel
    instead (a captured launch then takes new scales).  A map value that is negative, NaN or infinite counts as 0 and sets its image's
    word in `error` (int32 [n], on the device, 0 or 1).  Returns (buffers, error); `out` / `error`: the caller's, written in place."""
    who = "rate_map_levels"
    if not (torch.is_tensor(rd_map) and rd_map.is_cuda and rd_map.dtype == torch.float32 and rd_map.dim() in (1, 3) and rd_map.numel() > 0):
        raise ValueError(f"{who}: `rd_map` must be a non-empty float32 device tensor [n] or [n, h0, w0]")
    scales = [lambda_f32(s) for s in scales]
    levels = len(scales)
    lib = _lib.load()
    if levels == 0 or levels > int(lib.mcq_vq_max_levels()):
        raise ValueError(f"{who}: 1 .. {int(lib.mcq_vq_max_levels())} levels")
    if any(int(s) < 0 for s in rd_map.stride()):
        raise ValueError(f"{who}: negative strides")
    dev, n = rd_map.device, int(rd_map.shape[0])
    if rd_map.dim() == 1:
        h0 = w0 = 0
        strides = (rd_map.stride(0), 0, 0)
        shapes = [(n,)] * levels
    else:
        h0, w0 = int(rd_map.shape[1]), int(rd_map.shape[2])
        strides = tuple(rd_map.stride())
        shapes = [(n, h, w) for h, w in rate_map_grids(h0, w0, levels)]
    out = _reassign_rows(out, shapes, torch.float32, dev, "out", who)
    if error is None:
        error = torch.empty(n, dtype=torch.int32, device=dev)
    elif not (error.is_cuda and error.device == dev and error.dtype == torch.int32 and error.numel() == n and error.is_contiguous()):
        raise ValueError(f"{who}: `error` must be {n} contiguous int32 words on {dev}")
    if scales_dev is not None and not (scales_dev.is_cuda and scales_dev.device == dev and scales_dev.dtype == torch.float32
                                       and scales_dev.numel() == levels and scales_dev.is_contiguous()):
        raise ValueError(f"{who}: `scales_dev` must be {levels} contiguous float32 values on {dev}")
    with _guard(dev):
        check(lib.mcq_rate_map_levels_f32(_ptr(rd_map), n, h0, w0, int(strides[0]), int(strides[1]), int(strides[2]),
                                          (ctypes.c_float * levels)(*scales), _ptr(scales_dev), levels,
                                          (ctypes.c_void_p * levels)(*[t.data_ptr() for t in out]), _ptr(error), _stream()),
              "mcq_rate_map_levels_f32")
    return out, error


def rate_search_step(bits: torch.Tensor, target: torch.Tensor, lam: torch.Tensor, bracket: torch.Tensor, done: torch.Tensor,
                     trace_lam: Optional[torch.Tensor], trace_bpp: Optional[torch.Tensor], pixels: float, lambda_max: float, trial: int,
                     trials: int) -> None:
    """One launch of the per-image target-rate search after trial `trial` of `trials` (mcq_rate_search_step; the rule is in the header):
    `bits` double [n, levels] of the trial's codes, `target` double [n]; state `lam` float32 [n], `bracket` float32 [n, 2], `done` int32
    [n] and the traces float32 / double [trials + 1, n] are updated in place on the device."""
    n, levels = int(bits.shape[0]), int(bits.shape[1])
    for t, dt, numel, name in ((bits, torch.float64, n * levels, "bits"), (target, torch.float64, n, "target"), (lam, torch.float32, n, "lam"),
                               (bracket, torch.float32, 2 * n, "bracket"), (done, torch.int32, n, "done"),
                               (trace_lam, torch.float32, (trials + 1) * n, "trace_lam"), (trace_bpp, torch.float64, (trials + 1) * n, "trace_bpp")):
        if t is None and name.startswith("trace"):
            continue
        if not (torch.is_tensor(t) and t.is_cuda and t.device == bits.device and t.dtype == dt and t.numel() == numel and t.is_contiguous()):
            raise ValueError(f"rate_search_step: `{name}` must be {numel} contiguous {dt} values on {bits.device}")
    with _guard(bits.device):
        check(_lib.load().mcq_rate_search_step(_ptr(bits), _ptr(target), _ptr(lam), _ptr(bracket), _ptr(done), _ptr(trace_lam), _ptr(trace_bpp),
                                               n, levels, float(pixels), float(lambda_max), int(trial), int(trials), _stream()),
              "mcq_rate_search_step")


def activity_grid(h: int, w: int, base: int = 128):
    """(h0, w0): the 16 x 16 cells of an h x w image reflect-padded to multiples of `base` (`AlignedPadding`).  RuntimeError where
    reflect cannot make that padding -- a side's padding must be smaller than the image's side -- in the words of torch's reflect pad."""
    h, w, base = int(h), int(w), int(base)
    if base <= 0 or base % 16 != 0:
        raise ValueError(f"activity_cells: `base` must be a positive multiple of 16, got {base}")
    if h <= 0 or w <= 0:
        raise ValueError(f"activity_cells: an empty image ({h} x {w})")
    hpad, wpad = (base - h % base) % base, (base - w % base) % base
    if hpad - hpad // 2 > h - 1 or wpad - wpad // 2 > w - 1:
        raise RuntimeError(f"activity_cells: Padding size should be less than the corresponding input dimension, but got: padding "
                           f"({wpad // 2}, {wpad - wpad // 2}) x ({hpad // 2}, {hpad - hpad // 2}) for an image {h} x {w}")
    return (h + hpad) // 16, (w + wpad) // 16


def activity_cells(x: torch.Tensor, base: int = 128):
    """The activity of every level-0 code cell of an image batch in ONE launch (mcq_activity_cells_f32).  `x`: float32 [n, 3, H, W] on
    the device.  Returns (a, mask, error): a float32 [n, h0, w0] = log2(variance of the cell's luma + 2^-14) over the 16 x 16 cells of the
    image reflect-padded to multiples of `base` (read in place, no padded copy; centred two-pass variance); mask int32 [n, h0, w0] = 1
    where a cell holds a non-finite luma (its `a` is 0); error int32 [n] = 1 for an image with such a cell.  Nothing is read on the host."""
    who = "activity_cells"
    if not (torch.is_tensor(x) and x.dim() == 4 and x.shape[1] == 3 and x.shape[0] > 0):
        raise ValueError(f"{who}: `x` must be a non-empty image batch [n, 3, H, W], got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}")
    x = _dev(x, "x")
    n, _, h, w = (int(s) for s in x.shape)
    h0, w0 = activity_grid(h, w, base)
    a = torch.empty((n, h0, w0), dtype=torch.float32, device=x.device)
    mask = torch.empty((n, h0, w0), dtype=torch.int32, device=x.device)
    error = torch.empty(n, dtype=torch.int32, device=x.device)
    with _guard(x.device):
        check(_lib.load().mcq_activity_cells_f32(_ptr(x), n, h, w, int(base), _ptr(a), _ptr(mask), _ptr(error), _stream()),
              "mcq_activity_cells_f32")
    return a, mask, error


def activity_weights(a: torch.Tensor, mask: torch.Tensor, strength: float, clip: float, roi: Optional[torch.Tensor] = None,
                     lam: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The rate map of one use from `activity_cells`' (a, mask) in ONE launch (mcq_activity_weights_f32): float32 [n, h0, w0] =
    (w * roi) * lam with w = exp2(clamp(strength * (a - abar), -clip, +clip)), abar the image's mean of `a` over its unmasked cells, w = 1
    for a masked cell.  `strength` finite >= 0, `clip` finite > 0.  `roi`: None (1), or a float32 device tensor [n] or [n, h0, w0], any
    view with non-negative strides -- a negative, NaN or infinite value comes out as NaN, which `rate_map_levels` counts as 0 and reports.
    `lam`: None (1) or float32 [n] on the device (the multiplier of the per-image search).  `out`: the caller's buffer, written in place."""
    who = "activity_weights"
    if not (torch.is_tensor(a) and a.is_cuda and a.dtype == torch.float32 and a.dim() == 3 and a.numel() > 0 and a.is_contiguous()):
        raise ValueError(f"{who}: `a` must be a non-empty contiguous float32 device tensor [n, h0, w0]")
    dev, (n, h0, w0) = a.device, (int(s) for s in a.shape)
    if not (torch.is_tensor(mask) and mask.device == dev and mask.dtype == torch.int32 and mask.shape == a.shape and mask.is_contiguous()):
        raise ValueError(f"{who}: `mask` must be contiguous int32 {tuple(a.shape)} on {dev}")
    strength, clip = ctypes.c_float(float(strength)).value, ctypes.c_float(float(clip)).value
    if not (strength >= 0.0) or math.isinf(strength) or not (clip > 0.0) or math.isinf(clip):
        raise ValueError(f"{who}: `strength` must be a finite float32 >= 0 and `clip` a finite float32 > 0, got {strength!r}, {clip!r}")
    strides = (0, 0, 0)
    if roi is not None:
        if not (torch.is_tensor(roi) and roi.device == dev and roi.dtype == torch.float32 and tuple(roi.shape) in ((n,), (n, h0, w0))):
            raise ValueError(f"{who}: `roi` must be a float32 tensor [{n}] or [{n}, {h0}, {w0}] on {dev}")
        if any(int(s) < 0 for s in roi.stride()):
            raise ValueError(f"{who}: negative strides")
        strides = (roi.stride(0), 0, 0) if roi.dim() == 1 else tuple(roi.stride())
    if lam is not None and not (torch.is_tensor(lam) and lam.device == dev and lam.dtype == torch.float32 and tuple(lam.shape) == (n,)
                                and lam.is_contiguous()):
        raise ValueError(f"{who}: `lam` must be {n} contiguous float32 values on {dev}")
    if out is None:
        out = torch.empty((n, h0, w0), dtype=torch.float32, device=dev)
    elif not (torch.is_tensor(out) and out.device == dev and out.dtype == torch.float32 and out.shape == a.shape and out.is_contiguous()):
        raise ValueError(f"{who}: `out` must be contiguous float32 {tuple(a.shape)} on {dev}")
    with _guard(dev):
        check(_lib.load().mcq_activity_weights_f32(_ptr(a), _ptr(mask), n, h0, w0, strength, clip, _ptr(roi), int(strides[0]), int(strides[1]),
                                                   int(strides[2]), _ptr(lam), _ptr(out), _stream()), "mcq_activity_weights_f32")
    return out


def vq_gather(codes: torch.Tensor, cb: PackedCodebook, dual_silu: bool = False) -> torch.Tensor:
    """fp32 [n, m*d, h, w] = codebook[g, codes] (mcq_vq_gather_f32)."""
    codes = _dev(codes, "codes", torch.int64)
    n, m, h, w = codes.shape
    if m != cb.m:
        raise RuntimeError(f"codes carry m={m}, codebook has m={cb.m}")
    out = torch.empty((n, m * cb.d, h, w), dtype=torch.float32, device=codes.device)
    out2 = torch.empty_like(out) if dual_silu else None
    with _guard(codes.device):
        check(_lib.load().mcq_vq_gather_f32(_ptr(codes), _ptr(cb.codebook), _ptr(out), _ptr(out2), n, m, cb.d, h, w, cb.k,
                                            _stream()), "mcq_vq_gather_f32")
    if out2 is not None:
        set_silu_twin(out, out2)
    return out


def vq_logits(x: torch.Tensor, cb: PackedCodebook, temperature: torch.Tensor, bound: float) -> torch.Tensor:
    """Training logits [n, m, h, w, k] = (-dist / sqrt(k)) * max(temperature, bound) (mcq_vq_logits_f32)."""
    x, n, h, w = _latent(x, cb)
    t = _dev(temperature.detach().reshape(-1), "temperature")
    logits = torch.empty((n, cb.m, h, w, cb.k), dtype=torch.float32, device=x.device)
    with _guard(x.device):
        check(_lib.load().mcq_vq_logits_f32(_ptr(x), _ptr(cb.packed), _ptr(t), float(bound), _ptr(logits), n, cb.m, cb.d, h, w,
                                            cb.k, _stream()), "mcq_vq_logits_f32")
    return logits


# ---- the generator behind the soft assignment's draws (csrc/vq_train.hip: rng_uniform) ------------------------------------------
_rng_states = {}


def seed_rng(seed: int, device=None) -> None:
    """(Re)seed the in-kernel generator of `device` (default: the current one) and rewind its offset."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    st = _rng_states.get(dev.index)
    val = torch.tensor([int(seed) & 0x7fffffffffffffff, 0], dtype=torch.int64)
    if st is None:
        _rng_states[dev.index] = val.to(dev)
    else:
        st.copy_(val)


def get_rng_state(device=None) -> torch.Tensor:
    """{seed, offset} of the in-kernel generator of `device` as a CPU int64[2] tensor -- what a checkpoint stores beside
    torch.cuda.get_rng_state() (the soft assignment's draws are NOT torch's stream, so torch's state does not cover them)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    st = _rng_states.get(dev.index)
    if st is None:
        seed_rng(torch.initial_seed(), dev)
        st = _rng_states[dev.index]
    return st.detach().cpu().clone()


def set_rng_state(state: torch.Tensor, device=None) -> None:
    """Restore a state returned by get_rng_state (in place: a captured step keeps reading the same device tensor)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    state = torch.as_tensor(state, dtype=torch.int64).reshape(2)
    st = _rng_states.get(dev.index)
    if st is None:
        _rng_states[dev.index] = state.to(dev)
    else:
        st.copy_(state)


def rng_snapshot(device) -> torch.Tensor:
    """{seed, offset} for ONE pair of draws (a fresh int64[2] device tensor), after which the generator's offset moves on -- both
    on the device and in stream order, so the sequence is captured by a hipGraph and advances on every replay.  Seeded from
    torch's own seed at first use (`torch.manual_seed` before it, or `seed_rng` at any time)."""
    dev = torch.device(device)
    st = _rng_states.get(dev.index)
    if st is None:
        seed_rng(torch.initial_seed(), dev)
        st = _rng_states[dev.index]
    snap = st.clone()
    st[1:].add_(1)
    return snap


class VqStep:
    """What ONE mcq_vq_step_prologue_f32 launch prepared for a training forward of `levels` quantizations: the random drop's
    exponents (float32 [levels]), one generator snapshot per level (int64 [levels, 2]; None when the caller brings the draws)
    and the zeroed code-count buffer the sampling kernels add into (int64, level l at `offsets[l]`; None: no counting)."""

    __slots__ = ("exponents", "snaps", "counts", "offsets", "sizes")

    def level(self, l: int):
        """(drop exponent [1], generator snapshot [2] or None, this level's [m * k] counts or None)."""
        cnt = None if self.counts is None else self.counts[self.offsets[l]: self.offsets[l] + self.sizes[l]]
        return self.exponents[l: l + 1], (None if self.snaps is None else self.snaps[l]), cnt


def vq_step_prologue(freqs: Sequence[torch.Tensor], eps: float, want_rng: bool, counts: Optional[torch.Tensor] = None) -> VqStep:
    """The bookkeeping in front of a training forward's level cascade as ONE launch (mcq_vq_step_prologue_f32): per level the
    exponent of `_randomDrop` from its frequency EMA `freqs[l]` [m_l, k_l] (mcquic/modules/quantizer.py:194-198), a generator
    snapshot per level with the generator advanced past them (`want_rng`), and `counts` (int64, sum of m_l * k_l entries) zeroed."""
    fs = [_dev(f.detach(), "freq_ema") for f in freqs]
    levels = len(fs)
    lib = _lib.load()
    dev = fs[0].device
    ms = (ctypes.c_int32 * levels)(*[int(f.shape[0]) for f in fs])
    ks = (ctypes.c_int32 * levels)(*[int(f.shape[1]) for f in fs])
    st = VqStep()
    st.sizes = [int(f.shape[0]) * int(f.shape[1]) for f in fs]
    st.offsets = [sum(st.sizes[:l]) for l in range(levels)]
    st.exponents = torch.empty(levels, dtype=torch.float32, device=dev)
    st.snaps, state = None, None
    if want_rng:
        state = _rng_states.get(dev.index)
        if state is None:
            seed_rng(torch.initial_seed(), dev)
            state = _rng_states[dev.index]
        st.snaps = torch.empty((levels, 2), dtype=torch.int64, device=dev)
    st.counts = None
    if counts is not None:
        st.counts = _dev(counts, "counts", torch.int64)
        if st.counts.numel() != sum(st.sizes):
            raise ValueError("vq_step_prologue: the count buffer must hold sum(m_l * k_l) entries")
    # (the library's tables hold mcq_vq_max_levels() levels per launch -- 32; the reference's generator configs run 17 -- and
    #  anything beyond goes chunk by chunk: the generator's offset advances by each chunk's level count on the device, so the
    #  snapshots are the ones a single launch would hand out; the count buffer is zeroed whole by the first chunk)
    cap = int(lib.mcq_vq_max_levels())
    with _guard(dev):
        for l0 in range(0, levels, cap):
            nl = min(cap, levels - l0)
            ptrs = (ctypes.c_void_p * nl)(*[f.data_ptr() for f in fs[l0: l0 + nl]])
            ms_c = (ctypes.c_int32 * nl)(*ms[l0: l0 + nl])
            ks_c = (ctypes.c_int32 * nl)(*ks[l0: l0 + nl])
            first = l0 == 0 and st.counts is not None
            check(lib.mcq_vq_step_prologue_f32(ptrs, ms_c, ks_c, nl, float(eps), _ptr(st.exponents[l0: l0 + nl]), _ptr(state),
                                               None if st.snaps is None else _ptr(st.snaps[l0: l0 + nl]),
                                               _ptr(st.counts) if first else None, st.counts.numel() if first else 0, _stream()),
                  "mcq_vq_step_prologue_f32")
    return st


def vq_temperature_grad(dtrow: torch.Tensor, temperature: torch.Tensor, bound: float) -> torch.Tensor:
    """d temperature (the Parameter's shape) from the soft-max backward's per-row terms [n, m, h, w]: their sum over images and
    pixels per group, then LowerBound's gradient rule (mcquic/nn/base.py:24-29) -- one launch (mcq_vq_temperature_grad_f32)."""
    dtrow = _dev(dtrow, "dtrow")
    n, m, h, w = dtrow.shape
    t = _dev(temperature.detach().reshape(-1), "temperature")
    out = torch.empty(temperature.shape, dtype=torch.float32, device=dtrow.device)
    with _guard(dtrow.device):
        check(_lib.load().mcq_vq_temperature_grad_f32(_ptr(dtrow), _ptr(t), float(bound), _ptr(out), n, m, h * w, _stream()),
              "mcq_vq_temperature_grad_f32")
    return out


def freq_ema_update_(freqs: Sequence[torch.Tensor], counts: torch.Tensor, ema: float, skip=None) -> None:
    """In place on every level's frequency EMA [m_l, k_l]: (1 - ema) * counts_l / sum_k counts_l + ema * freq_l
    (mcquic/modules/entropyCoder.py:37-43) for all levels in ONE launch; `counts` = the levels' histograms back to back (int64).
    `skip`: a step's guard flag (one int32 on the device, `guard.StepGuard.skip`): set on the device, no entry moves."""
    fs = [_dev(f.detach(), "freq_ema") for f in freqs]
    for f, g in zip(fs, freqs):
        if f.data_ptr() != g.data_ptr():
            raise ValueError("freq_ema_update_: the frequency tensors must be contiguous (they are updated in place)")
    levels = len(fs)
    counts = _dev(counts, "counts", torch.int64)
    if counts.numel() != sum(int(f.numel()) for f in fs):
        raise ValueError("freq_ema_update_: `counts` must hold sum(m_l * k_l) entries")
    ms = (ctypes.c_int32 * levels)(*[int(f.shape[0]) for f in fs])
    ks = (ctypes.c_int32 * levels)(*[int(f.shape[1]) for f in fs])
    lib = _lib.load()
    cap = int(lib.mcq_vq_max_levels())
    from .guard import skip_pointer
    flag = skip_pointer(skip, counts.device, "freq_ema_update_")
    with _guard(counts.device):
        off = 0
        for l0 in range(0, levels, cap):                     # (a launch's tables hold `cap` levels; see vq_step_prologue)
            nl = min(cap, levels - l0)
            ptrs = (ctypes.c_void_p * nl)(*[f.data_ptr() for f in fs[l0: l0 + nl]])
            ms_c = (ctypes.c_int32 * nl)(*ms[l0: l0 + nl])
            ks_c = (ctypes.c_int32 * nl)(*ks[l0: l0 + nl])
            size = sum(int(f.numel()) for f in fs[l0: l0 + nl])
            check(lib.mcq_freq_ema_update_skip_f32(ptrs, ms_c, ks_c, nl, _ptr(counts[off: off + size]), float(ema), flag, _stream()),
                  "mcq_freq_ema_update_skip_f32")
            off += size


REASSIGN_STATE_WORDS = _lib.MCQ_REASSIGN_STATE_WORDS    # count, seen, fired, moved, proportion (float32, low word), seed, offset
REASSIGN_STREAM = _lib.MCQ_RNG_STREAM_REASSIGN          # the generator stream of the drawn priorities


def _reassign_state(state: torch.Tensor, who: str) -> torch.Tensor:
    s = _dev(state, "state", torch.int64)
    if s.data_ptr() != state.data_ptr() or s.numel() != REASSIGN_STATE_WORDS:
        raise ValueError(f"{who}: `state` must be {REASSIGN_STATE_WORDS} contiguous int64 words (it is updated in place)")
    return s


def _reassign_rows(ts, shapes, dtype, dev, name: str, who: str):
    """Per-level [m_l, k_l] buffers of `dtype`: the caller's (checked, written in place) or fresh ones."""
    if ts is None:
        return [torch.empty(s, dtype=dtype, device=dev) for s in shapes]
    ts = list(ts)
    if len(ts) != len(shapes):
        raise ValueError(f"{who}: `{name}` needs one tensor per level")
    for t, s in zip(ts, shapes):
        if not (t.is_cuda and t.device == dev and t.dtype == dtype and tuple(t.shape) == tuple(s) and t.is_contiguous()):
            raise ValueError(f"{who}: `{name}` must be contiguous {dtype} {tuple(s)} tensors on {dev} (they are written in place)")
    return ts


def vq_reassign_plan(freqs: Sequence[torch.Tensor], state: torch.Tensor, every: int, start: int = 0, priorities=None, skip=None,
                     source=None, refill=None):
    """The first of codebook reassignment's two launches (mcq_vq_reassign_plan), for all levels at once: from every level's RAW frequency
    EMA `freqs[l]` [m_l, k_l] the donor index per codeword `source[l]` (int32 [m_l, k_l]; a codeword's own index where nothing moves) and
    the mask `refill[l]` (bool [m_l, k_l]), by the rule of `_multiCodebookQuantization.reAssignCodebook`.  `priorities`: None, or per level
    a float32 [m_l, k_l] tensor or None -- a missing row is drawn under the generator state inside `state` (level l under {seed, offset +
    l}, stream `REASSIGN_STREAM`: `hash_uniform` of that snapshot).  `state`: the int64 [REASSIGN_STATE_WORDS] record (include/mcquic_hip.h);
    this launch advances its count and decides from it, `every` and `start` whether the step fires -- when it does not, or when `skip` (a
    step's guard flag) is set on the device, nothing else is written.  Returns (source, refill): the caller's buffers, or fresh ones."""
    who = "vq_reassign_plan"
    fs = [_dev(f.detach(), "freq_ema") for f in freqs]
    levels = len(fs)
    if levels == 0 or any(f.dim() != 2 for f in fs):
        raise ValueError(f"{who}: one [m, k] frequency tensor per level")
    dev = fs[0].device
    state = _reassign_state(state, who)
    if int(every) < 1 or int(start) < 0:
        raise ValueError(f"{who}: every >= 1 and start >= 0 are required")
    lib = _lib.load()
    kmax = int(lib.mcq_vq_reassign_max_k())
    if any(int(f.shape[1]) > kmax for f in fs):
        raise ValueError(f"{who}: a row of {max(int(f.shape[1]) for f in fs)} codewords does not fit the kernel's LDS arrays (at most {kmax})")
    shapes = [tuple(f.shape) for f in fs]
    source = _reassign_rows(source, shapes, torch.int32, dev, "source", who)
    refill = _reassign_rows(refill, shapes, torch.bool, dev, "refill", who)
    prios = [None] * levels if priorities is None else [None if p is None else _dev(p.detach(), "priority") for p in priorities]
    if len(prios) != levels or any(p is not None and tuple(p.shape) != s for p, s in zip(prios, shapes)):
        raise ValueError(f"{who}: `priorities` needs one [m, k] tensor (or None) per level")
    from .guard import skip_pointer
    flag = skip_pointer(skip, dev, who)
    cap = int(lib.mcq_vq_max_levels())
    with _guard(dev):
        for l0 in range(0, levels, cap):                     # (a launch's tables hold `cap` levels; see vq_step_prologue)
            sl = slice(l0, min(levels, l0 + cap))
            nl = sl.stop - l0
            check(lib.mcq_vq_reassign_plan((ctypes.c_void_p * nl)(*[f.data_ptr() for f in fs[sl]]),
                                           (ctypes.c_void_p * nl)(*[_ptr(p) for p in prios[sl]]),
                                           (ctypes.c_int32 * nl)(*[s[0] for s in shapes[sl]]), (ctypes.c_int32 * nl)(*[s[1] for s in shapes[sl]]),
                                           nl, l0, int(l0 == 0), (ctypes.c_void_p * nl)(*[t.data_ptr() for t in source[sl]]),
                                           (ctypes.c_void_p * nl)(*[t.data_ptr() for t in refill[sl]]), _ptr(state), int(every), int(start),
                                           flag, _stream()), "mcq_vq_reassign_plan")
    return source, refill


def vq_reassign_scratch_floats(codebooks: Sequence[torch.Tensor]) -> int:
    """Floats of scratch `vq_reassign_apply` needs for these codebooks: the largest group, k_l * d_l."""
    return max(int(c.shape[1]) * int(c.shape[2]) for c in codebooks)


def vq_reassign_apply(codebooks: Sequence[torch.Tensor], source, refill, state: torch.Tensor, every: int, start: int = 0, skip=None,
                      changed=None, scratch: Optional[torch.Tensor] = None):
    """The second launch (mcq_vq_reassign_apply): on a step that fires -- the same decision, from the same words -- codebook[l][g, i] =
    the OLD codebook[l][g, source[l][g, i]] wherever refill[l][g, i], in place on the contiguous `codebooks[l]` [m_l, k_l, d_l]; donors are
    read as they were before any move of this call (a scratch copy per group: `scratch`, `vq_reassign_scratch_floats` float32, or a
    fresh one).  `changed[l]` (bool [m_l, k_l]) = moved by more than 1e-4 in squared distance; `state` takes moved, proportion, fired and the
    generator's advance.  Returns `changed`: the caller's buffers, or fresh ones."""
    who = "vq_reassign_apply"
    cbs = [_dev(c.detach(), "codebook") for c in codebooks]
    for c, given in zip(cbs, codebooks):
        if c.data_ptr() != given.data_ptr() or c.dim() != 3:
            raise ValueError(f"{who}: the codebooks must be contiguous [m, k, d] tensors (they are moved in place)")
    levels = len(cbs)
    if levels == 0:
        raise ValueError(f"{who}: one codebook per level")
    dev = cbs[0].device
    state = _reassign_state(state, who)
    if int(every) < 1 or int(start) < 0:
        raise ValueError(f"{who}: every >= 1 and start >= 0 are required")
    lib = _lib.load()
    kmax = int(lib.mcq_vq_reassign_max_k())
    if any(int(c.shape[1]) > kmax for c in cbs):
        raise ValueError(f"{who}: a row of {max(int(c.shape[1]) for c in cbs)} codewords does not fit the kernel's LDS arrays (at most {kmax})")
    shapes = [tuple(c.shape[:2]) for c in cbs]
    source = _reassign_rows(source, shapes, torch.int32, dev, "source", who)
    refill = _reassign_rows(refill, shapes, torch.bool, dev, "refill", who)
    changed = _reassign_rows(changed, shapes, torch.bool, dev, "changed", who)
    need = vq_reassign_scratch_floats(cbs)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.float32, device=dev)
    scratch = _dev(scratch, "scratch")
    if scratch.numel() < need or scratch.device != dev:
        raise ValueError(f"{who}: `scratch` must hold {need} float32 on {dev}")
    from .guard import skip_pointer
    flag = skip_pointer(skip, dev, who)
    cap = int(lib.mcq_vq_max_levels())
    codewords = sum(s[0] * s[1] for s in shapes)
    with _guard(dev):
        for l0 in range(0, levels, cap):
            sl = slice(l0, min(levels, l0 + cap))
            nl = sl.stop - l0
            check(lib.mcq_vq_reassign_apply((ctypes.c_void_p * nl)(*[c.data_ptr() for c in cbs[sl]]),
                                            (ctypes.c_void_p * nl)(*[t.data_ptr() for t in source[sl]]),
                                            (ctypes.c_void_p * nl)(*[t.data_ptr() for t in refill[sl]]),
                                            (ctypes.c_void_p * nl)(*[t.data_ptr() for t in changed[sl]]),
                                            (ctypes.c_int32 * nl)(*[int(c.shape[0]) for c in cbs[sl]]), (ctypes.c_int32 * nl)(*[int(c.shape[1]) for c in cbs[sl]]),
                                            (ctypes.c_int32 * nl)(*[int(c.shape[2]) for c in cbs[sl]]), nl, int(l0 == 0), int(sl.stop == levels),
                                            levels, codewords, _ptr(scratch), _ptr(state), int(every), int(start), flag, _stream()),
                  "mcq_vq_reassign_apply")
    return changed


CDF_OK, CDF_BAD_ELEMENT, CDF_ZERO_TOTAL, CDF_NO_DONOR = 0, 1, 2, 3      # the status words of mcq_pmf_to_quantized_cdf_dev


def cdf_max_k() -> int:
    """The longest row `pmf_to_quantized_cdf_dev` takes (mcq_cdf_max_k: the kernel holds a row in LDS)."""
    return int(_lib.load().mcq_cdf_max_k())


def pmf_to_quantized_cdf_dev(pmfs: Sequence[torch.Tensor], normalize: bool = False, out=None, status: Optional[torch.Tensor] = None):
    """The 16-bit quantized CDF tables of every level and group in ONE launch (mcq_pmf_to_quantized_cdf_dev): `pmfs[l]` float32 [m_l, k_l]
    -> uint32 [m_l, k_l + 1], entry for entry what the host function `pmfToQuantizedCDF(row, 16)` returns for each row.  `normalize`:
    each row is first divided by its sum (formed in double in a fixed order, rounded once to float32); else the rows are taken as given.
    Returns (tables, status): `status` int32 [sum m_l] in (level, group) order stays on the device -- 0 valid, CDF_BAD_ELEMENT a negative
    or non-finite element, CDF_ZERO_TOTAL (with `normalize`: a row sum of zero), CDF_NO_DONOR; a row with a non-zero status leaves its table unspecified.  `out` / `status`: the
    caller's buffers (written in place: a captured launch keeps their addresses), or fresh ones.  Rows longer than `cdf_max_k()` are a
    ValueError."""
    who = "pmf_to_quantized_cdf_dev"
    ps = [_dev(p.detach(), "pmf") for p in pmfs]
    levels = len(ps)
    if levels == 0 or any(p.dim() != 2 or p.numel() == 0 for p in ps):
        raise ValueError(f"{who}: one non-empty [m, k] probability tensor per level")
    dev = ps[0].device
    lib = _lib.load()
    kmax = int(lib.mcq_cdf_max_k())
    if any(int(p.shape[1]) > kmax for p in ps):
        raise ValueError(f"{who}: a row of {max(int(p.shape[1]) for p in ps)} symbols does not fit the kernel's LDS array (at most {kmax})")
    shapes = [(int(p.shape[0]), int(p.shape[1]) + 1) for p in ps]
    out = _reassign_rows(out, shapes, torch.uint32, dev, "out", who)
    rows = sum(s[0] for s in shapes)
    if status is None:
        status = torch.empty(rows, dtype=torch.int32, device=dev)
    elif not (status.is_cuda and status.device == dev and status.dtype == torch.int32 and status.numel() == rows and status.is_contiguous()):
        raise ValueError(f"{who}: `status` must be {rows} contiguous int32 words on {dev} (one per row, written in place)")
    cap = int(lib.mcq_vq_max_levels())
    with _guard(dev):
        row0 = 0
        for l0 in range(0, levels, cap):                     # (a launch's tables hold `cap` levels; see vq_step_prologue)
            sl = slice(l0, min(levels, l0 + cap))
            nl = sl.stop - l0
            check(lib.mcq_pmf_to_quantized_cdf_dev((ctypes.c_void_p * nl)(*[p.data_ptr() for p in ps[sl]]),
                                                   (ctypes.c_void_p * nl)(*[t.data_ptr() for t in out[sl]]),
                                                   (ctypes.c_int32 * nl)(*[s[0] for s in shapes[sl]]),
                                                   (ctypes.c_int32 * nl)(*[s[1] - 1 for s in shapes[sl]]), nl, int(bool(normalize)),
                                                   status.data_ptr() + 4 * row0, _stream()), "mcq_pmf_to_quantized_cdf_dev")
            row0 += sum(s[0] for s in shapes[sl])
    return out, status


def code_bits(codes: Sequence[torch.Tensor], cdfs: Sequence[torch.Tensor], out: Optional[torch.Tensor] = None,
              error: Optional[torch.Tensor] = None):
    """What the tables charge for the codes, per image and level, in ONE launch (mcq_code_bits): bits[i, l] = the sum over groups and
    positions of 16 - log2(cdf[c + 1] - cdf[c]) for `codes[l]` int64 [n, m_l, h_l, w_l] under `cdfs[l]` uint32 [m_l, k_l + 1], in double
    in a fixed order (equal inputs give equal bits).  Returns (bits double [n, levels], error int32 [n, levels]), both on the device:
    error[i, l] = 1 where a code lay outside [0, k_l) or met an empty bin -- such a code adds nothing.  `out` / `error`: the caller's
    buffers, or fresh ones."""
    who = "code_bits"
    cs = [_dev(c.detach(), "codes", torch.int64) for c in codes]
    ts = [_dev(t, "cdf", torch.uint32) for t in cdfs]
    levels = len(cs)
    if levels == 0 or len(ts) != levels:
        raise ValueError(f"{who}: one code tensor and one table per level")
    n = int(cs[0].shape[0])
    for c, t in zip(cs, ts):
        if c.dim() != 4 or t.dim() != 2 or int(c.shape[0]) != n or int(c.shape[1]) != int(t.shape[0]) or int(t.shape[1]) < 2 or c.numel() == 0:
            raise ValueError(f"{who}: codes [n, m, h, w] need a table [m, k + 1] per level (got {tuple(c.shape)} and {tuple(t.shape)})")
        if c.device != cs[0].device or t.device != cs[0].device:
            raise ValueError(f"{who}: codes and tables must live on one device")
        if c[0].numel() > _lib.MCQ_CODE_BITS_MAX_SYMBOLS:
            raise ValueError(f"{who}: more than 2^30 codes per image and level")
    dev = cs[0].device
    if out is None:
        out = torch.empty((n, levels), dtype=torch.float64, device=dev)
    if error is None:
        error = torch.empty((n, levels), dtype=torch.int32, device=dev)
    for t, dt, name in ((out, torch.float64, "out"), (error, torch.int32, "error")):
        if not (t.is_cuda and t.device == dev and t.dtype == dt and tuple(t.shape) == (n, levels) and t.is_contiguous()):
            raise ValueError(f"{who}: `{name}` must be a contiguous {dt} [{n}, {levels}] tensor on {dev} (it is written in place)")
    lib = _lib.load()
    cap = int(lib.mcq_vq_max_levels())
    with _guard(dev):
        for l0 in range(0, levels, cap):
            sl = slice(l0, min(levels, l0 + cap))
            nl = sl.stop - l0
            check(lib.mcq_code_bits((ctypes.c_void_p * nl)(*[c.data_ptr() for c in cs[sl]]), (ctypes.c_void_p * nl)(*[t.data_ptr() for t in ts[sl]]),
                                    (ctypes.c_int32 * nl)(*[int(c.shape[1]) for c in cs[sl]]),
                                    (ctypes.c_int32 * nl)(*[int(t.shape[1]) - 1 for t in ts[sl]]),
                                    (ctypes.c_int32 * nl)(*[int(c.shape[2]) * int(c.shape[3]) for c in cs[sl]]), nl, n, l0, levels,
                                    _ptr(out), _ptr(error), _stream()), "mcq_code_bits")
    return out, error


# ---- the rANS coder on the device (csrc/rans_dev.hip): byte streams from codes and back, nothing through the host -------------------
RANS_OK, RANS_BAD_SYMBOL, RANS_BAD_STREAM = _lib.MCQ_RANS_OK, _lib.MCQ_RANS_BAD_SYMBOL, _lib.MCQ_RANS_BAD_STREAM      # the status words
RANS_DEV_CHUNK = _lib.MCQ_RANS_DEV_CHUNK                # symbols (and stream words) the kernels hold in LDS at a time


class RansEncoded(tuple):
    """What `rans_encode_dev` returns: the tuple (blob, offsets, status), and behind it the buffers a later call reuses when it is
    handed back as `out` -- `sizes` (int64 [n * levels], the coded bytes per stream, image-major), `scratch` (the kernels' [streams, cap]
    slots) and `meta`, the ONE allocation that `offsets`, `sizes` and `status` are views of (so one copy takes all three to the host)."""

    def __new__(cls, blob, offsets, status, sizes, scratch, meta, key):
        self = super().__new__(cls, (blob, offsets, status))
        self.sizes, self.scratch, self.meta, self.key = sizes, scratch, meta, key
        return self

    blob = property(lambda self: self[0])
    offsets = property(lambda self: self[1])
    status = property(lambda self: self[2])

    @staticmethod
    def meta_words(streams: int) -> int:
        return 2 * streams + 1 + (streams + 1) // 2

    @staticmethod
    def split(meta: torch.Tensor, streams: int):
        """(offsets int64 [streams + 1], sizes int64 [streams], status int32 [streams]) as views of `meta` (int64 [meta_words(streams)]),
        on whichever side it lives."""
        return meta[:streams + 1], meta[streams + 1:2 * streams + 1], meta[2 * streams + 1:].view(torch.int32)[:streams]


def _rans_levels(codes_shapes, ts, who: str):
    """(n, [m_l], [k_l], [h_l w_l]) of a batch's levels against their tables, checked as the launchers check them."""
    n = int(codes_shapes[0][0])
    kmax = _lib.MCQ_CDF_MAX_K
    for shp, t in zip(codes_shapes, ts):
        if len(shp) != 4 or t.dim() != 2 or int(shp[0]) != n or int(shp[1]) != int(t.shape[0]) or int(t.shape[1]) < 2 or min(int(v) for v in shp) < 1:
            raise ValueError(f"{who}: codes [n, m, h, w] need a table [m, k + 1] per level (got {tuple(shp)} and {tuple(t.shape)})")
        if t.device != ts[0].device:
            raise ValueError(f"{who}: codes and tables must live on one device")
        if int(t.shape[1]) - 1 > kmax:
            raise ValueError(f"{who}: a table of {int(t.shape[1]) - 1} symbols does not fit the decoder's LDS array (at most {kmax})")
        if int(shp[1]) * int(shp[2]) * int(shp[3]) > _lib.MCQ_RANS_DEV_MAX_SYMBOLS:
            raise ValueError(f"{who}: more than 2^28 codes per image and level")
    if n > 65535:
        raise ValueError(f"{who}: more than 65535 images per call")
    return (n, [int(s[1]) for s in codes_shapes], [int(t.shape[1]) - 1 for t in ts], [int(s[2]) * int(s[3]) for s in codes_shapes])


RANS_LANES_MAX = _lib.MCQ_RANS_LANES_MAX                 # the widest lanes stream: one state per lane of a wave
RANS_LANES_HEAD = 4 * (1 + 2 * RANS_LANES_MAX)          # bytes of prefix and state words at that width


def rans_lanes_widths(lanes, levels: int, who: str = "lanes"):
    """A `lanes` argument as one int per level for the C ABI: "auto" -> 0 (the library's rule, `mcq_rans_lanes_auto`), a power of two
    <= RANS_LANES_MAX -> itself, a sequence -> one of either per level.  None / False (the plain layout) is not a width."""
    per = list(lanes) if isinstance(lanes, (list, tuple)) else [lanes] * levels
    if len(per) != levels:
        raise ValueError(f"{who}: one lanes entry per level ({levels}), got {len(per)}")
    out = []
    for w in per:
        if isinstance(w, str) and w == "auto":
            out.append(0)
        elif isinstance(w, int) and not isinstance(w, bool) and 1 <= w <= RANS_LANES_MAX and w & (w - 1) == 0:
            out.append(int(w))
        else:
            raise ValueError(f"{who}: lanes must be 'auto' or a power of two <= {RANS_LANES_MAX}, got {w!r}")
    return out


def rans_encode_dev(codes: Sequence[torch.Tensor], cdfs: Sequence[torch.Tensor], out: Optional[RansEncoded] = None, lanes=None) -> RansEncoded:
    """The coder's byte streams made on the device (mcq_rans_encode_dev + mcq_rans_pack_dev: three launches for all levels and images,
    nothing read by the host, so the call captures): `codes[l]` int64 [n, m_l, h_l, w_l] under `cdfs[l]` uint32 [m_l, k_l + 1] (the
    tables of `pmf_to_quantized_cdf_dev`) -> (blob, offsets, status).  Stream s = i * levels + l (image-major) is
    blob[offsets[s] : offsets[s + 1]], byte for byte what the host coder writes for `codes[l][i].flatten()` with the group index
    selecting the table; `blob` uint8 is allocated at the worst case, 4 (symbols + 2) bytes per stream, and only offsets[-1] bytes
    of it mean anything.  `status` int32 [n * levels]: RANS_OK, or RANS_BAD_SYMBOL where a code lay outside [0, k_l) or met an empty
    bin -- the host coder's RuntimeError -- and then the stream's size is 0.  The bypass digits of the host coder are not implemented:
    no code in [0, k) reaches them.  `out`: the result of an earlier call with codes of these shapes (its buffers are written in place:
    a captured launch keeps their addresses), or None for fresh ones.
    `lanes`: None for the layout above; "auto", a power of two <= 64, or one of either per level for the lane-interleaved layout
    (mcq_rans_lanes_encode_dev, csrc/rans_lanes.hip: one wave per stream, the same pack launches) -- byte for byte the host lanes coder's
    streams; the blob's worst case is then 4 (1 + 2 * 64) bytes per stream larger.  `out` must come from a call of the same layout."""
    who = "rans_encode_dev"
    widths = None if lanes is None else rans_lanes_widths(lanes, len(codes), who)
    cs = [_dev(c.detach(), "codes", torch.int64) for c in codes]
    ts = [_dev(t, "cdf", torch.uint32) for t in cdfs]
    levels = len(cs)
    if levels == 0 or len(ts) != levels:
        raise ValueError(f"{who}: one code tensor and one table per level")
    dev = cs[0].device
    if any(c.device != dev for c in cs) or ts[0].device != dev:
        raise ValueError(f"{who}: codes and tables must live on one device")
    n, ms, ks, hws = _rans_levels([tuple(c.shape) for c in cs], ts, who)
    counts = [m * hw for m, hw in zip(ms, hws)]
    streams = n * levels
    head = 0 if widths is None else RANS_LANES_HEAD          # a lanes stream's prefix and state words at the widest W
    cap = 4 * max(counts) + 64 + head                        # per-stream slot, the host coder's own allowance (4 (count + 2) is the bound)
    key = (n, tuple(tuple(c.shape[1:]) for c in cs), dev) + (() if widths is None else ("lanes",))
    if out is None:
        meta = torch.empty(RansEncoded.meta_words(streams), dtype=torch.int64, device=dev)
        offsets, sizes, status = RansEncoded.split(meta, streams)
        out = RansEncoded(torch.empty(n * sum(4 * c + 8 + head for c in counts), dtype=torch.uint8, device=dev), offsets, status, sizes,
                          torch.empty(streams * cap, dtype=torch.uint8, device=dev), meta, key)
    elif not isinstance(out, RansEncoded) or out.key != key:
        raise ValueError(f"{who}: `out` must be the result of an earlier call with codes of these shapes on {dev} (it is written in place)")
    lib = _lib.load()
    limit = int(lib.mcq_vq_max_levels())
    with _guard(dev):
        for l0 in range(0, levels, limit):
            sl = slice(l0, min(levels, l0 + limit))
            nl = sl.stop - l0
            if widths is not None:
                check(lib.mcq_rans_lanes_encode_dev((ctypes.c_void_p * nl)(*[c.data_ptr() for c in cs[sl]]),
                                                    (ctypes.c_void_p * nl)(*[t.data_ptr() for t in ts[sl]]), (ctypes.c_int32 * nl)(*ms[sl]),
                                                    (ctypes.c_int32 * nl)(*ks[sl]), (ctypes.c_int32 * nl)(*hws[sl]), (ctypes.c_int32 * nl)(*widths[sl]),
                                                    nl, n, l0, levels, _ptr(out.scratch), cap, _ptr(out.sizes), _ptr(out.status), _stream()),
                      "mcq_rans_lanes_encode_dev")
                continue
            check(lib.mcq_rans_encode_dev((ctypes.c_void_p * nl)(*[c.data_ptr() for c in cs[sl]]), (ctypes.c_void_p * nl)(*[t.data_ptr() for t in ts[sl]]),
                                          (ctypes.c_int32 * nl)(*ms[sl]), (ctypes.c_int32 * nl)(*ks[sl]), (ctypes.c_int32 * nl)(*hws[sl]), nl, n, l0,
                                          levels, _ptr(out.scratch), cap, _ptr(out.sizes), _ptr(out.status), _stream()), "mcq_rans_encode_dev")
        check(lib.mcq_rans_pack_dev(_ptr(out.scratch), cap, _ptr(out.sizes), streams, _ptr(out.blob), out.blob.numel(), _ptr(out.offsets),
                                    _stream()), "mcq_rans_pack_dev")
    return out


def rans_decode_dev(blob: torch.Tensor, offsets: torch.Tensor, cdfs: Sequence[torch.Tensor], shapes: Sequence[Sequence[int]], out=None, lanes: bool = False):
    """The inverse, in ONE launch (mcq_rans_decode_dev): stream s = i * levels + l is blob[offsets[s] : offsets[s + 1]] (`blob` uint8,
    `offsets` int64 [n * levels + 1], both on the device) and decodes under `cdfs[l]` straight into int64 [n, m_l, h_l, w_l] --
    `shapes[l]`.  Returns (codes, status): `status` int32 [n * levels] is RANS_OK, or RANS_BAD_STREAM for a stream that is shorter than 8
    bytes, not a multiple of 4 long, lies outside the blob, or runs out of words -- the host coder's "truncated or malformed" -- and
    that stream's codes are ZERO; the others decode.  The streams are untrusted input and no content of `blob` or `offsets` leads to a
    read outside them.  `out`: the (codes, status) of an earlier call with these shapes, written in place, or None for fresh ones.
    `lanes`: True when the streams are lane-interleaved (mcq_rans_lanes_decode_dev): each stream's width comes from its own prefix, and
    a stream without that prefix -- a plain one among them -- is RANS_BAD_STREAM like any other malformed stream."""
    who = "rans_decode_dev"
    blob = _dev(blob, "blob", torch.uint8)
    offsets = _dev(offsets, "offsets", torch.int64)
    ts = [_dev(t, "cdf", torch.uint32) for t in cdfs]
    shapes = [tuple(int(v) for v in s) for s in shapes]
    levels = len(shapes)
    if levels == 0 or len(ts) != levels:
        raise ValueError(f"{who}: one shape and one table per level")
    dev = blob.device
    if offsets.device != dev or ts[0].device != dev:
        raise ValueError(f"{who}: the blob, its offsets and the tables must live on one device")
    n, ms, ks, hws = _rans_levels(shapes, ts, who)
    streams = n * levels
    if blob.dim() != 1 or offsets.dim() != 1 or offsets.numel() != streams + 1:
        raise ValueError(f"{who}: a flat uint8 blob and {streams + 1} int64 offsets (n * levels + 1) expected")
    nbytes = blob.numel()
    if nbytes == 0:                                          # (an empty blob still needs an address; every stream is refused)
        blob = blob.new_zeros(4)
    if out is None:
        out = ([torch.empty(s, dtype=torch.int64, device=dev) for s in shapes], torch.empty(streams, dtype=torch.int32, device=dev))
    codes, status = _reassign_rows(out[0], shapes, torch.int64, dev, "out", who), out[1]
    if not (status.is_cuda and status.device == dev and status.dtype == torch.int32 and status.numel() == streams and status.is_contiguous()):
        raise ValueError(f"{who}: `out`'s status must be {streams} contiguous int32 words on {dev} (written in place)")
    lib = _lib.load()
    limit = int(lib.mcq_vq_max_levels())
    with _guard(dev):
        for l0 in range(0, levels, limit):
            sl = slice(l0, min(levels, l0 + limit))
            nl = sl.stop - l0
            entry = "mcq_rans_lanes_decode_dev" if lanes else "mcq_rans_decode_dev"       # (one argument list for both)
            check(getattr(lib, entry)(_ptr(blob), nbytes, _ptr(offsets), (ctypes.c_void_p * nl)(*[t.data_ptr() for t in ts[sl]]),
                                      (ctypes.c_int32 * nl)(*ms[sl]), (ctypes.c_int32 * nl)(*ks[sl]), (ctypes.c_int32 * nl)(*hws[sl]), nl, n, l0,
                                      levels, (ctypes.c_void_p * nl)(*[c.data_ptr() for c in codes[sl]]), _ptr(status), _stream()), entry)
    return codes, status


def hash_uniform(rng: torch.Tensor, stream_id: int, shape) -> torch.Tensor:
    """The generator's draws for a tensor of `shape` (stream 0 = random drop, 1 = Gumbel noise) under the snapshot `rng`:
    exactly what the kernels use in place of a missing u_drop / u_gumbel (mcq_hash_uniform_f32)."""
    rng = _dev(rng, "rng", torch.int64)
    out = torch.empty(tuple(shape), dtype=torch.float32, device=rng.device)
    with _guard(rng.device):
        check(_lib.load().mcq_hash_uniform_f32(_ptr(rng), int(stream_id), _ptr(out), out.numel(), _stream()), "mcq_hash_uniform_f32")
    return out


# ---- k-means on the device (csrc/vq_kmeans.hip): what turns ops.vq_assign's codes into new codewords -------------------------------
class KMeansAcc:
    """The running accumulators of one level's Lloyd iteration: `sums` float64 [m, k, d], `sqsums` float64 [m, k] and `counts`
    int64 [m, k], one allocation each, zeroed at construction and by `zero_()` (mcq_vq_kmeans_zero: a kernel, not a memset)."""

    __slots__ = ("sums", "sqsums", "counts", "m", "k", "d")

    def __init__(self, m: int, k: int, d: int, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"mcquic_amd: KMeansAcc must live on a HIP device (got {device}); the HIP kernels have no CPU fallback")
        self.m, self.k, self.d = int(m), int(k), int(d)
        self.sums = torch.empty((self.m, self.k, self.d), dtype=torch.float64, device=device)
        self.sqsums = torch.empty((self.m, self.k), dtype=torch.float64, device=device)
        self.counts = torch.empty((self.m, self.k), dtype=torch.int64, device=device)
        self.zero_()

    def zero_(self) -> "KMeansAcc":
        with _guard(self.sums.device):
            check(_lib.load().mcq_vq_kmeans_zero(_ptr(self.sums), _ptr(self.sqsums), _ptr(self.counts), self.m, self.k, self.d, _stream()),
                  "mcq_vq_kmeans_zero")
        return self


def _kmeans_latent(x: torch.Tensor, m: int, d: int) -> torch.Tensor:
    x = _dev(x, "x")
    if x.dim() != 4 or x.shape[1] != m * d:
        raise ValueError(f"latent must be [n, {m}*{d}, h, w], got {tuple(x.shape)}")
    return x


def _kmeans_codebook(codebook: torch.Tensor) -> torch.Tensor:
    cb = _dev(codebook, "codebook")
    if cb.dim() != 3 or cb.data_ptr() != codebook.data_ptr():
        raise ValueError("codebook must be a contiguous [m, k, d] tensor (it is written in place)")
    return cb


def vq_kmeans_accumulate(x: torch.Tensor, codes: torch.Tensor, acc: KMeansAcc) -> None:
    """Adds one batch onto `acc`: per codeword the sum of the latent vectors `x` [n, m*d, h, w] whose code (`codes` int64
    [n, m, h, w], ops.vq_assign's layout) it is, the sum of their squared norms and their number; codes outside [0, k) are skipped.
    No atomics, one fixed order per sum: bit-reproducible (mcq_vq_kmeans_accumulate_f32)."""
    x = _kmeans_latent(x, acc.m, acc.d)
    codes = _dev(codes, "codes", torch.int64)
    n, _, h, w = x.shape
    if tuple(codes.shape) != (n, acc.m, h, w):
        raise ValueError(f"codes must be [{n}, {acc.m}, {h}, {w}], got {tuple(codes.shape)}")
    with _guard(x.device):
        check(_lib.load().mcq_vq_kmeans_accumulate_f32(_ptr(x), _ptr(codes), _ptr(acc.sums), _ptr(acc.sqsums), _ptr(acc.counts), n, acc.m,
                                                       acc.d, h, w, acc.k, _stream()), "mcq_vq_kmeans_accumulate_f32")


def vq_kmeans_update(codebook: torch.Tensor, acc: KMeansAcc):
    """In place on `codebook` [m, k, d]: the mean of every codeword that was assigned a vector; the others stay as they are.
    Returns (inertia float64 [m] against the old codewords, empty int64 [m] = codewords left untouched), both on the device
    (mcq_vq_kmeans_update_f32).  The caller tells whoever caches the codebook (`_multiCodebookQuantization._store`)."""
    cb = _kmeans_codebook(codebook)
    if tuple(cb.shape) != (acc.m, acc.k, acc.d):
        raise ValueError(f"codebook must be [{acc.m}, {acc.k}, {acc.d}], got {tuple(cb.shape)}")
    inertia = torch.empty(acc.m, dtype=torch.float64, device=cb.device)
    empty = torch.empty(acc.m, dtype=torch.int64, device=cb.device)
    with _guard(cb.device):
        check(_lib.load().mcq_vq_kmeans_update_f32(_ptr(cb), _ptr(acc.sums), _ptr(acc.sqsums), _ptr(acc.counts), _ptr(inertia), _ptr(empty),
                                                   acc.m, acc.k, acc.d, _stream()), "mcq_vq_kmeans_update_f32")
    return inertia, empty


def vq_kmeans_seed(x: torch.Tensor, codebook: torch.Tensor, rng: torch.Tensor, counts: Optional[torch.Tensor] = None) -> None:
    """In place on `codebook` [m, k, d]: codeword (g, c) becomes latent vector min(V - 1, floor(u V)) of group g of `x`, u =
    hash_uniform(rng, 2, (m, k))[g, c] -- every codeword (`counts` None), or those with counts[g, c] == 0.  `rng` is a {seed, offset}
    int64[2] device tensor; the caller moves its offset on between calls (mcq_vq_kmeans_seed_f32)."""
    cb = _kmeans_codebook(codebook)
    m, k, d = cb.shape
    x = _kmeans_latent(x, m, d)
    rng = _dev(rng, "rng", torch.int64)
    if counts is not None:
        counts = _dev(counts, "counts", torch.int64)
        if counts.numel() != m * k:
            raise ValueError("vq_kmeans_seed: `counts` must hold m * k entries")
    n, _, h, w = x.shape
    with _guard(x.device):
        check(_lib.load().mcq_vq_kmeans_seed_f32(_ptr(x), _ptr(cb), _ptr(counts), _ptr(rng), n, m, d, h, w, k, _stream()),
              "mcq_vq_kmeans_seed_f32")


def vq_gumbel_sample(logits: torch.Tensor, u_drop: Optional[torch.Tensor], u_gumbel: Optional[torch.Tensor], freq_ema: torch.Tensor,
                     drop_exponent: torch.Tensor, rng: Optional[torch.Tensor] = None, counts: Optional[torch.Tensor] = None):
    """In place on `logits`: random drop; returns (codes, sample_index, sample_hot), each [n, m, h, w].  A draw that is None is
    made inside the kernel from the generator snapshot `rng` (rng_snapshot).  `counts` (int64 [m * k], zeroed by the caller once
    per step): every code made here is counted into it -- the level's histogram for the frequency EMA."""
    logits = _dev(logits, "logits")
    n, m, h, w, k = logits.shape
    if (u_drop is None or u_gumbel is None) and rng is None:
        raise ValueError("vq_gumbel_sample: give both uniform draws or a generator snapshot")
    u_drop = None if u_drop is None else _dev(u_drop, "u_drop")
    u_gumbel = None if u_gumbel is None else _dev(u_gumbel, "u_gumbel")
    rng = None if rng is None else _dev(rng, "rng", torch.int64)
    if any(u is not None and u.shape != logits.shape for u in (u_drop, u_gumbel)):
        raise ValueError("uniform draws must have the logits' shape")
    freq = _dev(freq_ema.detach(), "freq_ema")
    expo = _dev(drop_exponent.detach().reshape(1), "drop_exponent")
    codes = torch.empty((n, m, h, w), dtype=torch.int64, device=logits.device)
    index = torch.empty_like(codes)
    hot = torch.empty((n, m, h, w), dtype=torch.float32, device=logits.device)
    if counts is not None:
        counts = _dev(counts, "counts", torch.int64)
        if counts.numel() != m * k:
            raise ValueError("vq_gumbel_sample: `counts` must hold m * k entries")
    with _guard(logits.device):
        check(_lib.load().mcq_vq_gumbel_sample_f32(_ptr(logits), _ptr(u_drop), _ptr(u_gumbel), _ptr(rng), _ptr(freq), _ptr(expo), _ptr(codes),
                                                   _ptr(index), _ptr(hot), _ptr(counts), n, m, h, w, k, _stream()), "mcq_vq_gumbel_sample_f32")
    return codes, index, hot


def vq_dequant_soft(index: torch.Tensor, hot: torch.Tensor, cb: PackedCodebook, dual_silu: bool = False) -> torch.Tensor:
    """sample @ codebook for the one-hot-valued straight-through sample -> [n, m*d, h, w] (`dual_silu`: + its SiLU twin)."""
    index = _dev(index, "sample_index", torch.int64)
    hot = _dev(hot, "sample_hot")
    n, m, h, w = index.shape
    out = torch.empty((n, m * cb.d, h, w), dtype=torch.float32, device=index.device)
    out2 = torch.empty_like(out) if dual_silu else None
    with _guard(index.device):
        check(_lib.load().mcq_vq_dequant_soft_f32(_ptr(index), _ptr(hot), _ptr(cb.codebook), _ptr(out), _ptr(out2), n, m, cb.d, h, w, cb.k,
                                                  _stream()), "mcq_vq_dequant_soft_f32")
    if out2 is not None:
        set_silu_twin(out, out2)
    return out


def add(a: torch.Tensor, b: torch.Tensor, dual_silu: bool = False) -> torch.Tensor:
    a, b = _dev16(a, "a"), _dev16(b, "b")
    if a.shape != b.shape:
        raise ValueError("add: shape mismatch")
    out = torch.empty_like(a)
    out2 = torch.empty_like(a) if dual_silu else None
    with _guard(a.device):
        check(_lib.load().mcq_add_f32(_ptr(a), _ptr(b), _ptr(out), _ptr(out2), a.numel(), _stream()), "mcq_add_f32")
    if out2 is not None:
        set_silu_twin(out, out2)
    return out


def add3(a: torch.Tensor, b: torch.Tensor, c: torch.Tensor) -> torch.Tensor:
    """(a + b) + c in one launch (mcq_add3_f32)."""
    a, b, c = _dev16(a, "a"), _dev16(b, "b"), _dev16(c, "c")
    if a.shape != b.shape or a.shape != c.shape:
        raise ValueError("add3: shape mismatch")
    out = torch.empty_like(a)
    with _guard(a.device):
        check(_lib.load().mcq_add3_f32(_ptr(a), _ptr(b), _ptr(c), _ptr(out), a.numel(), _stream()), "mcq_add3_f32")
    return out


def mse(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """mean((a - b)^2) as a 0-dim tensor (mcq_mse_f32: two launches, fixed summation order, no memset -- see csrc/train_ops.hip)."""
    a, b = _dev(a, "a"), _dev(b, "b")
    if a.shape != b.shape or a.numel() == 0:
        raise ValueError("mse: shape mismatch or empty input")
    lib = _lib.load()
    out = torch.empty((), dtype=torch.float32, device=a.device)
    ws = torch.empty(lib.mcq_mse_workspace_bytes(a.numel()) // 8, dtype=torch.float64, device=a.device)
    with _guard(a.device):
        check(lib.mcq_mse_f32(_ptr(a), _ptr(b), _ptr(out), _ptr(ws), a.numel(), _stream()), "mcq_mse_f32")
    return out


def mse_bwd(a: torch.Tensor, b: torch.Tensor, dloss: torch.Tensor, want_db: bool = False):
    """(da, db or None) of `mse`: da = 2 (a - b) / n * dloss (mcq_mse_bwd_f32); `dloss` stays on the device."""
    a, b, dloss = _dev(a, "a"), _dev(b, "b"), _dev(dloss, "dloss")
    da = torch.empty_like(a)
    db = torch.empty_like(a) if want_db else None
    with _guard(a.device):
        check(_lib.load().mcq_mse_bwd_f32(_ptr(a), _ptr(b), _ptr(dloss), _ptr(da), _ptr(db) if want_db else None, a.numel(), _stream()),
              "mcq_mse_bwd_f32")
    return da, db


def sumsq(x: torch.Tensor) -> torch.Tensor:
    """sum(x^2) as a 0-dim float32 tensor (mcq_sumsq_f32: double partials, fixed order, no memset)."""
    x = _dev(x, "x")
    lib = _lib.load()
    out = torch.empty((), dtype=torch.float32, device=x.device)
    ws = torch.empty(lib.mcq_mse_workspace_bytes(x.numel()) // 8, dtype=torch.float64, device=x.device)
    with _guard(x.device):
        check(lib.mcq_sumsq_f32(_ptr(x), _ptr(out), _ptr(ws), x.numel(), _stream()), "mcq_sumsq_f32")
    return out


def _cosine_codebook(codebook: torch.Tensor):
    codebook = _dev(codebook, "codebook")
    if codebook.dim() != 3 or codebook.numel() == 0:
        raise ValueError(f"expected a non-empty [m, k, d] codebook, got {tuple(codebook.shape)}")
    m, k, d = codebook.shape
    nbytes = _lib.load().mcq_codebook_cos_workspace(m, k, d)
    if nbytes == 0:
        raise ValueError(f"codebook_cosine: [m, k, d] = {(m, k, d)} is not taken (1 <= d <= 256, m * k below 2^31)")
    return codebook, torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=codebook.device)


def codebook_cosine(codebook: torch.Tensor) -> torch.Tensor:
    """Sum over the groups of a [m, k, d] codebook and the pairs i < j of clamp(cos(c_i, c_j), 0, 2) as a 0-dim float32 tensor
    (mcquic/loss/__init__.py:32-41 without the [k, k] plane; mcq_codebook_cos_f32: fixed summation order, no memset)."""
    codebook, ws = _cosine_codebook(codebook)
    m, k, d = codebook.shape
    out = torch.empty((), dtype=torch.float32, device=codebook.device)
    with _guard(codebook.device):
        check(_lib.load().mcq_codebook_cos_f32(_ptr(codebook), _ptr(out), _ptr(ws), m, k, d, _stream()), "mcq_codebook_cos_f32")
    return out


def codebook_cosine_bwd(codebook: torch.Tensor, dout: torch.Tensor, gamma: float) -> torch.Tensor:
    """Gradient [m, k, d] of `gamma * codebook_cosine(codebook)` times the device scalar `dout` (mcq_codebook_cos_bwd_f32: the
    tiles are recomputed, every element has one writer)."""
    codebook, ws = _cosine_codebook(codebook)
    dout = _dev(dout, "dout")
    if dout.numel() != 1:
        raise ValueError("codebook_cosine_bwd: `dout` must hold one element")
    m, k, d = codebook.shape
    out = torch.empty_like(codebook)
    with _guard(codebook.device):
        check(_lib.load().mcq_codebook_cos_bwd_f32(_ptr(codebook), _ptr(dout), float(gamma), _ptr(out), _ptr(ws), m, k, d, _stream()),
              "mcq_codebook_cos_bwd_f32")
    return out


def clip_by_norm_(x: torch.Tensor, max_norm: float, eps: float = 1e-6, sq: Optional[torch.Tensor] = None, skip=None) -> torch.Tensor:
    """In place: x *= max_norm / (||x|| + eps) where that is < 1 (torch.nn.utils.clip_grad_norm_ over one flat buffer; the reference's
    trainer.py:280).  Returns ||x|| BEFORE clipping as a 0-dim device tensor; no host read, so it can be captured.
    `sq`: `sumsq(x)` where the caller has formed it already (a step's guard decides from it in between); `skip`: that guard's flag
    (one int32 on the device, `guard.StepGuard.skip`): set on the device, the factor is not applied (the norm is still returned)."""
    x = _dev(x, "x")
    if not x.is_contiguous():
        raise ValueError("clip_by_norm_: needs a contiguous buffer (it is scaled in place)")
    sq = sumsq(x) if sq is None else _dev(sq, "sq")
    norm = torch.empty((), dtype=torch.float32, device=x.device)
    from .guard import skip_pointer
    flag = skip_pointer(skip, x.device, "clip_by_norm_")
    with _guard(x.device):
        check(_lib.load().mcq_clip_by_norm_skip_f32(_ptr(x), _ptr(sq), float(max_norm), float(eps), _ptr(norm), x.numel(), flag, _stream()),
              "mcq_clip_by_norm_skip_f32")
    return norm


def _phase_word(phase: torch.Tensor, k: int, what: str) -> torch.Tensor:
    if not isinstance(k, int) or isinstance(k, bool) or k < 2:
        raise ValueError(f"{what}: k must be an int >= 2 (one micro-step is the plain copy)")
    phase = _dev(phase, "phase", torch.int32)
    if phase.numel() != 1:
        raise ValueError(f"{what}: `phase` is one int32 on the device")
    return phase


def gather_accum_flat_(ptrs: torch.Tensor, flat: torch.Tensor, offsets: torch.Tensor, table, phase: torch.Tensor, k: int) -> None:
    """Micro-step `phase` of k into `flat` (mcq_gather_accum_flat_f32): per element flat = src at phase 0, flat + src afterwards, and
    (flat + src) * float32(1 / k) at phase k - 1, all in float32.  `ptrs` / `offsets`: int64 device arrays of the sources' addresses and
    of their offsets into `flat` (floats); `table`: their `tensor_list.ChunkTable`; `phase`: one device int32, read by the launch."""
    phase = _phase_word(phase, k, "gather_accum_flat_")
    if not flat.is_contiguous():
        raise ValueError("gather_accum_flat_: needs a contiguous buffer (it is accumulated in place)")
    flat = _dev(flat, "flat")
    ptrs, offsets = _dev(ptrs, "ptrs", torch.int64), _dev(offsets, "offsets", torch.int64)
    with _guard(flat.device):
        check(_lib.load().mcq_gather_accum_flat_f32(_ptr(ptrs), _ptr(flat), _ptr(offsets), _ptr(table.numel), _ptr(table.blk_tensor),
                                                    _ptr(table.blk_first), table.nblocks, _ptr(phase), k, _stream()), "mcq_gather_accum_flat_f32")


def accum_step_scalars_(counts: Optional[torch.Tensor], counts_acc: Optional[torch.Tensor], loss: Optional[torch.Tensor],
                        loss_acc: Optional[torch.Tensor], phase: torch.Tensor, k: int) -> None:
    """The scalars of micro-step `phase` of k in one launch (mcq_accum_step_scalars): the int64 code counts into `counts_acc` (overwritten
    at phase 0, added to afterwards: exact), the 0-dim float32 `loss` into `loss_acc` by `gather_accum_flat_`'s rule (the mean of the k
    losses after the last phase).  Either pair may be None."""
    phase = _phase_word(phase, k, "accum_step_scalars_")
    n = 0
    if counts is not None or counts_acc is not None:
        if counts is None or counts_acc is None or counts.numel() != counts_acc.numel() or counts.numel() == 0 or not counts_acc.is_contiguous():
            raise ValueError("accum_step_scalars_: `counts` and the contiguous `counts_acc` hold the same number of entries (not none)")
        counts, counts_acc = _dev(counts, "counts", torch.int64), _dev(counts_acc, "counts_acc", torch.int64)
        n = counts.numel()
    if loss is not None or loss_acc is not None:
        if loss is None or loss_acc is None or loss.numel() != 1 or loss_acc.numel() != 1:
            raise ValueError("accum_step_scalars_: `loss` and `loss_acc` hold one float32 each")
        loss, loss_acc = _dev(loss, "loss"), _dev(loss_acc, "loss_acc")
    with _guard(phase.device):
        check(_lib.load().mcq_accum_step_scalars(_ptr(counts), _ptr(counts_acc), n, _ptr(loss), _ptr(loss_acc), _ptr(phase), k, _stream()),
              "mcq_accum_step_scalars")


def group_norm(x: torch.Tensor, weight: Optional[torch.Tensor], bias: Optional[torch.Tensor], groups: int, eps: float = 1e-5,
               dual_silu: bool = False, want_stats: bool = False):
    """nn.GroupNorm(groups, C) on [n, C, h, w] (mcq_group_norm_f32; `denseNorm=True`, mcquic/nn/blocks.py:179-200).
    With `want_stats` returns (y, mean, rstd), the per-(image, group) statistics the backward pass needs."""
    x = _dev(x, "x")
    n, c, h, w = x.shape
    if c % groups != 0:
        raise ValueError(f"GroupNorm: {c} channels do not divide into {groups} groups")
    weight = None if weight is None else _dev(weight.detach(), "weight")
    bias = None if bias is None else _dev(bias.detach(), "bias")
    y = torch.empty_like(x)
    y2 = torch.empty_like(x) if dual_silu else None
    mean = torch.empty(n * groups, dtype=torch.float32, device=x.device) if want_stats else None
    rstd = torch.empty_like(mean) if want_stats else None
    lib = _lib.load()
    nws = lib.mcq_group_norm_workspace_floats(n, c, h * w, groups)       # > 0: large runs, many workgroups per (image, group)
    ws = torch.empty(nws, dtype=torch.float32, device=x.device) if nws else None
    with _guard(x.device):
        check(lib.mcq_group_norm_f32(_ptr(x), _ptr(weight), _ptr(bias), _ptr(y), _ptr(y2), _ptr(mean), _ptr(rstd), _ptr(ws), n, c, h * w,
                                     groups, float(eps), _stream()), "mcq_group_norm_f32")
    if y2 is not None:
        set_silu_twin(y, y2)
    return (y, mean, rstd) if want_stats else y


def group_norm_bwd(x: torch.Tensor, dy: torch.Tensor, weight: Optional[torch.Tensor], mean: torch.Tensor, rstd: torch.Tensor,
                   groups: int, want_params: bool = True):
    """(dx, dweight, dbias) of group_norm (mcq_group_norm_bwd_f32)."""
    x, dy = _dev(x, "x"), _dev(dy, "dy")
    n, c, h, w = x.shape
    weight = None if weight is None else _dev(weight.detach(), "weight")
    lib = _lib.load()
    ws = torch.empty(lib.mcq_group_norm_bwd_workspace_floats(n, c, h * w, groups), dtype=torch.float32, device=x.device)
    dx = torch.empty_like(x)
    dw = torch.empty(c, dtype=torch.float32, device=x.device) if want_params else None
    db = torch.empty(c, dtype=torch.float32, device=x.device) if want_params else None
    with _guard(x.device):
        check(lib.mcq_group_norm_bwd_f32(_ptr(x), _ptr(dy), _ptr(weight), _ptr(mean), _ptr(rstd), _ptr(dx), _ptr(dw), _ptr(db), _ptr(ws),
                                         n, c, h * w, groups, _stream()), "mcq_group_norm_bwd_f32")
    return dx, dw, db


def detransform(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[-1, 1] fp32 -> uint8 (mcquic/utils/vision.py:143-146).  `out`: a contiguous uint8 tensor of x's size on x's device to write
    into (nothing is allocated then)."""
    x = _dev(x, "x")
    if out is None:
        out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    elif out.dtype != torch.uint8 or out.device != x.device or out.numel() != x.numel() or not out.is_contiguous():
        raise ValueError(f"mcquic_amd: `out` must be {x.numel()} contiguous uint8 values on {x.device}")
    with _guard(x.device):
        check(_lib.load().mcq_detransform_u8(_ptr(x), _ptr(out), x.numel(), _stream()), "mcq_detransform_u8")
    return out


# ---- the trainer's log payload (csrc/step_snapshot.hip; gathered by monitor.StepSnapshot) ------------------------------------------
HIST_IDENTITY, HIST_LOG_DISTANCE = 0, 1
HIST_MAX_BINS = 4096


def histogram(x: torch.Tensor, bins: int = 64, transform: int = HIST_IDENTITY, eps: float = 1e-6):
    """`np.histogram(v, bins)` of a float32 device tensor, v = x or (`HIST_LOG_DISTANCE`) `(-x).clamp(eps).log10()` evaluated in
    registers: (counts int64 [bins], edges float64 [bins + 1], stats int64 [2]: finite, non-finite values) as device tensors.  The
    edges and the bin index are numpy's in float64 (include/mcquic_hip.h has the statement); non-finite values are counted in
    `stats[1]` and left out, where numpy raises.  Nothing is read by the host."""
    x = _dev(x, "x")
    n, bins = x.numel(), int(bins)
    lib = _lib.load()
    nbytes = int(lib.mcq_histogram_workspace_bytes(n, bins))
    if nbytes <= 0 or transform not in (HIST_IDENTITY, HIST_LOG_DISTANCE):
        raise ValueError(f"mcquic_amd.ops.histogram: n > 0, 1 <= bins <= {HIST_MAX_BINS} and a known transform are required "
                         f"(got n={n}, bins={bins}, transform={transform})")
    counts = torch.empty(bins, dtype=torch.int64, device=x.device)
    edges = torch.empty(bins + 1, dtype=torch.float64, device=x.device)
    stats = torch.empty(2, dtype=torch.int64, device=x.device)
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=x.device)
    with _guard(x.device):
        check(lib.mcq_histogram_f32(_ptr(x), n, int(transform), float(eps), bins, _ptr(counts), _ptr(edges), _ptr(stats), _ptr(ws), _stream()),
              "mcq_histogram_f32")
    return counts, edges, stats


def log_distance(x: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    """`(-x).clamp(eps).log10()` (mcquic/train/trainer.py:469), float32 op by op: what `histogram(..., HIST_LOG_DISTANCE)` bins."""
    x = _dev(x, "x")
    out = torch.empty_like(x)
    with _guard(x.device):
        check(_lib.load().mcq_log_distance_f32(_ptr(x), _ptr(out), x.numel(), float(eps), _stream()), "mcq_log_distance_f32")
    return out


def code_image(codes: torch.Tensor, keep: Optional[int] = None, out: Optional[torch.Tensor] = None,
               maxbuf: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`Validator.visualizeIntermediate` (mcquic/validate/validator.py:30-38): int64 codes [N, m, h, w] -> uint8 [N, 1, 4h, 4w], group 0
    scaled by the maximum over the WHOLE tensor, de-transformed and enlarged 4x (nearest).  `keep`: the first `keep` images only (the
    maximum is still the whole tensor's).  An all-zero tensor gives 0 (0 / 0 in the reference).  `out` / `maxbuf` (int64 [1]): buffers to
    write into, nothing is allocated then."""
    codes = _dev(codes, "codes", torch.int64)
    if codes.dim() != 4 or codes.numel() == 0:
        raise ValueError(f"mcquic_amd.ops.code_image: codes [N, m, h, w] are required (got {tuple(codes.shape)})")
    N, m, h, w = (int(s) for s in codes.shape)
    keep = N if keep is None else int(keep)
    if not 1 <= keep <= N:
        raise ValueError(f"mcquic_amd.ops.code_image: 1 <= keep <= {N} is required (got {keep})")
    if out is None:
        out = torch.empty((keep, 1, 4 * h, 4 * w), dtype=torch.uint8, device=codes.device)
    elif (out.dtype != torch.uint8 or out.device != codes.device or out.numel() != keep * 16 * h * w or not out.is_contiguous()
          or out.data_ptr() % 4):
        raise ValueError(f"mcquic_amd: `out` must be {keep * 16 * h * w} contiguous, 4-byte aligned uint8 values on {codes.device}")
    if maxbuf is None:
        maxbuf = torch.empty(1, dtype=torch.int64, device=codes.device)
    with _guard(codes.device):
        check(_lib.load().mcq_code_image_first_u8(_ptr(codes), _ptr(out), _ptr(maxbuf), N, m, h, w, keep, _stream()), "mcq_code_image_first_u8")
    return out


# ---- the training input transform (csrc/augment.hip) -----------------------------------------------------------------------------
# (the AUG_* columns, gamma modes and outputs of the decision table are the header's MCQ_AUG_*, imported from _lib above;
#  AUG_OUT_*: what follows the gains -- clamp + (v - 0.5) / 0.5, the clamp alone, neither)


def augment_identity_params(n: int, src_size, device=None) -> torch.Tensor:
    """The table under which `augment` only resamples the whole [Hs, Ws] source: no gamma, gains of 1, no flips, then clamp and (v - 0.5) / 0.5 (a CPU tensor
    unless `device` is given; a caller edits rows to fix decisions and moves it to the device)."""
    t = torch.zeros((int(n), AUG_COLUMNS), dtype=torch.float32)
    t[:, AUG_H], t[:, AUG_W] = float(src_size[0]), float(src_size[1])
    t[:, AUG_GAMMA_MODE] = float(AUG_GAMMA_IDENTITY)
    t[:, AUG_GAMMA] = t[:, AUG_GAIN0] = t[:, AUG_GAIN2] = 1.0
    t[:, AUG_GAIN_ROW] = -1.0
    return t if device is None else t.to(device)


def augment_draw(rng: torch.Tensor, n: int, src_size, crop=None, gamma: bool = False, coeffs: Optional[torch.Tensor] = None,
                 p_gain: float = 0.0, p_hflip: float = 0.0, p_vflip: float = 0.0, output: int = AUG_OUT_NORMALIZED) -> torch.Tensor:
    """The decisions of the training input transform for `n` images of a [Hs, Ws] source as a device table [n, 16] float32
    (mcq_augment_draw; columns AUG_*), drawn from `rng` = {seed, offset} (int64 [2] on the device), whose offset the launch
    advances in place -- captured in a hipGraph, every replay draws a fresh table.  `crop` = (scale, ratio) of torchvision's
    RandomResizedCrop or None (the whole source); `gamma`: draw one of RandomGamma's four modes; `coeffs` [T, 2]: with
    probability `p_gain` the gains of one row (RandomPlanckianJitter); `p_hflip` / `p_vflip`: the flips; `output`: AUG_OUT_*."""
    if not (torch.is_tensor(rng) and rng.is_cuda and rng.dtype == torch.int64 and rng.numel() == 2 and rng.is_contiguous()):
        raise TypeError("augment_draw: `rng` must be a contiguous int64 [2] tensor {seed, offset} on a HIP device (it is advanced in place)")
    hs, ws = int(src_size[0]), int(src_size[1])
    if n <= 0 or hs <= 0 or ws <= 0:
        raise ValueError(f"augment_draw: need a positive batch and source size, got n = {n}, source {hs}x{ws}")
    (s0, s1), (r0, r1) = crop if crop is not None else ((1.0, 1.0), (1.0, 1.0))
    if crop is not None and not (0.0 < s0 <= s1 and 0.0 < r0 <= r1):
        raise ValueError(f"augment_draw: scale and ratio must be positive, ordered ranges, got {crop}")
    t = 0
    if coeffs is not None:
        coeffs = _dev(coeffs.detach(), "coeffs")
        if coeffs.dim() != 2 or coeffs.shape[1] != 2 or coeffs.shape[0] < 1 or coeffs.device != rng.device:
            raise ValueError(f"augment_draw: `coeffs` must be a [T, 2] table of gains on the device of `rng`, got {tuple(coeffs.shape)}")
        t = int(coeffs.shape[0])
    for name, pr in (("p_gain", p_gain), ("p_hflip", p_hflip), ("p_vflip", p_vflip)):
        if not 0.0 <= pr <= 1.0:
            raise ValueError(f"augment_draw: `{name}` is a probability, got {pr}")
    if output not in (AUG_OUT_NORMALIZED, AUG_OUT_CLAMPED, AUG_OUT_RAW):
        raise ValueError(f"augment_draw: `output` must be one of AUG_OUT_*, got {output}")
    params = torch.empty((int(n), AUG_COLUMNS), dtype=torch.float32, device=rng.device)
    with _guard(rng.device):
        check(_lib.load().mcq_augment_draw(_ptr(rng), _ptr(params), int(n), hs, ws, int(crop is not None), float(s0), float(s1), float(r0),
                                           float(r1), int(bool(gamma)), _ptr(coeffs), t, float(p_gain), float(p_hflip), float(p_vflip),
                                           int(output), _stream()), "mcq_augment_draw")
    return params


def augment(src: torch.Tensor, size, params: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[N, 3, Hs, Ws] uint8 (read as v / 255) or float32 in [0, 1] -> [N, 3, H, W] float32 under the table `params` [N, 16]
    (augment_draw's, or a caller's): crop box resampled to `size` like F.interpolate(mode="bilinear", antialias=True) on the
    crop, gamma, colour gains, clamp to [0, 1], flips, (v - 0.5) / 0.5 (column AUG_OUTPUT: a half of the pipeline stops earlier) -- one launch (mcq_augment_f32 / _u8).  `out`: write there."""
    if not torch.is_tensor(src) or not src.is_cuda:
        raise RuntimeError(f"mcquic_amd: `src` must live on a HIP device (got {getattr(src, 'device', type(src))}); "
                           "the HIP kernels have no CPU fallback")
    if src.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"augment: `src` must be uint8 or float32 (got {src.dtype})")
    if src.dim() != 4 or src.shape[1] != 3:
        raise ValueError(f"augment: `src` must be a [N, 3, Hs, Ws] batch, got {tuple(src.shape)}")
    if not src.is_contiguous():
        raise ValueError("augment: `src` must be contiguous (NCHW)")
    n, _, hs, ws = src.shape
    h, w = int(size[0]), int(size[1])
    if h <= 0 or w <= 0:
        raise ValueError(f"augment: the output size must be positive, got {h}x{w}")
    if not torch.is_tensor(params) or not params.is_cuda or params.device != src.device:
        raise RuntimeError("augment: `params` must live on the device of `src`; the HIP kernels have no CPU fallback")
    if params.dtype != torch.float32:
        raise TypeError(f"augment: `params` must be float32 (got {params.dtype})")
    if tuple(params.shape) != (n, AUG_COLUMNS) or not params.is_contiguous():
        raise ValueError(f"augment: `params` must be a contiguous [{n}, {AUG_COLUMNS}] table, got {tuple(params.shape)}")
    if out is None:
        out = torch.empty((n, 3, h, w), dtype=torch.float32, device=src.device)
    elif not (out.is_cuda and out.device == src.device and out.dtype == torch.float32 and tuple(out.shape) == (n, 3, h, w) and out.is_contiguous()):
        raise ValueError(f"augment: `out` must be a contiguous float32 [{n}, 3, {h}, {w}] tensor on the device of `src`")
    lib = _lib.load()
    fn, name = (lib.mcq_augment_u8, "mcq_augment_u8") if src.dtype == torch.uint8 else (lib.mcq_augment_f32, "mcq_augment_f32")
    with _guard(src.device):
        check(fn(_ptr(src), _ptr(params), _ptr(out), n, hs, ws, h, w, _stream()), name)
    return out


# ---- validation metrics (mcquic/validate/handlers.py) ----------------------------------------------------------
def _u8_pair(x: torch.Tensor, y: torch.Tensor):
    x, y = _dev(x, "x", torch.uint8), _dev(y, "y", torch.uint8)
    if x.shape != y.shape or x.dim() != 4:
        raise ValueError(f"expected two uint8 [N, C, H, W] batches of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    return x, y


def ms_ssim(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """MS-SSIM value in [0, 1] per image of two uint8 batches (mcquic/validate/metrics.py:142-193 as called by
    handlers.py:14-27).  Sides must exceed 160 pixels (metrics.py:163-166)."""
    x, y = _u8_pair(x, y)
    n, c, h, w = x.shape
    lib = _lib.load()
    nbytes = lib.mcq_ms_ssim_workspace_bytes(n, c, h, w)
    if nbytes == 0:
        raise ValueError(f"MS-SSIM needs image sides larger than 160 pixels, got {h}x{w}")
    ws = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=x.device)
    out = torch.empty(n, dtype=torch.float32, device=x.device)
    with _guard(x.device):
        check(lib.mcq_ms_ssim_u8(_ptr(x), _ptr(y), _ptr(out), _ptr(ws), n, c, h, w, _stream()), "mcq_ms_ssim_u8")
    return out


# The stages of `ms_ssim` one launch at a time, through the launch code of mcq_ms_ssim_u8 (tests/test_gpu_metrics_leaf.py).
def _plane_pair(x: torch.Tensor, y: torch.Tensor, what: str):
    """Two [..., H, W] batches of one shape, both uint8 or both float32 -> (x, y, planes, H, W, "u8" | "f32")."""
    if x.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f"{what}: images must be uint8 or float32 (got {x.dtype})")
    x, y = _dev(x, "x", x.dtype), _dev(y, "y", x.dtype)
    if x.shape != y.shape or x.dim() < 2:
        raise ValueError(f"{what}: expected two [..., H, W] batches of one shape, got {tuple(x.shape)} and {tuple(y.shape)}")
    h, w = x.shape[-2:]
    return x, y, x.numel() // max(h * w, 1), h, w, "u8" if x.dtype == torch.uint8 else "f32"


def ssim_tiles(h: int, w: int):
    """(tiles_y, tiles_x) of the 16 x 118 map tiles of an h x w level (mcq_ssim_tiles; host arithmetic)."""
    ty, tx = ctypes.c_int32(), ctypes.c_int32()
    if _lib.load().mcq_ssim_tiles(h, w, ctypes.byref(ty), ctypes.byref(tx)) != 0:
        raise ValueError(f"an SSIM level needs sides of at least 11 pixels, got {h}x{w}")
    return ty.value, tx.value


def ssim_level(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """One SSIM level of two uint8 or float32 [..., H, W] batches (data range 255): float64 [planes, tiles_y, tiles_x, 2], per map
    tile the sums of the SSIM and of the contrast-structure map over the tile's valid positions (mcq_ssim_level_u8 / _f32)."""
    x, y, planes, h, w, kind = _plane_pair(x, y, "ssim_level")
    ty, tx = ssim_tiles(h, w)
    lib = _lib.load()
    out = torch.empty((planes, ty, tx, 2), dtype=torch.float64, device=x.device)
    fn, name = (lib.mcq_ssim_level_u8, "mcq_ssim_level_u8") if kind == "u8" else (lib.mcq_ssim_level_f32, "mcq_ssim_level_f32")
    with _guard(x.device):
        check(fn(_ptr(x), _ptr(y), planes, h, w, _ptr(out), _stream()), name)
    return out


def ms_ssim_halve(x: torch.Tensor, y: torch.Tensor, out=None):
    """One pooling step of the MS-SSIM pyramid on both images: float32 [..., (H + 1) // 2, (W + 1) // 2] each (mcq_ms_ssim_halve_u8 /
    _f32).  `out`: a pair of contiguous float32 tensors of that size to write into."""
    x, y, planes, h, w, kind = _plane_pair(x, y, "ms_ssim_halve")
    if planes == 0 or h == 0 or w == 0:
        raise ValueError(f"ms_ssim_halve: empty input {tuple(x.shape)}")
    shape = tuple(x.shape[:-2]) + ((h + 1) // 2, (w + 1) // 2)
    if out is None:
        out = (torch.empty(shape, dtype=torch.float32, device=x.device), torch.empty(shape, dtype=torch.float32, device=x.device))
    xo, yo = (_dev(t, "out") for t in out)
    if xo.numel() != planes * shape[-2] * shape[-1] or yo.numel() != xo.numel() or not (out[0].is_contiguous() and out[1].is_contiguous()):
        raise ValueError(f"ms_ssim_halve: `out` must be two contiguous float32 tensors of {shape}")
    lib = _lib.load()
    fn, name = (lib.mcq_ms_ssim_halve_u8, "mcq_ms_ssim_halve_u8") if kind == "u8" else (lib.mcq_ms_ssim_halve_f32, "mcq_ms_ssim_halve_f32")
    with _guard(x.device):
        check(fn(_ptr(x), _ptr(y), _ptr(xo), _ptr(yo), planes, h, w, _stream()), name)
    return xo, yo


def ms_ssim_combine(levels: torch.Tensor) -> torch.Tensor:
    """float32 [5, N, C, 2] per-level {SSIM mean, CS mean} -> MS-SSIM value [N] (mcq_ms_ssim_combine_f32)."""
    levels = _dev(levels, "levels")
    if levels.dim() != 4 or levels.shape[0] != 5 or levels.shape[3] != 2 or levels.numel() == 0:
        raise ValueError(f"ms_ssim_combine: expected a [5, N, C, 2] table, got {tuple(levels.shape)}")
    n, c = levels.shape[1:3]
    out = torch.empty(n, dtype=torch.float32, device=levels.device)
    with _guard(levels.device):
        check(_lib.load().mcq_ms_ssim_combine_f32(_ptr(levels), n, c, _ptr(out), _stream()), "mcq_ms_ssim_combine_f32")
    return out


def ms_ssim_stages(x: torch.Tensor, y: torch.Tensor):
    """`ms_ssim(x, y)` with what the call left in its workspace (mcq_ms_ssim_workspace_layout): (value [N], level table
    [5, N, C, 2] float32 {SSIM mean, CS mean}, [(x_l, y_l) for l = 1..4] pooled images [N, C, H_l, W_l] float32)."""
    x, y = _u8_pair(x, y)
    n, c, h, w = x.shape
    lib = _lib.load()
    lay = (ctypes.c_int64 * _lib.MCQ_MS_SSIM_LAYOUT_WORDS)()
    if lib.mcq_ms_ssim_workspace_layout(n, c, h, w, lay) != 0:
        raise ValueError(f"MS-SSIM needs image sides larger than 160 pixels, got {h}x{w}")
    ws = torch.empty((lay[32] + 7) // 8, dtype=torch.float64, device=x.device)
    out = torch.empty(n, dtype=torch.float32, device=x.device)
    with _guard(x.device):
        check(lib.mcq_ms_ssim_u8(_ptr(x), _ptr(y), _ptr(out), _ptr(ws), n, c, h, w, _stream()), "mcq_ms_ssim_u8")
    floats = ws.view(torch.float32)
    table = floats[lay[31] // 4: lay[31] // 4 + 5 * n * c * 2].view(5, n, c, 2).clone()
    pooled = []
    for l in range(1, 5):
        hl, wl, xo, yo = lay[6 * l], lay[6 * l + 1], lay[6 * l + 4], lay[6 * l + 5]
        pooled.append((floats[xo: xo + n * c * hl * wl].view(n, c, hl, wl).clone(), floats[yo: yo + n * c * hl * wl].view(n, c, hl, wl).clone()))
    return out, table, pooled


def _f32_pair(a: torch.Tensor, b: torch.Tensor):
    a, b = _dev(a, "a"), _dev(b, "b")
    if a.shape != b.shape or a.dim() != 4:
        raise ValueError(f"expected two float32 [N, C, H, W] batches of one shape, got {tuple(a.shape)} and {tuple(b.shape)}")
    if min(a.shape[-2:]) <= 160:
        raise ValueError(f"MS-SSIM needs image sides larger than 160 pixels, got {a.shape[-2]}x{a.shape[-1]}")
    return a, b


def ms_ssim_loss(a: torch.Tensor, b: torch.Tensor, offset: float = 1.0, data_range: float = 2.0):
    """1 - MS-SSIM(a + offset, b + offset) over the batch (mcquic/loss/__init__.py:47-55: data range 2, batch mean) as a
    0-dim float32 tensor, with what the backward needs: (loss, values [5, N, C] per-level map means, saved pooled pyramids).
    mcq_ms_ssim_loss_f32: fixed-order float64 means, no memset -- safe inside a captured step."""
    a, b = _f32_pair(a, b)
    n, c, h, w = a.shape
    lib = _lib.load()
    ws = torch.empty((lib.mcq_ms_ssim_loss_workspace_bytes(n, c, h, w, 0) + 7) // 8, dtype=torch.float64, device=a.device)
    saved = torch.empty(lib.mcq_ms_ssim_loss_saved_bytes(n, c, h, w) // 4, dtype=torch.float32, device=a.device)
    loss = torch.empty((), dtype=torch.float32, device=a.device)
    values = torch.empty((5, n, c), dtype=torch.float32, device=a.device)
    with _guard(a.device):
        check(lib.mcq_ms_ssim_loss_f32(_ptr(a), _ptr(b), float(offset), float(data_range), _ptr(loss), _ptr(values), _ptr(saved),
                                       _ptr(ws), n, c, h, w, _stream()), "mcq_ms_ssim_loss_f32")
    return loss, values, saved


def ms_ssim_loss_bwd(a: torch.Tensor, b: torch.Tensor, values: torch.Tensor, saved: torch.Tensor, dloss: torch.Tensor,
                     offset: float = 1.0, data_range: float = 2.0, want_db: bool = False):
    """(da, db or None) of `ms_ssim_loss` from its `values` and `saved` (mcq_ms_ssim_loss_bwd_f32); `dloss` stays on the device."""
    a, b = _f32_pair(a, b)
    values, saved, dloss = _dev(values, "values"), _dev(saved, "saved"), _dev(dloss, "dloss")
    n, c, h, w = a.shape
    lib = _lib.load()
    if values.shape != (5, n, c) or saved.numel() * 4 != lib.mcq_ms_ssim_loss_saved_bytes(n, c, h, w) or dloss.numel() != 1:
        raise ValueError("ms_ssim_loss_bwd: `values` / `saved` / `dloss` do not belong to this shape")
    ws = torch.empty((lib.mcq_ms_ssim_loss_workspace_bytes(n, c, h, w, 1) + 7) // 8, dtype=torch.float64, device=a.device)
    da = torch.empty_like(a)
    db = torch.empty_like(b) if want_db else None
    with _guard(a.device):
        check(lib.mcq_ms_ssim_loss_bwd_f32(_ptr(a), _ptr(b), float(offset), float(data_range), _ptr(values), _ptr(saved), _ptr(dloss),
                                           _ptr(da), _ptr(db), _ptr(ws), n, c, h, w, _stream()), "mcq_ms_ssim_loss_bwd_f32")
    return da, db


def sqdiff_sum(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """Exact per-image sum of squared differences of two uint8 batches, int64 [N]."""
    x, y = _u8_pair(x, y)
    n = x.shape[0]
    out = torch.empty(n, dtype=torch.int64, device=x.device)
    with _guard(x.device):
        check(_lib.load().mcq_sqdiff_sum_u8(_ptr(x), _ptr(y), _ptr(out), x[0].numel(), n, _stream()), "mcq_sqdiff_sum_u8")
    return out


# ---- backward-pass kernels (training step) ---------------------------------------------------------------------
def nchw_to_nhwc(x: torch.Tensor, square: bool = False) -> torch.Tensor:
    x = _dev(x, "x")
    n, c, h, w = x.shape
    out = torch.empty((n, h, w, c), dtype=torch.float32, device=x.device)
    with _guard(x.device):
        check(_lib.load().mcq_nchw_to_nhwc_f32(_ptr(x), _ptr(out), n, c, h * w, int(square), _stream()), "mcq_nchw_to_nhwc_f32")
    return out


_WGRAD_ROWS = os.environ.get("MCQUIC_AMD_WGRAD_ROWS", "1") != "0"      # A/B switch: 0 = always the NHWC weight-gradient kernel

# ---- the weight gradients' reduce passes, batched over a backward pass (mcq_wgrad_defer / mcq_wgrad_flush) -------------------------------
_WGRAD_DEFER = os.environ.get("MCQUIC_AMD_WGRAD_DEFER", "1") != "0"    # A/B switch: 0 = every weight-gradient launch reduces right away
_defer = {"on": False, "keep": []}
# (round 6, built and dropped: the weight-gradient launches queued onto a side stream, docs/experiments.md section 11.8)


def _set_deferral(on: bool) -> None:
    """The deferral state lives in two places, this module's flag and the library's: they only ever change together."""
    _lib.load().mcq_wgrad_defer(int(on))
    _defer["on"] = on


class wgrad_deferral:
    """`with ops.wgrad_deferral():` around a backward pass this library owns end to end (autograd.backward, parallel.GraphedTrainStep):
    inside, weight-gradient launches leave their partial tiles in their workspaces and record the reduce pass; on exit ALL recorded
    passes run in a few launches (a captured training step: 56 reduce launches -> 3).  Nothing may read a weight gradient before the
    exit -- torch DDP's bucket hooks do, which is why a plain `loss.backward()` never defers.  Workspaces are kept alive until then."""

    def __enter__(self):
        self.active = _WGRAD_DEFER and not _defer["on"]
        if self.active:
            _set_deferral(True)
        return self

    def __exit__(self, exc_type, exc, tb):
        if not self.active:
            return False
        lib = _lib.load()
        _set_deferral(False)
        try:
            if exc_type is None:
                # the library records a reduce pass under the device its launch ran on and flushes the current device's: every
                # device that holds a kept workspace flushes its own passes on its own stream
                for dev in dict.fromkeys(k.device for k in _defer["keep"] if isinstance(k, torch.Tensor)):
                    with _guard(dev):
                        if lib.mcq_wgrad_pending():
                            check(lib.mcq_wgrad_flush(0, _stream()), "mcq_wgrad_flush")
        finally:
            lib.mcq_wgrad_flush(1, None)                     # (whatever is left: the pass it belonged to is gone)
            del _defer["keep"][:]
        return False


class wgrad_now:
    """Inside a `wgrad_deferral`: the weight gradients of this block are reduced right away (their values are read next)."""

    def __enter__(self):
        self.was = _defer["on"]
        if self.was:
            _set_deferral(False)
        return self

    def __exit__(self, *exc):
        if self.was:
            _set_deferral(True)
        return False


def _keep(*tensors) -> None:
    """Workspace AND outputs of a deferred weight-gradient launch stay alive until the flush has written them: a dW the autograd
    engine drops (a frozen weight: requires_grad False) would otherwise be handed to another tensor and the flush would write
    over that one.  Outputs are held through their STORAGE, never the tensor itself (nor a view of it: a view made without grad
    mode still references its base tensor): AccumulateGrad only takes a gradient as it is while nothing else references that very
    tensor -- with a second reference it clones it, during the pass, i.e. before the flush has written the values."""
    if _defer["on"]:
        _defer["keep"].append(tensors[0])
        _defer["keep"].extend(t.untyped_storage() for t in tensors[1:] if t is not None)


def _wgrad_outputs(shapes, device):
    return [None if shape is None else torch.empty(shape, dtype=torch.float32, device=device) for shape in shapes]


def _wgrad_rows_launch(nws: int, device, shapes, launch):
    """One row-kernel launch (csrc/wgrad_rows.hip): a workspace of `nws` floats and an empty output per shape, `launch(ws, outs)`
    on `device`, and everything kept alive for a deferred reduce pass.  Returns the outputs (None where the shape is None)."""
    ws = torch.empty(nws, dtype=torch.float32, device=device)
    outs = _wgrad_outputs(shapes, device)
    with _guard(device):
        launch(ws, outs)
    _keep(ws, *outs)
    return outs


def conv2d_wgrad_group(xs, dys, want_bias: bool = True):
    """Weight (and bias) gradients of several 3x3 stride-1 convolutions of ONE shape in one launch pair
    (mcq_conv2d_wgrad_nchw_group_f32).  Returns [(dW, db or None), ...]; shapes the row-walk kernel does not take, or a
    single pair, go through conv2d_wgrad one by one."""
    lib = _lib.load()
    n, cin, h, w = xs[0].shape
    cout = dys[0].shape[1]
    same = all(x.shape == xs[0].shape for x in xs) and all(d.shape == dys[0].shape for d in dys)
    nws = lib.mcq_conv2d_wgrad_nchw_workspace_floats(n, cin, h, w, cout) if (_WGRAD_ROWS and same and tuple(dys[0].shape[2:]) == (h, w)) else 0
    if not nws or len(xs) == 1:
        out = []
        for x, dy in zip(xs, dys):
            r = conv2d_wgrad(x, dy, 3, 1, want_bias=want_bias)
            out.append(r if want_bias else (r, None))
        return out
    out = []
    cap = lib.mcq_conv2d_wgrad_nchw_max_group()
    # (round 3: capping a group by its operand footprint -- twelve 8 x 128 x 64 x 64 problems as three launches of four --
    #  changed nothing, 984 vs 1038 us: the 82 us per convolution are the kernel's own, not cache eviction between problems)
    for lo in range(0, len(xs), cap):
        gx = [_dev(t, "x") for t in xs[lo:lo + cap]]
        gd = [_dev(t, "dy") for t in dys[lo:lo + cap]]
        k = len(gx)
        table = ctypes.c_void_p * k

        def launch(ws, outs):
            check(lib.mcq_conv2d_wgrad_nchw_group_f32(table(*[t.data_ptr() for t in gx]), table(*[t.data_ptr() for t in gd]),
                                                      table(*[t.data_ptr() for t in outs[:k]]),
                                                      table(*[t.data_ptr() for t in outs[k:]]) if want_bias else None, k, _ptr(ws),
                                                      n, cin, h, w, cout, _stream()), "mcq_conv2d_wgrad_nchw_group_f32")
        outs = _wgrad_rows_launch(nws * k, gx[0].device, [(cout, cin, 3, 3)] * k + [(cout,) if want_bias else None] * k, launch)
        out.extend(zip(outs[:k], outs[k:]))
    return out


def conv2d_wgrad(x: torch.Tensor, dy: torch.Tensor, ksize: int, stride: int, square_x: bool = False, want_bias: bool = False):
    """dW [Cout, Cin, k, k] of y = conv(x, W) + b from NCHW x and dy (channel-major copies are made here, one launch for
    the pair); with `want_bias` returns (dW, db) where db[co] = sum of dy over images and pixels, from the same kernel."""
    x, dy = _dev(x, "x"), _dev(dy, "dy")
    n, cin, h, w = x.shape
    cout, ho, wo = dy.shape[1], dy.shape[2], dy.shape[3]
    lib = _lib.load()
    shapes = [(cout, cin, ksize, ksize), (cout,) if want_bias else None]
    # straight from the NCHW tensors (csrc/wgrad_rows.hip), the first form that applies: (applies?, workspace query, launch, its
    # extra arguments); a query's 0 = a shape that kernel does not take
    rows = ((ksize == 3 and stride == 1 and not square_x,
             lib.mcq_conv2d_wgrad_nchw_workspace_floats, lib.mcq_conv2d_wgrad_nchw_f32, ()),
            (ksize == 3 and stride == 2 and not square_x and (ho, wo) == (h // 2, w // 2),
             lib.mcq_conv2d_wgrad_s2_nchw_workspace_floats, lib.mcq_conv2d_wgrad_s2_nchw_f32, ()),
            (ksize == 1 and stride == 1,
             lib.mcq_conv2d_wgrad1x1_nchw_workspace_floats, lib.mcq_conv2d_wgrad1x1_nchw_f32, (int(square_x),)))
    for applies, query, fn, extra in rows if _WGRAD_ROWS else ():
        nws = query(n, cin, h, w, cout) if applies else 0
        if nws:
            dw, db = _wgrad_rows_launch(nws, x.device, shapes, lambda ws, outs: check(
                fn(_ptr(x), _ptr(dy), _ptr(outs[0]), _ptr(outs[1]), _ptr(ws), n, cin, h, w, cout, *extra, _stream()), fn.__name__))
            return (dw, db) if want_bias else dw
    xt = torch.empty((n, h, w, cin), dtype=torch.float32, device=x.device)
    dyt = torch.empty((n, ho, wo, cout), dtype=torch.float32, device=x.device)
    ws = torch.empty(lib.mcq_conv2d_wgrad_workspace_floats(n, cin, h, w, cout, ksize, stride), dtype=torch.float32, device=x.device)
    dw, db = _wgrad_outputs(shapes, x.device)
    with _guard(x.device):
        check(lib.mcq_nchw_to_nhwc_pair_f32(_ptr(x), _ptr(xt), cin, h * w, int(square_x), _ptr(dy), _ptr(dyt), cout, ho * wo, n,
                                            _stream()), "mcq_nchw_to_nhwc_pair_f32")
        check(lib.mcq_conv2d_wgrad_f32(_ptr(xt), _ptr(dyt), _ptr(dw), _ptr(db), _ptr(ws), n, cin, h, w, cout, ksize, stride,
                                       _stream()), "mcq_conv2d_wgrad_f32")
    return (dw, db) if want_bias else dw


def channel_sum(x: torch.Tensor) -> torch.Tensor:
    x = _dev(x, "x")
    n, c, h, w = x.shape
    out = torch.empty((c,), dtype=torch.float32, device=x.device)
    ws = torch.empty((min(n, 16) * c,), dtype=torch.float32, device=x.device) if n > 1 else None
    with _guard(x.device):
        check(_lib.load().mcq_channel_sum_f32(_ptr(x), _ptr(out), _ptr(ws), n, c, h * w, _stream()), "mcq_channel_sum_f32")
    return out


def silu_bwd(x: torch.Tensor, dy: torch.Tensor, other: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dy * silu'(x) (+ other, a gradient that reaches x along a second path) in one launch."""
    x, dy = _dev(x, "x"), _dev(dy, "dy")
    other = None if other is None else _dev(other, "other")
    if dy.shape != x.shape or (other is not None and other.shape != x.shape):
        raise ValueError("silu_bwd: shape mismatch")
    dx = torch.empty_like(x)
    with _guard(x.device):
        check(_lib.load().mcq_silu_bwd_f32(_ptr(x), _ptr(dy), _ptr(other), _ptr(dx), x.numel(), _stream()), "mcq_silu_bwd_f32")
    return dx


def gate_bwd(a: torch.Tensor, b: torch.Tensor, dout: torch.Tensor):
    a, b, dout = _dev(a, "a"), _dev(b, "b"), _dev(dout, "dout")
    da, db = torch.empty_like(a), torch.empty_like(a)
    with _guard(a.device):
        check(_lib.load().mcq_gate_bwd_f32(_ptr(a), _ptr(b), _ptr(dout), _ptr(da), _ptr(db), a.numel(), _stream()), "mcq_gate_bwd_f32")
    return da, db


def gdn_bwd_prep(x: torch.Tensor, s: torch.Tensor, dy: torch.Tensor, inverse: bool):
    x, s, dy = _dev(x, "x"), _dev(s, "s"), _dev(dy, "dy")
    dxd, ds = torch.empty_like(x), torch.empty_like(x)
    with _guard(x.device):
        check(_lib.load().mcq_gdn_bwd_prep_f32(_ptr(x), _ptr(s), _ptr(dy), int(inverse), _ptr(dxd), _ptr(ds), x.numel(), _stream()),
              "mcq_gdn_bwd_prep_f32")
    return dxd, ds


def pixel_unshuffle2(x: torch.Tensor) -> torch.Tensor:
    x = _dev(x, "x")
    n, c, h2, w2 = x.shape
    out = torch.empty((n, c * 4, h2 // 2, w2 // 2), dtype=torch.float32, device=x.device)
    with _guard(x.device):
        check(_lib.load().mcq_pixel_unshuffle2_f32(_ptr(x), _ptr(out), n, c, h2 // 2, w2 // 2, _stream()), "mcq_pixel_unshuffle2_f32")
    return out


def silu(x: torch.Tensor) -> torch.Tensor:
    x = _dev(x, "x")
    y = torch.empty_like(x)
    with _guard(x.device):
        check(_lib.load().mcq_silu_f32(_ptr(x), _ptr(y), x.numel(), _stream()), "mcq_silu_f32")
    return y


def gate(a: torch.Tensor, b: torch.Tensor, x: torch.Tensor, dual_silu: bool = False) -> torch.Tensor:
    """a * sigmoid(b) + x; with `dual_silu` the result carries silu(result) as its twin (same launch)."""
    a, b, x = _dev(a, "a"), _dev(b, "b"), _dev(x, "x")
    out = torch.empty_like(a)
    out2 = torch.empty_like(a) if dual_silu else None
    with _guard(a.device):
        check(_lib.load().mcq_gate_f32(_ptr(a), _ptr(b), _ptr(x), _ptr(out), _ptr(out2), a.numel(), _stream()), "mcq_gate_f32")
    if out2 is not None:
        set_silu_twin(out, out2)
    return out


def axpby(a: torch.Tensor, b: torch.Tensor, alpha: float, beta: float, dual_silu: bool = False) -> torch.Tensor:
    a, b = _dev(a, "a"), _dev(b, "b")
    if a.shape != b.shape:
        raise ValueError("axpby: shape mismatch")
    out = torch.empty_like(a)
    out2 = torch.empty_like(a) if dual_silu else None
    with _guard(a.device):
        check(_lib.load().mcq_axpby_f32(_ptr(a), _ptr(b), float(alpha), float(beta), _ptr(out), _ptr(out2), a.numel(), _stream()), "mcq_axpby_f32")
    if out2 is not None:
        set_silu_twin(out, out2)
    return out


def vq_inner(x: torch.Tensor, cb: PackedCodebook) -> torch.Tensor:
    """[n, m, h, w, k] inner products <x_v, c_k> (mcq_vq_inner_f32)."""
    x = _dev(x, "x")
    n, c, h, w = x.shape
    out = torch.empty((n, cb.m, h, w, cb.k), dtype=torch.float32, device=x.device)
    with _guard(x.device):
        check(_lib.load().mcq_vq_inner_f32(_ptr(x), _ptr(cb.packed), _ptr(out), n, cb.m, cb.d, h, w, cb.k, _stream()), "mcq_vq_inner_f32")
    return out


def vq_softmax_bwd(logits: torch.Tensor, u_gumbel: Optional[torch.Tensor], ds: torch.Tensor, temperature: torch.Tensor, bound: float,
                   dlogits: Optional[torch.Tensor] = None, raw_logits: Optional[torch.Tensor] = None, rng: Optional[torch.Tensor] = None):
    """In place on `ds` (dSample -> d dist); returns (rowsum, dtrow), each [n, m, h, w].  `dlogits`: a gradient on the returned
    logits themselves, with `raw_logits` = the logits before the random drop.  `u_gumbel` None: the forward's Gumbel draw is
    remade from its generator snapshot `rng`."""
    logits, ds = _dev(logits, "logits"), _dev(ds, "ds")
    if u_gumbel is None and rng is None:
        raise ValueError("vq_softmax_bwd: give the Gumbel draw or the forward's generator snapshot")
    u_gumbel = None if u_gumbel is None else _dev(u_gumbel, "u_gumbel")
    rng = None if rng is None else _dev(rng, "rng", torch.int64)
    if dlogits is not None:
        dlogits, raw_logits = _dev(dlogits, "dlogits"), _dev(raw_logits, "raw_logits")
        if dlogits.shape != logits.shape or raw_logits.shape != logits.shape:
            raise ValueError("dlogits / raw_logits must have the logits' shape")
    n, m, h, w, k = logits.shape
    t = _dev(temperature.detach().reshape(-1), "temperature")
    rowsum = torch.empty((n, m, h, w), dtype=torch.float32, device=logits.device)
    dtrow = torch.empty_like(rowsum)
    with _guard(logits.device):
        check(_lib.load().mcq_vq_softmax_bwd_f32(_ptr(logits), _ptr(u_gumbel), _ptr(rng), _ptr(ds), _ptr(t), float(bound), _ptr(rowsum), _ptr(dtrow),
                                                 _ptr(dlogits), _ptr(raw_logits), n, m, h, w, k, _stream()), "mcq_vq_softmax_bwd_f32")
    return rowsum, dtrow


def vq_soft_bwd(ddist: torch.Tensor, rowsum: torch.Tensor, x: torch.Tensor, ddeq: torch.Tensor, index: torch.Tensor,
                hot: torch.Tensor, cb: PackedCodebook):
    """(dx [n, m*d, h, w], dcodebook [m, k, d]) of the soft assignment + soft dequantisation."""
    x, ddeq = _dev(x, "x"), _dev(ddeq, "ddeq")
    n, m, h, w, k = ddist.shape
    c, hw = x.shape[1], h * w
    xt = torch.empty((n, h, w, c), dtype=torch.float32, device=x.device)
    dqt = torch.empty_like(xt)
    with _guard(x.device):                                     # both channel-major copies from one launch
        check(_lib.load().mcq_nchw_to_nhwc_pair_f32(_ptr(x), _ptr(xt), c, hw, 0, _ptr(ddeq), _ptr(dqt), c, hw, n, _stream()),
              "mcq_nchw_to_nhwc_pair_f32")
    dx = torch.empty_like(x)
    dcb = torch.empty_like(cb.codebook)
    with _guard(x.device):
        check(_lib.load().mcq_vq_soft_bwd_f32(_ptr(ddist), _ptr(rowsum), _ptr(x), _ptr(xt), _ptr(dqt), _ptr(index), _ptr(hot),
                                              _ptr(cb.codebook), _ptr(dx), _ptr(dcb), n, m, cb.d, h, w, k, _stream()), "mcq_vq_soft_bwd_f32")
    return dx, dcb
