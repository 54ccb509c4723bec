"""References for the fused convolution's epilogues: what a test of conv_mfma_kernel's and conv_t16_kernel's epilogue paths compares a
launch with (tests/test_conv_refs.py holds them to float64 autograd / torch's own operations on the CPU).  Nothing here imports
mcquic_amd: every reference is the mathematics, written with torch on the CPU.

A launch computes  out = epilogue(v, sides),  v = conv(prologue(x)) + bias.  The two halves have references of their own:

  conv64 / conv_scale64 / conv_seq_f32   v in float64, the magnitude of its terms (sum |x'| |w| + |b|: what a sum that cancels is
                                         accurate relative to), and v as ONE float32 chain over (channel, tap) -- the longest chain any
                                         tile of the kernel forms (split-K and channel pairs only shorten it), hence the yardstick
  out64 / out_f32 / out_scale64          the epilogue on a given v: the definition in float64; the kernel's operation order with one
                                         float32 rounding per operation (-ffp-contract=off, correctly rounded divide and square root);
                                         and what the result is accurate relative to: the scale of v carried through |d out / d v|,
                                         plus the magnitudes of every addend, never below |out| itself

An epilogue is the keyword set `ops._conv_desc` takes, split into `ep` (its flags and res_scale) and `sides` (its tensors), or one of
the three backward pairs ep = {"bwd": "gdn" | "igdn" | "gate"} with sides {"m", "g"} (the factor and the incoming gradient).
Every function returns the pair (y, second output or None): the second output is the SiLU twin or the backward pair's d s."""
import torch
import torch.nn.functional as F

import _leaf_refs as R

F32 = torch.float32
F64 = torch.float64
EXPF_FLAGS = ("dsilu_mul", "gate_mul", "silu_out")      # what puts an expf in front of y (the twin always has one)


def has_expf(ep, sides=()) -> bool:
    """Does y itself depend on a transcendental?  Where not, a correct kernel returns out_f32's bits."""
    return any(ep.get(k) or k in sides for k in EXPF_FLAGS) or ep.get("bwd") == "gate"


# ---- the accumulate part ---------------------------------------------------------------------------------------------------------------
def prologue64(x, prologue):
    xd = x.double()
    return R.silu64(xd) if prologue == "silu" else xd * xd if prologue == "square" else xd


def prologue_f32(x, prologue):
    return R.silu_f32(x) if prologue == "silu" else x * x if prologue == "square" else x


def conv64(x, w, b, stride=1, prologue=None):
    ks = w.shape[-1]
    return F.conv2d(prologue64(x, prologue), w.double(), None if b is None else b.double(), stride=stride, padding=ks // 2)


def conv_scale64(x, w, b, stride=1, prologue=None):
    ks = w.shape[-1]
    return F.conv2d(prologue64(x, prologue).abs(), w.double().abs(), None if b is None else b.double().abs(), stride=stride, padding=ks // 2)


def conv_seq_f32(x, w, b, stride=1, prologue=None):
    """sum_k x'[k] w[k] as one float32 chain in (channel, tap) order -- product and addition rounded separately -- then + bias."""
    assert x.dtype == F32 and w.dtype == F32
    cout, cin, ks, _ = w.shape
    n, _, h, wd = x.shape
    ho, wo = (h + 2 * (ks // 2) - ks) // stride + 1, (wd + 2 * (ks // 2) - ks) // stride + 1
    cols = F.unfold(prologue_f32(x, prologue), ks, padding=ks // 2, stride=stride)          # [n, cin ks ks, ho wo], channel-major
    wk = w.reshape(cout, cin * ks * ks)
    acc = torch.zeros((n, cout, ho * wo), dtype=F32)
    for k in range(cin * ks * ks):
        acc = acc + wk[None, :, k, None] * cols[:, None, k, :]
    if b is not None:
        acc = acc + b.reshape(1, cout, 1)
    return acc.reshape(n, cout, ho, wo)


def dgrad2_weight(w):
    """The [4 cin, cout, 3, 3] stride-1 filter whose PixelShuffle(2)-stored convolution of dy is the input gradient of the 3x3
    stride-2 padding-1 convolution with `w` [cout, cin, 3, 3]: y[o] reads x[2 o - 1 + k], so dx[2 i + a] collects dy[i] w[k = 1]
    (a = 0) or dy[i] w[k = 2] + dy[i + 1] w[k = 0] (a = 1); as taps t of a padding-1 convolution over dy (tap t reads dy[i + t - 1])
    that is t = 1 <- k = 1 | t = 1 <- k = 2, t = 2 <- k = 0: zero outside the lower-right 2 x 2 taps.  Output channel 4 ci + 2 a + b."""
    cout, cin, ks, _ = w.shape
    assert ks == 3
    taps = {0: ((1, 1),), 1: ((1, 2), (2, 0))}                      # a -> ((t, k), ...)
    wd = torch.zeros((4 * cin, cout, 3, 3), dtype=w.dtype)
    for a in (0, 1):
        for b in (0, 1):
            for th, kh in taps[a]:
                for tw, kw in taps[b]:
                    wd[2 * a + b::4, :, th, tw] = w[:, :, kh, kw].t()
    return wd


# ---- the epilogue ------------------------------------------------------------------------------------------------------------------------
def _dsilu64(m):
    s = torch.sigmoid(m)
    return s * (1 + m * (1 - s))


def out64(v, ep, sides):
    """The definition in float64 on a pre-epilogue value `v` (any dtype; taken as exact)."""
    v = v.double()
    sd = {k: t.double() for k, t in sides.items()}
    bwd = ep.get("bwd")
    if bwd in ("gdn", "igdn"):                             # (clones: the autograd helpers mark a float64 argument itself as a leaf)
        return R.gdn_bwd_prep64(sd["m"].clone(), v.clone(), sd["g"], bwd == "igdn")
    if bwd == "gate":
        return R.gate_bwd64(sd["m"].clone(), v.clone(), sd["g"])
    if ep.get("shuffle2"):
        v = F.pixel_shuffle(v, 2)
    if "dsilu_mul" in sd:
        v = R.silu_bwd64(sd["dsilu_mul"].clone(), v)
    if "mul" in sd:
        v = sd["mul"] * v
    if "gdn_mul" in sd:
        v = sd["gdn_mul"] * v ** -0.5
    if "igdn_mul" in sd:
        v = sd["igdn_mul"] * v ** 0.5
    if "gate_mul" in sd:
        v = R.gate64(sd["gate_mul"], v, sd["gate_id"])
    if "res" in sd:
        v = v + R.f32(ep.get("res_scale", 1.0)).double() * sd["res"]
    if ep.get("silu_out"):
        v = R.silu64(v)
    return v, (R.silu64(v) if ep.get("dual_silu") else None)


def out_f32(v, ep, sides):
    """The kernel's order, one float32 rounding per operation: bias (already in v), * silu'(m), + res_scale * res, SiLU, twin."""
    assert v.dtype == F32 and all(t.dtype == F32 for t in sides.values())
    bwd = ep.get("bwd")
    if bwd in ("gdn", "igdn"):
        return R.gdn_bwd_prep_f32(sides["m"], v, sides["g"], bwd == "igdn")
    if bwd == "gate":
        return R.gate_bwd_f32(sides["m"], v, sides["g"])
    if ep.get("shuffle2"):
        v = F.pixel_shuffle(v, 2)
    if "dsilu_mul" in sides:
        v = R.silu_bwd_f32(sides["dsilu_mul"], v)
    if "mul" in sides:
        v = sides["mul"] * v
    if "gdn_mul" in sides:
        v = sides["gdn_mul"] * R.div_f32(1.0, R.sqrt_f32(v))
    if "igdn_mul" in sides:
        v = sides["igdn_mul"] * R.sqrt_f32(v)
    if "gate_mul" in sides:
        v = R.gate_f32(sides["gate_mul"], v, sides["gate_id"])
    if "res" in sides:
        v = v + R.f32(ep.get("res_scale", 1.0)) * sides["res"]
    if ep.get("silu_out"):
        v = R.silu_f32(v)
    return v, (R.silu_f32(v) if ep.get("dual_silu") else None)


def out_scale64(v64, vscale64, ep, sides):
    """What the two outputs are accurate relative to when v is accurate relative to `vscale64`: the scale goes through every
    operation times |d out / d v|, an addition adds the magnitude of its addend, a product with silu'(m) near the zero of silu' counts
    relative to |v| (R.silu_bwd_scale64) and d s of the gate's backward relative to |g a| / 4 where 1 - s cancels
    (R.gate_bwd_db_scale64); no result is accurate beyond its own magnitude (every operation rounds relative to its result)."""
    v, s = v64.double(), vscale64.double()
    sd = {k: t.double() for k, t in sides.items()}
    bwd = ep.get("bwd")
    if bwd in ("gdn", "igdn"):
        m, g = sd["m"], sd["g"]
        o1, o2 = out64(v, ep, sides)
        if bwd == "gdn":                                    # g v^-1/2, -1/2 g m v^-3/2
            d1, d2 = 0.5 * g.abs() * v ** -1.5, 0.75 * (g * m).abs() * v ** -2.5
        else:                                               # g v^1/2, 1/2 g m v^-1/2
            d1, d2 = 0.5 * g.abs() * v ** -0.5, 0.25 * (g * m).abs() * v ** -1.5
        return torch.maximum(s * d1, o1.abs()), torch.maximum(s * d2, o2.abs())
    if bwd == "gate":
        m, g = sd["m"], sd["g"]
        o1, o2 = out64(v, ep, sides)
        sg = torch.sigmoid(v)
        d1, d2 = g.abs() * sg * (1 - sg), (g * m).abs() * sg * (1 - sg) * (1 - 2 * sg).abs()
        return torch.maximum(s * d1, o1.abs()), torch.maximum(torch.maximum(s * d2, o2.abs()), R.gate_bwd_db_scale64(m, v, g))
    if ep.get("shuffle2"):
        v, s = F.pixel_shuffle(v, 2), F.pixel_shuffle(s, 2)
    if "dsilu_mul" in sd:
        m = sd["dsilu_mul"]
        s = torch.maximum(s * _dsilu64(m).abs(), R.silu_bwd_scale64(m, v))
        v = v * _dsilu64(m)
    if "mul" in sd:
        v, s = sd["mul"] * v, sd["mul"].abs() * s
    if "gdn_mul" in sd:
        m = sd["gdn_mul"]
        v, s = m * v ** -0.5, 0.5 * m.abs() * v ** -1.5 * s
    if "igdn_mul" in sd:
        m = sd["igdn_mul"]
        v, s = m * v ** 0.5, 0.5 * m.abs() * v ** -0.5 * s
    if "gate_mul" in sd:
        m, sg = sd["gate_mul"], torch.sigmoid(v)
        s = s * m.abs() * sg * (1 - sg) + (m * sg).abs() + sd["gate_id"].abs()
        v = m * sg + sd["gate_id"]
    if "res" in sd:
        add = R.f32(ep.get("res_scale", 1.0)).double() * sd["res"]
        v, s = v + add, s + add.abs()
    s = torch.maximum(s, v.abs())
    if ep.get("silu_out"):
        s = torch.maximum(s * _dsilu64(v).abs(), R.silu64(v).abs())
        v = R.silu64(v)
    twin = None
    if ep.get("dual_silu"):
        twin = torch.maximum(s * _dsilu64(v).abs(), R.silu64(v).abs())
    return s, twin


def rel_err(got, want64, scale64) -> float:
    """max |got - want| / scale; a scale of exactly zero (an output whose every term is zero) counts as the smallest normal."""
    assert torch.isfinite(got).all(), "non-finite result"
    return float(((got.double() - want64).abs() / scale64.clamp_min(R.TINY)).max())
