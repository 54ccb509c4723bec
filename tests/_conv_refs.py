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
Every function returns the pair (y, second output or None): the second output is the SiLU twin or the backward pair's d s.

The fused 1x1 layer behind a 3x3 convolution (the POST section of conv_mfma_kernel: MCQ_CONV_POST_GDN / _IGDN / _GATE) is a second
contraction on top of v and has references of its own at the end of this file:

  post64 / post_f32 / post_scale64       the close on a given v: s = b1 + w1 @ v^2 (GDN / IGDN) or b1 + w1 @ (v + res_scale res) (gate) and
                                         out = v / sqrt(s) | v sqrt(s) | mul sigmoid(s) + id; the float32 form sums s as ONE chain from
                                         the bias over all 128 channels in the kernel's channel order (POST_ORDER)
  to_subpixel_rows / from_subpixel_rows  the row order of a [512, Cin, 3, 3] layer whose four 128-row tiles are the four sub-pixels of
                                         a PixelShuffle(2) store, and the way back from such a layer's output to the shuffled map
  POST_GEOMS / post_problem / post_layer the seeded inputs of tests/test_gpu_conv_post_epilogues.py (tests/test_conv_refs.py checks
                                         the same ones on the CPU)

The kernels beside the direct form -- conv_head16_kernel and the three Winograd forms -- have their references at the very end:

  wino1d_f32 / wino2d_f32                F(2, 3) along x and F(2x2, 3x3) restated with one float32 (or float64) rounding per operation
  exact_case                             integer inputs on which the direct and the Winograd arithmetic are exact, the bound asserted
  OTHER_GEOMS / OTHER_CHANNELS / other_problem / other_yardstick   the inputs of tests/test_gpu_conv_other_kernels.py"""
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


# ---- the fused 1x1 layer behind a 3x3 convolution (MCQ_CONV_POST_*) ------------------------------------------------------------------------
POST_C = 128
# the kernel contracts over the accumulator registers in THEIR order: k-step t = 16 mb + r takes the channels c = 32 mb + (r & 3) + 8 (r >> 2)
# and c + 4 (the two k-slots of a 32x32x2 MFMA)
POST_ORDER = tuple(ch for mb in range(4) for r in range(16) for ch in (32 * mb + (r & 3) + 8 * (r >> 2), 32 * mb + (r & 3) + 8 * (r >> 2) + 4))
assert sorted(POST_ORDER) == list(range(POST_C))


def _post_w(w1):
    assert w1.numel() == POST_C * POST_C and tuple(w1.shape[:2]) == (POST_C, POST_C)
    return w1.reshape(POST_C, POST_C)


def _mix64(w, b1, u):
    """b1 + w @ u over the channel axis of u [n, 128, h, w] in float64 (a plain contraction, no convolution routine)."""
    s = torch.einsum("oc,nchw->nohw", w, u)
    return s if b1 is None else s + b1.double().reshape(1, POST_C, 1, 1)


def post64(v, kind, w1, b1, sides=None, res_scale=1.0):
    """The definition in float64 on the producing convolution's value `v` [n, 128, h, w] (bias included, residual not yet added; any
    dtype, taken as exact) -> (out, twin or None): the twin, silu(out), belongs to the gate only."""
    v, w = v.double(), _post_w(w1).double()
    sd = {k: t.double() for k, t in (sides or {}).items()}
    if kind in ("gdn", "igdn"):
        s = _mix64(w, b1, v * v)
        return (v * torch.sqrt(s) if kind == "igdn" else v / torch.sqrt(s)), None
    assert kind == "gate"
    if "res" in sd:
        v = v + R.f32(res_scale).double() * sd["res"]
    out = sd["gate_mul"] * torch.sigmoid(_mix64(w, b1, v)) + sd["gate_id"]
    return out, R.silu64(out)


def post_f32(v, kind, w1, b1, sides=None, res_scale=1.0, chunk=8192):
    """The same with one float32 rounding per operation, in the kernel's order: + res_scale * res, then s as ONE chain that starts
    from the 1x1 layer's bias (0 without one) and adds the rounded products w1[o, c] u[c] one by one in POST_ORDER, then the close
    (correctly rounded square root and quotient; the gate and the twin as R.gate_f32 / R.silu_f32)."""
    sides = sides or {}
    assert v.dtype == F32 and w1.dtype == F32 and all(t.dtype == F32 for t in sides.values())
    w = _post_w(w1)
    n, c, h, wd = v.shape
    assert c == POST_C
    if kind == "gate" and "res" in sides:
        v = v + R.f32(res_scale) * sides["res"]
    u = (v * v if kind in ("gdn", "igdn") else v).permute(1, 0, 2, 3).reshape(POST_C, -1)          # [channel, pixel]
    s = torch.empty_like(u)
    start = torch.zeros(POST_C, dtype=F32) if b1 is None else b1.to(F32)
    for lo in range(0, u.shape[1], chunk):                          # (pixel chunks that stay in the cache; the chain is per element)
        uc = u[:, lo:lo + chunk]
        acc = start.reshape(POST_C, 1).repeat(1, uc.shape[1])
        tmp = torch.empty_like(acc)
        for ch in POST_ORDER:
            torch.mul(w[:, ch:ch + 1], uc[ch:ch + 1, :], out=tmp)
            acc.add_(tmp)
        s[:, lo:lo + chunk] = acc
    s = s.reshape(POST_C, n, h, wd).permute(1, 0, 2, 3).contiguous()
    if kind == "gdn":
        return v * R.div_f32(1.0, R.sqrt_f32(s)), None
    if kind == "igdn":
        return v * R.sqrt_f32(s), None
    out = R.gate_f32(sides["gate_mul"], s, sides["gate_id"])
    return out, R.silu_f32(out)


def post_scale64(v64, vscale64, kind, w1, b1, sides=None, res_scale=1.0):
    """What the two outputs are accurate relative to when v is accurate relative to `vscale64` (never below |v|): s carries the
    magnitude sum of its chain, |b1| + |w1| @ |v|^p, and what v's own error does to it (|w1| @ 2 |v| vscale for the squares,
    |w1| @ vscale for the gate, whose v first takes |res_scale res| into its scale); the close carries that through its derivative
    in s, adds v's own scale through its derivative in v (GDN / IGDN) or the magnitudes of the gate's two addends, and is never
    accurate beyond its own magnitude.  The twin: the output's scale through |silu'|, never below |silu(out)|."""
    v, w = v64.double(), _post_w(w1).double().abs()
    vs = torch.maximum(vscale64.double(), v.abs())
    sd = {k: t.double() for k, t in (sides or {}).items()}
    ab = None if b1 is None else b1.double().abs()
    out, _ = post64(v, kind, w1, b1, sides, res_scale)
    if kind in ("gdn", "igdn"):
        s = _mix64(_post_w(w1).double(), b1, v * v)
        ss = _mix64(w, ab, v * v) + _mix64(w, None, 2.0 * v.abs() * vs)
        if kind == "gdn":                                   # v s^-1/2
            sc = vs * s ** -0.5 + 0.5 * v.abs() * s ** -1.5 * ss
        else:                                               # v s^1/2
            sc = vs * s ** 0.5 + 0.5 * v.abs() * s ** -0.5 * ss
        return torch.maximum(sc, out.abs()), None
    if "res" in sd:
        add = R.f32(res_scale).double() * sd["res"]
        v, vs = v + add, vs + add.abs()
        vs = torch.maximum(vs, v.abs())
    sg = torch.sigmoid(_mix64(_post_w(w1).double(), b1, v))
    ss = _mix64(w, ab, vs)
    m = sd["gate_mul"]
    sc = torch.maximum(ss * m.abs() * sg * (1 - sg) + (m * sg).abs() + sd["gate_id"].abs(), out.abs())
    return sc, torch.maximum(sc * _dsilu64(out).abs(), R.silu64(out).abs())


# ---- the sub-pixel form: MCQ_CONV_POST_IGDN through the PixelShuffle store ---------------------------------------------------------------------
def to_subpixel_rows(w, b):
    """A [512, Cin, 3, 3] layer (+ bias) in sub-pixel-major row order: row 128 T + c = channel 4 c + T, so that row tile T holds the
    128 channels PixelShuffle(2) sends to sub-pixel T = 2 dy + dx of every 2 x 2 cell."""
    assert w.shape[0] == 4 * POST_C
    rows = torch.tensor([4 * c + t for t in range(4) for c in range(POST_C)])
    return w[rows].contiguous(), (None if b is None else b[rows].contiguous())


def from_subpixel_rows(v):
    """The output [n, 512, h, w] of a layer in sub-pixel-major row order as the shuffled map [n, 128, 2 h, 2 w]:
    out[n, c, 2 y + dy, 2 x + dx] = v[n, 128 (2 dy + dx) + c, y, x]."""
    n, c4, h, wd = v.shape
    assert c4 == 4 * POST_C
    out = torch.empty((n, POST_C, 2 * h, 2 * wd), dtype=v.dtype)
    for t in range(4):
        out[:, :, (t >> 1)::2, (t & 1)::2] = v[:, POST_C * t:POST_C * (t + 1)]
    return out


# ---- the inputs of tests/test_gpu_conv_post_epilogues.py -----------------------------------------------------------------------------------------
# the smallest geometries at which each index of the POST section can go wrong; N = 2 (the second image's slab is addressed); `sub`: the
# 3x3 layer has 512 rows and stores through the PixelShuffle.  The last two fill the chip (2048 wave tiles of 128 channels x 32
# pixels: the launcher takes the fused form by its own choice there); Cin = 8 keeps their CPU references at about a second each.
POST_GEOMS = {
    "odd7x9": dict(n=2, cin=20, h=7, w=9, stride=1, sub=False),          # 63 pixels: two pixel blocks, the second ragged; odd width; Cin % 8 = 4
    "s2_7x10": dict(n=2, cin=20, h=7, w=10, stride=2, sub=False),        # stride 2 from an odd and an even input side -> 4 x 5
    "tiny3x3": dict(n=2, cin=128, h=3, w=3, stride=1, sub=False),        # smaller than one pixel block: most lanes carry the out-of-range marker
    "sub5x7": dict(n=2, cin=20, h=5, w=7, stride=1, sub=True),           # -> 10 x 14
    "sub3x3": dict(n=2, cin=128, h=3, w=3, stride=1, sub=True),          # -> 6 x 6
    "chip128x256": dict(n=2, cin=8, h=128, w=256, stride=1, sub=False),
    "chip_sub128x128": dict(n=1, cin=8, h=128, w=128, stride=1, sub=True),
}
POST_EXACT = ("shift1", "shift4", "shift32", "perm")


def post_problem(gname, bias3=True):
    """(x, w, b) of the producing 3x3 layer at geometry `gname`: seeded normal values, the weights scaled to a unit-variance v."""
    g = POST_GEOMS[gname]
    seed = 3000 + 11 * sum(ord(ch) for ch in gname)
    cout = 4 * POST_C if g["sub"] else POST_C
    x = R.randn((g["n"], g["cin"], g["h"], g["w"]), seed)
    w = R.randn((cout, g["cin"], 3, 3), seed + 1, (g["cin"] * 9) ** -0.5)
    return x, w, (R.randn((cout,), seed + 2, 0.1) if bias3 else None)


def post_layer(kind, variant="dense", bias1=True):
    """(w1 [128, 128], b1 or None) of the fused 1x1 layer.  dense: GDN / IGDN positive with b1 >= 1 (s >= 1: no bar divides by a
    vanishing scale), the gate signed at scale 1 / sqrt(128).  One of POST_EXACT: a permutation matrix times powers of two (a cyclic
    shift by 1, 4 or 32, or a seeded permutation) with b1 = 1 (GDN / IGDN) or 0 (gate): s has ONE non-zero term next to its bias, so
    it is the same in any summation order, and a weight packed into the wrong lane or k-step is an O(1) error."""
    seed = 4000 + 17 * ("gdn", "igdn", "gate").index(kind)
    if variant == "dense":
        if kind == "gate":
            return R.randn((POST_C, POST_C), seed, POST_C ** -0.5), (R.randn((POST_C,), seed + 1, 0.1) if bias1 else None)
        return R.randn((POST_C, POST_C), seed).abs() / POST_C, (R.randn((POST_C,), seed + 1, 0.5).abs() + 1.0 if bias1 else None)
    assert variant in POST_EXACT and bias1
    g = torch.Generator().manual_seed(seed + 5 + POST_EXACT.index(variant))
    if variant == "perm":
        src = torch.randperm(POST_C, generator=g)
    else:
        src = (torch.arange(POST_C) + int(variant[5:])) % POST_C
    w1 = torch.zeros((POST_C, POST_C), dtype=F32)
    w1[torch.arange(POST_C), src] = torch.exp2(torch.randint(-2, 3, (POST_C,), generator=g).float())
    return w1, torch.full((POST_C,), 0.0 if kind == "gate" else 1.0, dtype=F32)


def post_sides(names, shape, seed=5000):
    """The gate's output-shaped side tensors (res, gate_mul, gate_id), seeded."""
    scale = dict(res=1.0, gate_mul=2.0, gate_id=0.5)
    return {k: R.randn(shape, seed + 13 * ("res", "gate_mul", "gate_id").index(k), scale[k]) for k in names}


# ---- the other convolution kernels: conv_head16_kernel and the three Winograd forms (tests/test_gpu_conv_other_kernels.py) ------------------
# F(2, 3) / F(2x2, 3x3):  Y = A^T [ sum_c (G g G^T) . (B^T d B) ] A  with
#   G = [[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]],  B^T d = (d0 - d2, d1 + d2, d2 - d1, d1 - d3),  A^T m = (m0 + m1 + m2, m1 - m2 - m3)
WINO_G = ((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0))


def _bt(d0, d1, d2, d3, bound):
    """B^T along one axis: one subtraction or addition each (with `bound`: of magnitudes, every sign a plus)."""
    if bound:
        return d0 + d2, d1 + d2, d2 + d1, d1 + d3
    return d0 - d2, d1 + d2, d2 - d1, d1 - d3


def _at(m0, m1, m2, m3, bound):
    """A^T along one axis in the kernels' order: (m0 + m1) + m2 and (m1 - m2) - m3."""
    if bound:
        return (m0 + m1) + m2, (m1 + m2) + m3
    return (m0 + m1) + m2, (m1 - m2) - m3


def _wino(form, x, w, b, dtype, bound=False):
    """Both Winograd forms of the 3x3 stride-1 padding-1 convolution with one rounding of `dtype` per operation.  U is formed in
    float64 and rounded once (as the pack kernels do), the input transform, the sum over channels (1-D: over channel and filter row)
    as ONE sequential chain of separately rounded products, and the inverse transform run in `dtype`; the bias is added last.
    `bound`: the same walk over magnitudes with every sign a plus -- an upper bound of every intermediate of the true walk
    (returned as (result, largest input-transform value, largest |U|); the chain's partial sums are below its last one)."""
    assert form in ("wino1d", "wino2d") and w.shape[-2:] == (3, 3) and x.dtype == w.dtype
    n, cin, h, wd = x.shape
    cout = w.shape[0]
    g = torch.tensor(WINO_G, dtype=F64)
    if form == "wino1d":
        u = torch.einsum("pa,ocya->ocyp", g, w.double())                # [cout, cin, filter row, position]
    else:
        u = torch.einsum("pa,ocab,qb->ocpq", g, w.double(), g)          # [cout, cin, position y, position x]
    u = u.to(dtype)
    xx = x.to(dtype)
    if bound:
        u, xx = u.abs(), xx.abs()
    wt = (wd + 1) // 2
    if form == "wino1d":
        xp = F.pad(xx, (1, 2 * wt + 1 - wd, 1, 1))                      # columns 2 xp - 1 .. 2 xp + 2 of pair xp, rows y - 1 .. y + 1
        # v[pos]: [n, cin, filter row, h, wt]
        rows = [[xp[:, :, dy:dy + h, j:j + 2 * wt:2] for j in range(4)] for dy in range(3)]
        v = [torch.stack([_bt(*rows[dy], bound)[pos] for dy in range(3)], dim=2) for pos in range(4)]
        acc = [torch.zeros((n, cout, h, wt), dtype=dtype) for _ in range(4)]
        for c in range(cin):
            for dy in range(3):
                for pos in range(4):
                    acc[pos] = acc[pos] + u[None, :, c, dy, pos, None, None] * v[pos][:, None, c, dy]
        even, odd = _at(*acc, bound)
        out = torch.stack((even, odd), dim=-1).reshape(n, cout, h, 2 * wt)[..., :wd]
        vmax = max(float(t.max()) for t in v) if bound else None
    else:
        ht = (h + 1) // 2
        xp = F.pad(xx, (1, 2 * wt + 1 - wd, 1, 2 * ht + 1 - h))
        d = [[xp[:, :, i:i + 2 * ht:2, j:j + 2 * wt:2] for j in range(4)] for i in range(4)]          # the 4 x 4 patch under a tile
        t = [_bt(*d[i], bound) for i in range(4)]                       # along x, row by row
        v = [_bt(t[0][j], t[1][j], t[2][j], t[3][j], bound) for j in range(4)]      # along y: v[j][i] = V[i][j]
        acc = [[torch.zeros((n, cout, ht, wt), dtype=dtype) for _ in range(4)] for _ in range(4)]
        for c in range(cin):
            for i in range(4):
                for j in range(4):
                    acc[i][j] = acc[i][j] + u[None, :, c, i, j, None, None] * v[j][i][:, None, c]
        sx = [_at(*acc[i], bound) for i in range(4)]                    # sx[i][ox]
        col = [_at(sx[0][ox], sx[1][ox], sx[2][ox], sx[3][ox], bound) for ox in range(2)]          # col[ox][oy]
        out = torch.empty((n, cout, 2 * ht, 2 * wt), dtype=dtype)
        for oy in range(2):
            for ox in range(2):
                out[:, :, oy::2, ox::2] = col[ox][oy]
        out = out[:, :, :h, :wd]
        vmax = max(float(e.max()) for r in v for e in r) if bound else None
    if b is not None:
        out = out + (b.abs() if bound else b).to(dtype).reshape(1, cout, 1, 1)
    out = out.contiguous()
    return (out, vmax, float(u.max())) if bound else out


def wino1d_f32(x, w, b, dtype=F32):
    """F(2, 3) along x (MCQ_CONV_WINOGRAD) restated with one `dtype` rounding per operation: see _wino."""
    return _wino("wino1d", x, w, b, dtype)


def wino2d_f32(x, w, b, dtype=F32):
    """F(2x2, 3x3) (MCQ_CONV_WINOGRAD2D / _WINOGRAD2D16) restated with one `dtype` rounding per operation: see _wino."""
    return _wino("wino2d", x, w, b, dtype)


EXACT_LIMIT = float(1 << 24)            # integers below this magnitude are float32 values, and so are their sums and differences


def exact_case(form, cin, cout, h, w, n=2, seed=0):
    """Integer-valued float32 (x, weight, bias, res) for which every intermediate of the direct and of the `form` arithmetic
    ("direct", "wino1d", "wino2d") is an integer below 2^24 in magnitude, whatever the order of summation: x in -3 .. 3, the bias and
    the residual in -8 .. 8, the weights in -2 .. 2 times 1 (direct), 2 (1-D: U = G g is integral) or 4 (2-D: U = G g G^T is).
    The bound is computed, not assumed: the direct sum of magnitudes sum |x| |w| + |b| + |res|, and for the Winograd forms the walk
    of _wino over magnitudes (sum over channels of |U| |V|, through A^T with every sign a plus, + |b| + |res|), which bounds every
    partial sum and every transform value of the true walk; U is checked to be integral."""
    step = dict(direct=1, wino1d=2, wino2d=4)[form]
    g = torch.Generator().manual_seed(9000 + seed)
    ri = lambda lo, hi, shape: torch.randint(lo, hi + 1, shape, generator=g).to(F32)          # noqa: E731
    x, wt, b = ri(-3, 3, (n, cin, h, w)), step * ri(-2, 2, (cout, cin, 3, 3)), ri(-8, 8, (cout,))
    res = ri(-8, 8, (n, cout, h, w))
    direct = conv_scale64(x, wt, b) + res.double().abs()
    assert float(direct.max()) < EXACT_LIMIT, f"direct sum of magnitudes {float(direct.max()):.0f}"
    if form != "direct":
        gm = torch.tensor(WINO_G, dtype=F64)
        u = torch.einsum("pa,ocya->ocyp", gm, wt.double()) if form == "wino1d" else torch.einsum("pa,ocab,qb->ocpq", gm, wt.double(), gm)
        assert torch.equal(u, u.round()), "U is not integral"
        top, vmax, umax = _wino(form, x, wt, b, F64, bound=True)
        top = top + res.double().abs()
        assert max(float(top.max()), vmax, umax) < EXACT_LIMIT, f"Winograd walk of magnitudes {float(top.max()):.0f}"
    return x, wt, b, res


# geometries (N = 2 everywhere: the second image's slab is addressed) and channel counts of tests/test_gpu_conv_other_kernels.py;
# tests/test_conv_refs.py holds the restatements to conv64 on the same ones
OTHER_GEOMS = {
    "odd7x9": (7, 9),           # half-empty pairs / 2 x 2 tiles on both edges; no multiple of a block
    "row1x9": (1, 9),           # a one-pixel-high map: every tile half empty along y
    "col5x1": (5, 1),           # a one-pixel-wide map: every pair / tile half empty along x
    "tiny2x2": (2, 2),          # one tile, one block
    "wide9x35": (9, 35),        # 18 tiles per row: more than one 16-tile block (wino16); a second 16-pixel segment and a ragged third (head16)
    "seg3x17": (3, 17),         # head16: the 4 segments of a wave straddle the row and the image boundary; the last wave's groups clamp
}
WINO_GEOMS = ("odd7x9", "row1x9", "col5x1", "tiny2x2", "wide9x35")
HEAD_GEOMS = WINO_GEOMS + ("seg3x17",)
# (cin, cout, forced tile).  head16: Cin 6 = no multiple of 4 (the last group's k lanes past Cin).  F(2, 3): Cin 20 = channel-pair
# padding live; Cout 64 / 192 the 64-row instance, 128 the 128-row one, also forced to 64 rows (tile 0x22).  32x32x2: Cin 24 = the
# smallest wino16 refuses.  16x16x4: Cin 16 = the peeled first body and one pass of the loop (a body is two 4-channel groups and the
# launcher takes whole 16s: there is no smaller count), Cin 48 = six bodies.
OTHER_CHANNELS = {
    "head16": tuple((ci, co, 0) for ci in (6, 128) for co in (3, 12, 16)),
    "wino1d": tuple((ci, co, t) for ci in (20, 128) for co, t in ((64, 0), (192, 0), (128, 0), (128, 0x22))),
    "wino32": tuple((ci, co, 0) for ci in (24, 128) for co in (128, 256)),
    "wino16": tuple((ci, co, 0) for ci in (16, 48) for co in (128, 256)),
}
OTHER_FORM = dict(head16="direct", wino1d="wino1d", wino32="wino2d", wino16="wino2d")


def other_problem(kernel, gname, cin, cout, bias=True, variant=0):
    """Seeded (x, w, b) of one (kernel, geometry, channel count): normal values, the weights scaled to a unit-variance result;
    `variant` gives the problems of a multi-problem launch tensors of their own."""
    h, w = OTHER_GEOMS[gname]
    seed = 6000 + 31 * sum(ord(ch) for ch in kernel + gname) + 7 * cin + cout + 100000 * variant
    return (R.randn((2, cin, h, w), seed), R.randn((cout, cin, 3, 3), seed + 1, (cin * 9) ** -0.5),
            R.randn((cout,), seed + 2, 0.1) if bias else None)


def other_yardstick(kernel, x, w, b, prologue=None):
    """v as the float32 restatement of the kernel's OWN algorithm: the yardstick of the whole-launch bar."""
    form = OTHER_FORM[kernel]
    if form == "direct":
        return conv_seq_f32(x, w, b, 1, prologue)
    assert prologue is None
    return _wino(form, x, w, b, F32)
