"""Inputs and references for the leaf kernels of the training step (tests/test_gpu_leaf_ops.py and, for the training quantizer's
soft assignment, tests/test_gpu_soft_assign_leaf.py hold the HIP kernels to them, tests/test_leaf_ops_reference.py holds the
float32 restatements to float64 autograd on the CPU and soft_bwd64 to the oracle's own derivative).  Nothing here imports
mcquic_amd: every reference is the mathematics, written with torch on the CPU.

Two kinds of reference per op:
  *64       the operation in float64 (torch.autograd where it is a derivative)
  *_f32     the kernel's own operation order, one float32 rounding per operation (the library is built with -ffp-contract=off;
            float divide and square root are correctly rounded on both sides): what a correct kernel returns bit for bit where
            no transcendental is involved, and the yardstick for the ulp bars where one is (4x its own worst error)."""
import torch

F32 = torch.float32
FLAT_SIZES = (1, 3, 255, 256, 257, 1023, 4097, 2 ** 20 + 3)          # every n % 4, both sides of a 256-thread workgroup and of a 4096 chunk
NET_SHAPE = (8, 128, 64, 64)                                         # one network-sized activation (4 M elements)
SHAPES = ((1, 1, 1, 1), (2, 3, 5, 7), (3, 33, 1, 1), (2, 40, 9, 13), (1, 64, 32, 32), (35, 5, 3, 3))
SILU_DZERO = -1.2784645427610738                                     # the zero of silu'
ULP_FLOOR = 2.0 ** -80                                               # below this magnitude (8e-25) errors count absolutely (see ulp_err)


def f32(v) -> torch.Tensor:
    """A Python float as the float32 scalar a `float` kernel argument receives."""
    return torch.tensor(float(v), dtype=F32)


def sqrt_f32(t):
    """The correctly rounded float32 square root.  Not torch.sqrt: ATen's vectorised float32 kernel is up to an ulp off on AVX-512
    hosts (its scalar path is exact, so one- and three-element tensors agreed and 255-element ones did not -- found by the first
    GPU run of test_gdn_bwd_prep, where the device's sqrtf WAS the correctly rounded one).  The float64 root rounded to float32 is:
    53 >= 2 * 24 + 2 bits make the double rounding innocuous."""
    return torch.sqrt(t.double()).to(F32)


def div_f32(a, b):
    """The correctly rounded float32 quotient, through float64 for the same reason."""
    return (torch.as_tensor(a, dtype=torch.float64) / b.double()).to(F32)


def rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(shape, generator=g) * 2 - 1) * scale).to(F32)


def randn(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(F32)


def special_x(n, seed):
    """n arguments of a sigmoid: [-30, 30] evenly (shuffled), then -- room permitting -- the points where kernels go wrong written over
    the head: +-87 and +-100 (expf(-x) overflows to inf at x < -88.7), +-0, and a cluster around the zero of silu'."""
    g = torch.Generator().manual_seed(seed)
    x = torch.linspace(-30.0, 30.0, n)[torch.randperm(n, generator=g)].to(F32) if n > 1 else torch.tensor([0.75], dtype=F32)
    sp = torch.tensor([87.0, -87.0, 100.0, -100.0, 0.0, -0.0, SILU_DZERO, SILU_DZERO + 1e-3, SILU_DZERO - 1e-3, -88.5, -89.0, 16.7, -16.7, 1e-30, -1e-30],
                      dtype=F32)
    k = min(n // 2, sp.numel())
    x[:k] = sp[:k]
    return x


def ulp_err(got, want64, scale64=None):
    """|got - want| in units of the float32 spacing at max(|want|, |scale|, 2^-80).  `scale`: the magnitude the result is
    accurate RELATIVE TO where that is not its own (a sum that cancels: its larger operand; silu' near its zero: |dy|).  The floor
    keeps values no training step can tell from zero (float32 denormals included) from being measured relative to themselves."""
    ref = want64.abs()
    if scale64 is not None:
        ref = torch.maximum(ref, scale64.abs())
    ref = ref.clamp_min(ULP_FLOOR).float()
    spacing = (torch.nextafter(ref, torch.full_like(ref, float("inf"))) - ref).double()
    return (got.double() - want64).abs() / spacing


# ---- SiLU backward ----------------------------------------------------------------------------------------------------------------
def silu_bwd64(x, dy, other=None):
    """dy * silu'(x) (+ other) from float64 autograd through x * sigmoid(x)."""
    xd = x.double().requires_grad_()
    (xd * torch.sigmoid(xd)).backward(dy.double())
    return xd.grad if other is None else xd.grad + other.double()


def silu_bwd_scale64(x, dy, other=None):
    """What silu_bwd is accurate relative to: |dy| within 1/4 of the zero of silu' (s (1 + x (1 - s)) cancels there), the larger
    operand of the closing addition with `other`."""
    near = (x.double() - SILU_DZERO).abs() <= 0.25
    sc = torch.where(near, dy.double().abs(), torch.zeros((), dtype=torch.float64))
    if other is not None:
        xd = x.double()
        s = torch.sigmoid(xd)
        sc = torch.maximum(sc, torch.maximum((dy.double() * s * (1 + xd * (1 - s))).abs(), other.double().abs()))
    return sc


def silu_bwd_f32(x, dy, other=None):
    s = 1.0 / (1.0 + torch.exp(-x))
    v = dy * (s * (1.0 + x * (1.0 - s)))
    return v if other is None else v + other


# ---- attention gate ------------------------------------------------------------------------------------------------------------------
def gate64(a, b, x):
    return a.double() * torch.sigmoid(b.double()) + x.double()


def gate_scale64(a, b, x):
    return torch.maximum((a.double() * torch.sigmoid(b.double())).abs(), x.double().abs())


def gate_f32(a, b, x):
    return a * (1.0 / (1.0 + torch.exp(-b))) + x


def silu64(v):
    return v.double() * torch.sigmoid(v.double())


def silu_f32(v):
    return v / (1.0 + torch.exp(-v))


def gate_bwd64(a, b, dout):
    """(da, db) from float64 autograd through a * sigmoid(b) + x."""
    ad, bd = a.double().requires_grad_(), b.double().requires_grad_()
    xd = torch.zeros_like(ad, requires_grad=True)
    (ad * torch.sigmoid(bd) + xd).backward(dout.double())
    assert torch.equal(xd.grad, dout.double())
    return ad.grad, bd.grad


def gate_bwd_db_scale64(a, b, dout):
    """db = dout a s (1 - s): for b > 0 the factor 1 - s cancels (s is within half an ulp of 1 from b = 17 on), so the product is
    accurate relative to the factor's largest value, |dout a| / 4, not to itself; for b <= 0 nothing cancels (scale 0)."""
    return torch.where(b.double() > 0, (dout.double() * a.double()).abs() * 0.25, torch.zeros((), dtype=torch.float64))


def gate_bwd_f32(a, b, dout):
    s = 1.0 / (1.0 + torch.exp(-b))
    return dout * s, dout * a * s * (1.0 - s)


# ---- GDN / IGDN backward, element-wise part ------------------------------------------------------------------------------------------
def gdn_inputs(n, seed):
    """(x, s, dy): s log-uniform over [1e-6, 1e3] with both ends present."""
    x, dy = randn((n,), seed, 2.0), randn((n,), seed + 1)
    g = torch.Generator().manual_seed(seed + 2)
    s = (10.0 ** (torch.rand(n, generator=g, dtype=torch.float64) * 9.0 - 6.0)).to(F32)
    if n >= 2:
        s[0], s[1] = 1e-6, 1e3
    return x, s, dy


def gdn_bwd_prep64(x, s, dy, inverse):
    """(d y / d x at fixed s, d y / d s) times dy, from float64 autograd through y = x * s^(+-1/2)."""
    xd, sd = x.double().requires_grad_(), s.double().requires_grad_()
    (xd * sd ** (0.5 if inverse else -0.5)).backward(dy.double())
    return xd.grad, sd.grad


def gdn_bwd_prep_f32(x, s, dy, inverse):
    root = sqrt_f32(s)
    rs = div_f32(1.0, root)
    if inverse:
        return dy * root, dy * x * (0.5 * rs)
    return dy * rs, dy * x * (-0.5 * rs * rs * rs)


# ---- non-negative re-parametrisation ------------------------------------------------------------------------------------------------
class _LowerBound(torch.autograd.Function):
    """max(p, bound) whose gradient passes where p >= bound or where it is negative (it pushes p up): the rule the reference puts
    in front of its squared parameters."""

    @staticmethod
    def forward(ctx, p, bound):
        ctx.save_for_backward(p, bound)
        return torch.max(p, bound)

    @staticmethod
    def backward(ctx, g):
        p, bound = ctx.saved_tensors
        return torch.where((p >= bound) | (g < 0), g, torch.zeros_like(g)), None


def reparam_inputs(n, seed, bound):
    """(p, dfolded) around `bound`: p == float32(bound) exactly, p just below / above it, p < bound with a gradient of each sign,
    gradients of exactly +-0."""
    p, d = randn((n,), seed, 0.5) + 0.3, randn((n,), seed + 1)
    b = float(f32(bound))
    head = [(b, 1.0), (b, -1.0), (b, 0.0), (b - 0.25, 1.0), (b - 0.25, -1.0), (b - 0.25, 0.0), (b - 0.25, -0.0), (b + 0.25, 0.0),
            (float(torch.nextafter(f32(b), f32(-1e9))), 2.0), (float(torch.nextafter(f32(b), f32(1e9))), 2.0), (-3.0, 1.0), (-3.0, -1.0)]
    k = min(n, len(head))
    for i in range(k):
        p[i], d[i] = head[i]
    return p, d


def reparam64(p, bound, pedestal):
    return torch.maximum(p.double(), f32(bound).double()) ** 2 - f32(pedestal).double()


def reparam_f32(p, bound, pedestal):
    v = torch.maximum(p, f32(bound))
    return v * v - f32(pedestal)


def reparam_bwd64(p, dfolded, bound, pedestal=0.0):
    pd = p.double().requires_grad_()
    (_LowerBound.apply(pd, f32(bound).double()) ** 2 - pedestal).backward(dfolded.double())
    return pd.grad


def reparam_bwd_f32(p, dfolded, bound):
    g = (2.0 * torch.maximum(p, f32(bound))) * dfolded
    return torch.where((p >= f32(bound)) | (g < 0), g, torch.zeros_like(g))


# ---- linear forms ------------------------------------------------------------------------------------------------------------------------
def axpby_f32(a, b, alpha, beta):
    return f32(alpha) * a + f32(beta) * b


def add3_f32(a, b, c):
    return (a + b) + c


def mse_bwd64(a, b, dloss):
    ad, bd = a.double().requires_grad_(), b.double().requires_grad_()
    ((ad - bd) ** 2).mean().backward(dloss.double().reshape(()))
    return ad.grad, bd.grad


def mse_bwd_f32(a, b, dloss):
    scale = torch.tensor(2.0 / float(a.numel()), dtype=torch.float64).to(F32)        # (float)(2.0 / (double)n)
    g = (a - b) * (scale * dloss.reshape(()))
    return g, -g


def clip_f32(x, norm, max_norm, eps):
    """x scaled by max_norm / (norm + eps) where that is < 1 (a NaN compares false: untouched)."""
    coef = div_f32(f32(max_norm), norm.reshape(()) + f32(eps))
    return x * coef if bool(coef < 1.0) else x.clone()


# ---- reductions: the error bounds ----------------------------------------------------------------------------------------------------------
def channel_sum_chain(n, hw):
    """Longest chain of float32 additions behind one output of channel_sum: the launcher cuts the batch into min(n, 16) chunks (one
    for n == 1), a thread adds ceil(n / chunks) * ceil(hw / 256) terms, an 8-level tree follows, then the chunks in order."""
    chunks = min(n, 16) if n > 1 else 1
    per = -(-n // chunks)
    return per * -(-hw // 256) + 8 + (chunks if chunks > 1 else 0), chunks


# ---- views with the values of a fresh tensor ----------------------------------------------------------------------------------------------
def views_of(t):
    """[(name, tensor)]: the same values as `t` behind (1) a channel slice of a wider tensor, (2) a transposed map -- both
    non-contiguous -- and (3) a contiguous view that starts one ELEMENT into its allocation (float32: only 4-byte aligned)."""
    out = []
    if t.dim() == 4:
        wide = torch.zeros((t.shape[0], t.shape[1] + 2) + tuple(t.shape[2:]), dtype=t.dtype, device=t.device)
        wide[:, 1:-1] = t
        out.append(("channel slice", wide[:, 1:-1]))
        out.append(("transposed map", t.transpose(-1, -2).contiguous().transpose(-1, -2)))
    elif t.dim() == 1:
        wide = torch.zeros(2 * t.numel(), dtype=t.dtype, device=t.device)
        wide[::2] = t
        out.append(("stride 2", wide[::2]))
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:] = t.reshape(-1)
    out.append(("offset 1", buf[1:].view(t.shape)))
    for name, v in out:
        assert torch.equal(v, t), name
    assert out[-1][1].storage_offset() == 1
    return out


# ---- soft assignment of the training quantizer: Gumbel soft-max backward, <dDeq, c_k> ---------------------------------------------------
EPS_F32 = float(torch.finfo(F32).eps)
TINY = 1e-300                                                        # keeps 0 / 0 out of a relative error whose scale is exactly zero


def row_tb(temperature, bound, m, hw, rows, dtype):
    """max(T_g, bound) of every row, g = (row / hw) % m; `bound` as the float32 a `float` kernel argument receives."""
    g = (torch.arange(rows) // hw) % m
    return torch.maximum(temperature.reshape(-1).to(dtype)[g], f32(bound).to(dtype))


def soft_bwd64(post_logits, raw_logits, u_gumbel, ds, dlogits, temperature, bound, m, hw):
    """(d dist [.., k], rowsum [..], dtrow [..]) of one soft assignment from float64 autograd through the mathematics:
        tb = max(T_g, bound) per ROW, a leaf of its own per row, so that its gradient is the row's temperature term
        raw = (-dist / sqrt(k)) tb, dist a leaf (its value follows from the given raw logits)
        p = post + (raw - raw.detach()): the random drop adds a constant; the given float32 post-drop values are used exactly
        y = softmax(p - log(-log(clamp(u, eps32, 1 - eps32)))),   loss = sum y dS (+ sum p dlogits)
    `raw_logits`: the logits before the drop, always (a kernel may be handed less).  rowsum = sum_k d dist[k]."""
    k = post_logits.shape[-1]
    post, raw0 = post_logits.double().reshape(-1, k), raw_logits.double().reshape(-1, k)
    rows = post.shape[0]
    tb = row_tb(temperature, bound, m, hw, rows, torch.float64).clone().requires_grad_()
    root = torch.tensor(float(k), dtype=torch.float64).sqrt()
    dist = (-raw0 * root / tb.detach()[:, None]).requires_grad_()
    raw = (-dist / root) * tb[:, None]
    p = post + (raw - raw.detach())
    gumbel = -torch.log(-torch.log(u_gumbel.double().reshape(-1, k).clamp(EPS_F32, 1.0 - EPS_F32)))
    y = torch.softmax(p + gumbel, -1)
    loss = (y * ds.double().reshape(-1, k)).sum()
    if dlogits is not None:
        loss = loss + (p * dlogits.double().reshape(-1, k)).sum()
    loss.backward()
    lead = post_logits.shape[:-1]
    return dist.grad.reshape(post_logits.shape), dist.grad.sum(-1).reshape(lead), tb.grad.reshape(lead)


def soft_bwd_f32(post_logits, raw_logits, u_gumbel, ds, dlogits, temperature, bound, m, hw):
    """The same three results from the backward formulas written out, every operation in float32 (sums by torch.sum):
        dz = y (dS - <y, dS>) (+ dlogits),  d dist = dz (-tb / sqrt(k)),  dtrow = sum_k dz raw / tb,  rowsum = sum_k d dist."""
    k = post_logits.shape[-1]
    post, raw, dsv = post_logits.reshape(-1, k), raw_logits.reshape(-1, k), ds.reshape(-1, k)
    assert post.dtype == F32 and raw.dtype == F32 and dsv.dtype == F32 and u_gumbel.dtype == F32
    tb = row_tb(temperature, bound, m, hw, post.shape[0], F32)[:, None]
    u = u_gumbel.reshape(-1, k).clamp(EPS_F32, 1.0 - EPS_F32)
    z = post + -torch.log(-torch.log(u))
    e = torch.exp(z - z.max(-1, keepdim=True)[0])
    inv = 1.0 / e.sum(-1, keepdim=True)
    dot = (e * dsv).sum(-1, keepdim=True) * inv
    dz = (e * inv) * (dsv - dot)
    if dlogits is not None:
        dz = dz + dlogits.reshape(-1, k)
    dd = dz * (-tb / torch.tensor(float(k), dtype=torch.float64).sqrt().to(F32))
    dt = (dz * (raw / tb)).sum(-1)
    lead = post_logits.shape[:-1]
    return dd.reshape(post_logits.shape), dd.sum(-1).reshape(lead), dt.reshape(lead)


def soft_bwd_scales64(ddist64, raw_logits, temperature, bound, m, hw):
    """What the three results are accurate relative to: d dist to the largest |d dist| of its row; rowsum -- a sum that cancels,
    analytically to zero without dlogits -- to sum_k |d dist[k]|; dtrow, which cancels the same way, to sum_k |dz[k] raw[k] / tb|."""
    k = ddist64.shape[-1]
    dd, raw = ddist64.reshape(-1, k), raw_logits.double().reshape(-1, k)
    tb = row_tb(temperature, bound, m, hw, dd.shape[0], torch.float64)[:, None]
    dz = dd / (-tb / torch.tensor(float(k), dtype=torch.float64).sqrt())
    lead = ddist64.shape[:-1]
    return (dd.abs().max(-1, keepdim=True)[0].reshape(lead + (1,)), dd.abs().sum(-1).reshape(lead), (dz * raw / tb).abs().sum(-1).reshape(lead))


def scaled_err(got, want64, scale64, where=None):
    """max |got - want| / scale (over the rows `where` selects)."""
    assert torch.isfinite(got).all(), "non-finite result"
    err = (got.double() - want64).abs() / scale64.clamp_min(TINY)
    if where is not None:
        err = err[where]
    return float(err.max())


def soft_bwd_errs(got, want64, scales64, dtrow_rows=None):
    """(d dist, rowsum, dtrow) errors of a result triple in the scales above; `dtrow_rows`: the rows whose dtrow counts."""
    return (scaled_err(got[0], want64[0], scales64[0]), scaled_err(got[1], want64[1], scales64[1]),
            scaled_err(got[2], want64[2], scales64[2], dtrow_rows))


def inner64(x, codebook):
    """<x_v, c_k> -> [n, m, h, w, k] in float64, x [n, m d, h, w], codebook [m, k, d]."""
    m, k, d = codebook.shape
    n, _, h, w = x.shape
    return torch.einsum("ngdhw,gkd->nghwk", x.double().reshape(n, m, d, h, w), codebook.double())


def inner_scale64(x, codebook):
    """sum_j |x_j c_kj|: what a d-term inner product is accurate relative to."""
    return inner64(x.abs(), codebook.abs())


def inner_f32(x, codebook):
    """The inner product as a float32 chain in channel order, product and addition rounded separately."""
    m, k, d = codebook.shape
    n, _, h, w = x.shape
    xv = x.reshape(n, m, d, h, w)
    acc = torch.zeros((n, m, h, w, k), dtype=F32)
    for j in range(d):
        acc = acc + xv[:, :, j, :, :, None] * codebook[None, :, None, None, :, j]
    return acc


# ---- GroupNorm (csrc/norm.hip) ------------------------------------------------------------------------------------------------------------
# gamma / beta None mean 1 / 0.  A run = the cg * h * w elements one (image, group) normalises over; statistics come back as [n, groups].
def _per_channel(p, c, dtype, fill):
    return (torch.full((c,), fill, dtype=dtype) if p is None else p.to(dtype)).reshape(1, c, 1, 1)


def _gn_forward(x, gamma, beta, groups, eps, sqrt, div):
    """The definition in x's dtype: mean, then centred squares (biased), y = (x - mean) rstd gamma + beta."""
    n, c, h, w = x.shape
    runs = x.reshape(n, groups, -1)
    count = runs.shape[-1]
    mean = div(runs.sum(-1), torch.tensor(float(count), dtype=x.dtype))
    centred = runs - mean[..., None]
    var = div((centred * centred).sum(-1), torch.tensor(float(count), dtype=x.dtype))
    rstd = div(torch.ones((), dtype=x.dtype), sqrt(var + f32(eps).to(x.dtype)))          # eps as the float32 the kernel receives
    xhat = (centred * rstd[..., None]).reshape(x.shape)
    return xhat * _per_channel(gamma, c, x.dtype, 1.0) + _per_channel(beta, c, x.dtype, 0.0), mean, rstd, xhat


def group_norm64(x, gamma, beta, groups, eps):
    """(y, mean [n, groups], rstd [n, groups], silu(y)) in float64."""
    y, mean, rstd, _ = _gn_forward(x.double(), gamma, beta, groups, eps, torch.sqrt, lambda a, b: a / b)
    return y, mean, rstd, silu64(y)


def group_norm_f32(x, gamma, beta, groups, eps):
    """The same definition with every operation rounded to float32 (sums by torch.sum) -- one rounding per operation where the kernel fuses its last two."""
    assert x.dtype == F32
    y, mean, rstd, _ = _gn_forward(x, gamma, beta, groups, eps, sqrt_f32, div_f32)
    return y, mean, rstd, silu_f32(y)


def group_norm_bwd64(x, dy, gamma, groups, eps):
    """(dx, dgamma, dbeta) from float64 autograd through the definition."""
    c = x.shape[1]
    xd = x.double().requires_grad_()
    gd = (torch.ones(c, dtype=torch.float64) if gamma is None else gamma.double()).requires_grad_()
    bd = torch.zeros(c, dtype=torch.float64, requires_grad=True)
    _gn_forward(xd, gd, bd, groups, eps, torch.sqrt, lambda a, b: a / b)[0].backward(dy.double())
    return xd.grad, gd.grad, bd.grad


def group_norm_bwd_f32(x, dy, gamma, groups, eps):
    """The centred backward formulas, every operation in float32, on the float32 definition's own statistics:
        dx = rstd (g dy - mean_run(g dy) - xhat mean_run(g dy xhat)),  dgamma = sum_n sum_p dy xhat,  dbeta = sum_n sum_p dy."""
    assert x.dtype == F32 and dy.dtype == F32
    n, c, h, w = x.shape
    _, _, rstd, xhat = _gn_forward(x, None, None, groups, eps, sqrt_f32, div_f32)
    gdy = dy * _per_channel(gamma, c, F32, 1.0)
    count = torch.tensor(float(c // groups * h * w), dtype=F32)
    m1 = div_f32(gdy.reshape(n, groups, -1).sum(-1), count)[..., None]
    m2 = div_f32((gdy * xhat).reshape(n, groups, -1).sum(-1), count)[..., None]
    dx = (rstd[..., None] * (gdy.reshape(n, groups, -1) - m1 - xhat.reshape(n, groups, -1) * m2)).reshape(x.shape)
    return dx, (dy * xhat).sum((0, 2, 3)), dy.sum((0, 2, 3))


def group_norm_scales64(x, dy, gamma, beta, groups, eps):
    """What each result is accurate relative to (a sum that cancels: the sum of its terms' magnitudes), as tensors that broadcast
    against the result: y / silu(y) -- the run's max |y64|; mean -- |mean64| + the run's standard deviation; rstd -- itself;
    dx -- the run's rstd64 max |gamma dy|; dgamma[c] -- sum |dy xhat|; dbeta[c] -- sum |dy|."""
    n, c, h, w = x.shape
    xd = x.double()
    y, mean, rstd, _ = group_norm64(x, gamma, beta, groups, eps)
    runs = xd.reshape(n, groups, -1)
    sigma = ((runs - mean[..., None]) ** 2).mean(-1).sqrt()
    xhat = ((runs - mean[..., None]) * rstd[..., None]).reshape(x.shape)
    per_run = lambda t: t.reshape(n, groups, -1).abs().max(-1)[0].repeat_interleave(c // groups, 1).reshape(n, c, 1, 1)
    gdy = dy.double() * _per_channel(gamma, c, torch.float64, 1.0)
    return dict(y=per_run(y), mean=mean.abs() + sigma, rstd=rstd,
                dx=per_run(gdy) * rstd.repeat_interleave(c // groups, 1).reshape(n, c, 1, 1),
                dgamma=(dy.double() * xhat).abs().sum((0, 2, 3)), dbeta=dy.double().abs().sum((0, 2, 3)))


GN_REGIMES = ("plain", "biased", "bias_dominated", "bias_dominated_dy1", "channel_offsets", "quiet", "large", "outlier", "outlier_first")
_GN_X = dict(plain=(0.3, 1.5, 0.4), biased=(10.0, 1.0, 1.0), bias_dominated=(10.0, 0.1, 1.0), bias_dominated_dy1=(10.0, 0.1, 1.0),
             channel_offsets=(0.0, 0.1, 1.0), quiet=(0.0, 1e-3, 1e-3), large=(0.0, 1e4, 5e3), outlier=(0.0, 1.0, 0.5), outlier_first=(0.0, 1.0, 0.5))


def gn_case(shape, groups, regime, seed, constant_run=False, affine=True):
    """(x, dy, gamma, beta) of one GroupNorm case.  x = mean + sigma N(0, 1) per regime (_GN_X: mean, sigma, step), image i moved by
    (i % 7) step and spread by 1 + (i % 4) / 4 so that neighbouring images of a batch share neither mean nor rstd; `channel_offsets` adds 5 N(0, 1) per channel (only meaningful
    with more than one channel per group); `outlier` sets one element of image 0's first run to 1e3, `outlier_first` the FIRST element of every run of image 0; dy ~ N(0, 1), plus 1 in
    `bias_dominated_dy1`.  `constant_run`: the last run of the last image is 2.5 throughout.  gamma, beta ~ N(0, 1) of mixed sign."""
    n, c, h, w = shape
    g = torch.Generator().manual_seed(seed)
    mean, sigma, step = _GN_X[regime]
    img = torch.arange(n, dtype=F32).reshape(n, 1, 1, 1)
    x = torch.randn(shape, generator=g) * (sigma * (1.0 + 0.25 * (img % 4))) + mean + (img % 7) * step
    if regime == "channel_offsets":
        assert c // groups > 1
        x = x + 5.0 * torch.randn((1, c, 1, 1), generator=g)
    if regime == "outlier":
        x.view(-1)[(h * w) // 2] = 1e3
    if regime == "outlier_first":                                    # (where a kernel that shifts by a sample of the run would take it)
        x.reshape(n, groups, -1)[0, :, 0] = 1e3
    dy = torch.randn(shape, generator=g) + (1.0 if regime == "bias_dominated_dy1" else 0.0)
    gamma, beta = torch.randn(c, generator=g), torch.randn(c, generator=g)
    if constant_run:
        x.reshape(n, groups, -1)[n - 1, groups - 1] = 2.5
    return x.to(F32).contiguous(), dy.to(F32).contiguous(), (gamma if affine else None), (beta if affine else None)
