"""CPU: the references of tests/test_gpu_leaf_ops.py checked against each other.  Every hand-written float32 restatement of a
backward formula (tests/_leaf_refs.py, `*_f32`) must agree with float64 torch.autograd through the FORWARD formula on the same
special-value inputs the GPU tests use -- a wrong restatement would otherwise bless a wrong kernel -- and the soundness walk of
mcquic_amd.autograd in front of a deferred backward is exercised on CPU graphs."""
import pytest
import torch

import _leaf_refs as R

N = 20000


def _worst(got32, want64, scale64=None):
    assert torch.isfinite(got32).all()
    return float(R.ulp_err(got32, want64, scale64).max())


def test_silu_backward_restatement():
    """s (1 + x (1 - s)) op by op in float32 against float64 autograd through x * sigmoid(x) (|dy| ulps next to the zero of silu'),
    finite at +-87 / +-100 where exp(-x) overflows.  The formula is not a few-ulp one: for 8 < x < 17.4 (beyond that s == 1 and
    the term is gone) 1 - s carries s's absolute error, up to an ulp of 1, and x multiplies it -- up to 17.4 ulp(1) / 2 against a
    result near 1, i.e. ~17 ulp of the result's spacing 2^-23... measured 16.5 at x = 16.6.  32 = that with the other four roundings;
    a wrong formula is off by millions."""
    x, dy, other = R.special_x(N, 1), R.randn((N,), 2), R.randn((N,), 3)
    assert _worst(R.silu_bwd_f32(x, dy), R.silu_bwd64(x, dy), R.silu_bwd_scale64(x, dy)) <= 32.0
    assert _worst(R.silu_bwd_f32(x, dy, other), R.silu_bwd64(x, dy, other), R.silu_bwd_scale64(x, dy, other)) <= 32.0
    assert _worst(R.silu_bwd_f32(x, dy).neg(), R.silu_bwd64(x, dy), R.silu_bwd_scale64(x, dy)) > 1e6
    # the zero of silu' really is where the helper says
    z = torch.tensor([R.SILU_DZERO], dtype=torch.float64)
    assert float(R.silu_bwd64(z, torch.ones(1, dtype=torch.float64)).abs()) < 1e-15


def test_gate_restatements():
    a, b, x, g = R.randn((N,), 4), R.special_x(N, 5), R.randn((N,), 6), R.randn((N,), 7)
    assert _worst(R.gate_f32(a, b, x), R.gate64(a, b, x), R.gate_scale64(a, b, x)) <= 8.0
    da64, db64 = R.gate_bwd64(a, b, g)
    da, db = R.gate_bwd_f32(a, b, g)
    assert _worst(da, da64) <= 8.0
    assert _worst(db, db64, R.gate_bwd_db_scale64(a, b, g)) <= 8.0
    v = R.special_x(N, 8)
    assert _worst(R.silu_f32(v), R.silu64(v)) <= 8.0


def test_gdn_backward_restatement():
    """1 / sqrt(s), then at most five multiplications: within 8 ulp of float64 autograd through x s^-1/2 and x s^1/2 over s in
    [1e-6, 1e3]; and the sign and power that a wrong constant would change show up as a gross error."""
    x, s, dy = R.gdn_inputs(N, 9)
    assert float(s.min()) == float(R.f32(1e-6)) and float(s.max()) == float(R.f32(1e3))
    for inverse in (False, True):
        dxd64, ds64 = R.gdn_bwd_prep64(x, s, dy, inverse)
        dxd, ds = R.gdn_bwd_prep_f32(x, s, dy, inverse)
        assert _worst(dxd, dxd64) <= 8.0 and _worst(ds, ds64) <= 8.0
        assert _worst(-ds, ds64) > 1e6 and _worst(R.gdn_bwd_prep_f32(x, s, dy, not inverse)[1], ds64) > 1e6


def test_reparam_restatements():
    """max(p, bound)^2 - pedestal and its gradient under the LowerBound rule: the float32 restatement takes the same BRANCH as
    float64 autograd on every element (p == bound, p < bound with either sign of gradient, zero gradients) and the same value
    within 2 ulp (two roundings)."""
    bound, pedestal = 0.2, 2.0 ** -36
    p, d = R.reparam_inputs(N, 10, bound)
    b32 = float(R.f32(bound))
    assert int((p == b32).sum()) >= 3 and int(((p < b32) & (d > 0)).sum()) > 10 and int(((p < b32) & (d < 0)).sum()) > 10 and int((d == 0).sum()) >= 4
    assert _worst(R.reparam_f32(p, bound, pedestal), R.reparam64(p, bound, pedestal), R.f32(pedestal).double().expand(N)) <= 2.0
    want = R.reparam_bwd64(p, d, bound, pedestal)
    got = R.reparam_bwd_f32(p, d, bound)
    assert torch.equal(got == 0, want == 0)
    assert _worst(got, want) <= 2.0
    # the rule itself, spelled out: at the bound the gradient passes, below it only a negative one does
    q, e = torch.tensor([b32, b32, b32 - 0.25, b32 - 0.25], dtype=R.F32), torch.tensor([1.0, -1.0, 1.0, -1.0])
    assert torch.equal(R.reparam_bwd_f32(q, e, bound) != 0, torch.tensor([True, True, False, True]))
    assert torch.equal(R.reparam_bwd64(q, e, bound) != 0, torch.tensor([True, True, False, True]))


def test_linear_restatements():
    a, b, c = R.randn((N,), 11), R.randn((N,), 12), R.randn((N,), 13)
    dl = torch.tensor(0.37, dtype=R.F32)
    da64, db64 = R.mse_bwd64(a, b, dl)
    da, db = R.mse_bwd_f32(a, b, dl)
    assert _worst(da, da64) <= 3.0 and _worst(db, db64) <= 3.0           # (the difference, the scale's two roundings, the product)
    assert _worst(R.axpby_f32(a, b, 0.3, -1.7), 0.3 * a.double() + -1.7 * b.double(),
                  torch.maximum(a.double().abs() * 0.3, b.double().abs() * 1.7)) <= 2.5
    assert _worst(R.add3_f32(a, b, c), a.double() + b.double() + c.double(), a.double().abs() + b.double().abs() + c.double().abs()) <= 1.0     # (two roundings, each half an ulp of a partial sum)
    x = R.randn((N,), 14)
    norm = x.double().pow(2).sum().sqrt().float()
    assert torch.equal(R.clip_f32(x, norm, 1e9, 1e-6), x)
    clipped = R.clip_f32(x, norm, 1.0, 1e-6)
    assert abs(float(clipped.double().pow(2).sum().sqrt()) - 1.0) < 1e-5
    assert torch.equal(R.clip_f32(x, torch.tensor(float("nan")), 1.0, 1e-6), x)


def test_channel_sum_chain_follows_the_launcher():
    assert R.channel_sum_chain(1, 1) == (1 + 8, 1)
    assert R.channel_sum_chain(1, 4096) == (16 + 8, 1)
    assert R.channel_sum_chain(2, 257) == (2 + 8 + 2, 2)
    assert R.channel_sum_chain(35, 9) == (3 + 8 + 16, 16)


def test_views_have_the_values_and_the_layouts():
    t = R.randn((2, 5, 6, 8), 15)
    names = {}
    for name, v in R.views_of(t):
        assert torch.equal(v, t)
        names[name] = v
    assert not names["channel slice"].is_contiguous() and not names["transposed map"].is_contiguous()
    assert names["offset 1"].is_contiguous() and names["offset 1"].data_ptr() % 8 == 4
    flat = dict(R.views_of(t.flatten()))
    assert not flat["stride 2"].is_contiguous() and flat["offset 1"].data_ptr() % 8 == 4


class _Defers(torch.autograd.Function):
    """Stand-in for a node whose backward defers the gradients of its inputs 1 and 2 (ConvFn's weight and bias)."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(x, w)
        ctx.wgrad_slots = (1, 2)
        return x * w + b

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        return g * w, g * x, g


def test_deferral_walk_refuses_shared_and_derived_weights():
    """mcquic_amd.autograd._leaves_take_by_stealing on CPU graphs: a leaf reached alone by deferred edges passes; a weight read by
    two deferring nodes, by a deferring node and a torch op, or handed over as the output of a torch op does not; a parameter that
    two ordinary torch ops read (no deferred edge) does not stop deferral."""
    from mcquic_amd.autograd import _leaves_take_by_stealing as ok
    x = torch.randn(4, requires_grad=True)
    w, b, w2, b2 = (torch.randn(4, requires_grad=True) for _ in range(4))
    assert ok([_Defers.apply(_Defers.apply(x, w, b), w2, b2).sum()])
    assert not ok([_Defers.apply(_Defers.apply(x, w, b), w, b2).sum()])              # tied weights
    assert not ok([(_Defers.apply(x, w, b) * w).sum()])                               # a second, ordinary reader
    assert not ok([_Defers.apply(x, w * torch.ones(4), b).sum()])                     # a derived weight
    assert not ok([_Defers.apply(x, w, b * 1.0).sum()])                               # a derived bias
    assert ok([(_Defers.apply(x * w2, w, b) * w2).sum()])                             # two readers, neither deferred
    assert ok([_Defers.apply(x, w.detach(), b).sum()])                                # a frozen weight has no edge at all
    w.grad = torch.zeros(4)
    assert not ok([_Defers.apply(x, w, b).sum()])                                     # accumulation onto an existing .grad


# ---- soft assignment: the float64 reference is the oracle's own derivative ----------------------------------------------------------------
def _oracle_soft_case(k, seed):
    """Float64 inputs of one level: (x, codebook, temperature [m,1,1,1] with group 1 below `bound`, bound, freq, u_drop, u_gumbel,
    dS, W) on 30 latent vectors (n, m, h, w = 2, 3, 1, 5).  The Gumbel draw is float32's grid clamped to [eps32, 1 - eps32]: the
    oracle in float64 would clamp at float64's eps where soft_bwd64 clamps at float32's, as the kernels do."""
    m, d, n, h, w = 3, 4, 2, 1, 5
    g = torch.Generator().manual_seed(seed)
    cb = (torch.randn((m, k, d), generator=g) * (2 / (5 * d)) ** 0.5).double()
    x = (torch.randn((n, m * d, h, w), generator=g) * 0.5).double()
    temp = torch.tensor([1.3, 0.2, 0.8], dtype=torch.float64).reshape(m, 1, 1, 1)
    freq = (torch.rand((m, k), generator=g) ** 3 + 1e-3) * (torch.rand((m, k), generator=g) < 0.5)      # half the codes unused: the
    freq = (freq / freq.sum(-1, keepdim=True)).double()                  # drop's exponent grows, a fifth of the entries is dropped
    shape = (n, m, h, w, k)
    u1 = torch.rand(shape, generator=g).double()
    u2 = torch.rand(shape, generator=g).clamp(R.EPS_F32, 1.0 - R.EPS_F32).double()
    ds = (torch.randn(shape, generator=g) * 0.1).double()
    wl = ((torch.rand(shape, generator=g) - 0.5) * 0.05).double()
    return x, cb, temp, 0.5, freq, u1, u2, ds, wl, m, h * w


@pytest.mark.parametrize("with_dlogits", [False, True])
@pytest.mark.parametrize("k", [8, 65, 513])
def test_soft_bwd64_is_the_oracles_own_derivative(monkeypatch, k, with_dlogits):
    """oracle.mcquic_ref's vq_logit -> random_drop -> gumbel_softmax_hard in float64 with loss sum sample dS (+ sum logit W): its
    autograd gradients with respect to the distance and to max(temperature, bound) -- per group: the temperature's own where it is
    above the bound, the bound's where it is not -- equal R.soft_bwd64's d dist and the group sums of its dtrow to 1e-12 of the
    largest value.  That ties the reference of tests/test_gpu_soft_assign_leaf.py to the oracle, which test_oracle_vs_reference.py
    ties to the reference implementation."""
    from oracle import mcquic_ref as O
    x, cb, temp, bound, freq, u1, u2, ds, wl, m, hw = _oracle_soft_case(k, 700 + k)
    seen = []
    distance = O.vq_distance

    def kept(*a):
        out = distance(*a)
        out.retain_grad()
        seen.append(out)
        return out

    monkeypatch.setattr(O, "vq_distance", kept)
    x.requires_grad_()
    temp.requires_grad_()
    bnd = torch.tensor([bound], dtype=torch.float64, requires_grad=True)
    raw = O.vq_logit(x, cb, temp, bnd)
    post = O.random_drop(raw, freq, u1)
    assert 0.05 < float((post < -1e8).double().mean()) < 0.5              # the drop is there, and is not everything
    sample, _, _ = O.gumbel_softmax_hard(post, u2)
    loss = (sample * ds).sum() + ((post * wl).sum() if with_dlogits else 0.0)
    loss.backward()
    (dist,) = seen
    dd, rowsum, dtrow = R.soft_bwd64(post.detach(), raw.detach(), u2, ds, wl if with_dlogits else None, temp.detach(), bound, m, hw)
    assert float((dd - dist.grad).abs().max()) <= 1e-12 * float(dist.grad.abs().max())
    assert float((rowsum - dist.grad.sum(-1)).abs().max()) <= 1e-12 * float(dist.grad.abs().sum(-1).max())
    per_group = dtrow.sum((0, 2, 3))                                      # [n, m, h, w] -> [m]
    want = torch.stack([temp.grad.reshape(-1)[0], bnd.grad[0], temp.grad.reshape(-1)[2]])
    assert float(temp.grad.reshape(-1)[1]) == 0.0                         # group 1 sits below the bound
    assert float((per_group - want).abs().max()) <= 1e-12 * float(want.abs().max())


@pytest.mark.parametrize("k", [8, 65, 513])
def test_soft_bwd_restatement(k):
    """R.soft_bwd_f32 (the backward formulas, float32 throughout) against R.soft_bwd64 (autograd, float64) on float32 inputs, in
    the scales of R.soft_bwd_scales64.  Bar: 8 (k + 64) 2^-24 -- k 2^-24 is the worst-case bound of a k-term float32 sum relative to
    the sum of its terms' magnitudes, 64 2^-24 stands for the soft-max's exponent (|logit + noise - max| <= 40, rounded at that
    size, is that much relative error in y), 8 for the handful of such steps in a row.  A wrong sign is off by order one."""
    x, cb, temp, bound, freq, u1, u2, ds, wl, m, hw = _oracle_soft_case(k, 800 + k)
    from oracle import mcquic_ref as O
    raw = O.vq_logit(x.float(), cb.float(), temp.float(), torch.tensor([bound]))
    post = O.random_drop(raw, freq.float(), u1.float())
    for dl in (None, wl.float()):
        args = (post, raw, u2.float(), ds.float(), dl, temp.float(), bound, m, hw)
        want = R.soft_bwd64(*args)
        scales = R.soft_bwd_scales64(want[0], raw, temp.float(), bound, m, hw)
        errs = R.soft_bwd_errs(R.soft_bwd_f32(*args), want, scales)
        assert max(errs) <= 8 * (k + 64) * 2.0 ** -24, errs
        flipped = tuple(-t for t in R.soft_bwd_f32(*args))
        assert min(R.soft_bwd_errs(flipped, want, scales)[::2]) > 0.1     # (rowsum may vanish: d dist and dtrow do not)


def test_inner_restatement():
    """R.inner_f32, a float32 chain over d channels, against R.inner64: within (d + 1) 2^-24 of sum_j |x_j c_kj|, the standard bound
    of a d-term inner product (Higham, Accuracy and Stability of Numerical Algorithms, 3.1)."""
    for m, k, d, n, h, w in ((2, 40, 64, 1, 2, 3), (3, 7, 1, 2, 1, 1), (1, 130, 10, 1, 3, 3)):
        x, cb = R.randn((n, m * d, h, w), 900 + d), R.randn((m, k, d), 901 + d, 0.3)
        want = R.inner64(x, cb)
        assert want.shape == (n, m, h, w, k)
        assert R.scaled_err(R.inner_f32(x, cb), want, R.inner_scale64(x, cb)) <= (d + 1) * 2.0 ** -24
        assert torch.allclose(want[0, m - 1, h - 1, 0, k - 1], (x.double()[0, (m - 1) * d:, h - 1, 0] * cb.double()[m - 1, k - 1]).sum(), rtol=1e-13)


# ---- GroupNorm: the references of tests/test_gpu_group_norm_leaf.py ---------------------------------------------------------------------
GN_SHAPES = ((3, 8, 5, 51, 2), (2, 4, 1, 8193, 2), (2, 6, 1, 1, 3), (1, 4, 3, 5, 2), (5, 8, 16, 16, 4))


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("sg", GN_SHAPES)
def test_group_norm_references_are_torch_group_norm(sg, affine):
    """group_norm64 / group_norm_bwd64 (the definition written out, autograd through it) against torch.nn.functional.group_norm in
    float64 to 1e-12 in the scales of R.group_norm_scales64, with and without gamma / beta, on the cancelling regime too.  (The scales,
    not each tensor's largest entry: ATen's own backward forms (ds - mean db) rstd, and in `bias_dominated_dy1` on runs of 16386
    elements that difference of two sums of 1.6e5 leaves 1e-9 of absolute error in a dgamma of 190 -- in float64.)"""
    for regime in ("plain", "bias_dominated_dy1"):
        x, dy, gamma, beta = R.gn_case(sg[:4], sg[4], regime, 17, affine=affine)
        c = sg[1]
        xd = x.double().requires_grad_()
        gd, bd = (None, None) if not affine else (gamma.double().requires_grad_(), beta.double().requires_grad_())
        want = torch.nn.functional.group_norm(xd, sg[4], gd, bd, float(R.f32(1e-5)))
        want.backward(dy.double())
        y, mean, rstd, twin = R.group_norm64(x, gamma, beta, sg[4], 1e-5)
        dx, dgamma, dbeta = R.group_norm_bwd64(x, dy, gamma, sg[4], 1e-5)
        assert mean.shape == rstd.shape == (sg[0], sg[4])
        pairs = [(y, want.detach()), (dx, xd.grad), (twin, torch.nn.functional.silu(want.detach()))]
        if affine:
            pairs += [(dgamma, gd.grad), (dbeta, bd.grad)]
        else:                                                        # (the gradients of the implied gamma = 1, beta = 0)
            xhat = torch.nn.functional.group_norm(x.double(), sg[4], None, None, float(R.f32(1e-5)))
            pairs += [(dgamma, (dy.double() * xhat).sum((0, 2, 3))), (dbeta, dy.double().sum((0, 2, 3)))]
        sc = R.group_norm_scales64(x, dy, gamma, beta, sg[4], 1e-5)
        for (got, ref), scale in zip(pairs, (sc["y"], sc["dx"], sc["y"], sc["dgamma"], sc["dbeta"])):
            assert got.dtype == torch.float64 and got.shape == ref.shape
            assert R.scaled_err(got, ref, scale.expand_as(ref)) <= 1e-12
        runs = x.double().reshape(sg[0], sg[4], -1)
        assert torch.allclose(mean, runs.mean(-1), rtol=0, atol=1e-12 * float(runs.abs().max()))
        assert torch.allclose(rstd, 1.0 / torch.sqrt(runs.var(-1, unbiased=False) + float(R.f32(1e-5))), rtol=1e-12, atol=0)


@pytest.mark.parametrize("regime", R.GN_REGIMES)
@pytest.mark.parametrize("sg", GN_SHAPES[:2] + GN_SHAPES[4:])
def test_group_norm_float32_definition(sg, regime):
    """The float32 definition (group_norm_f32 / group_norm_bwd_f32: the yardstick of the GPU bars) against float64 in every input
    regime, in the scales of R.group_norm_scales64.  Its error has two sources: a few roundings at the scale of the result (u = 2^-24
    each), and the rounding of the mean -- up to u max |x| -- seen from the run's 1 / rstd, i.e. u kappa with kappa = max |x| rstd
    (100 .. 170 in the bias-dominated regimes, sqrt(count) with one outlier).  So: mean, rstd and dbeta, which never see xhat,
    within 8 u; everything built on xhat within 8 u (1 + kappa).  A sign error or a dropped term is off by O(1)."""
    u = 2.0 ** -24
    groups = sg[4]
    x, dy, gamma, beta = R.gn_case(sg[:4], groups, regime, 23)
    y64, mean64, rstd64, silu64 = R.group_norm64(x, gamma, beta, groups, 1e-5)
    dx64, dg64, db64 = R.group_norm_bwd64(x, dy, gamma, groups, 1e-5)
    sc = R.group_norm_scales64(x, dy, gamma, beta, groups, 1e-5)
    y, mean, rstd, silu = R.group_norm_f32(x, gamma, beta, groups, 1e-5)
    dx, dg, db = R.group_norm_bwd_f32(x, dy, gamma, groups, 1e-5)
    kappa = float((x.double().reshape(sg[0], groups, -1).abs().max(-1)[0] * rstd64).max())
    for name, got, want, scale, bound in (("y", y, y64, sc["y"], 8 * u * (1 + kappa)), ("silu", silu, silu64, sc["y"], 8 * u * (1 + kappa)),
                                          ("mean", mean, mean64, sc["mean"], 8 * u), ("rstd", rstd, rstd64, sc["rstd"], 8 * u),
                                          ("dx", dx, dx64, sc["dx"], 8 * u * (1 + kappa)), ("dgamma", dg, dg64, sc["dgamma"], 8 * u * (1 + kappa)),
                                          ("dbeta", db, db64, sc["dbeta"], 8 * u)):
        assert got.dtype == R.F32
        err = R.scaled_err(got, want, scale.expand_as(want))
        assert err <= bound, (name, err, bound, kappa)
    assert R.scaled_err(-dx, dx64, sc["dx"].expand_as(dx64)) > 0.1 and R.scaled_err(dg.flip(0), dg64, sc["dgamma"]) > 1e-3
