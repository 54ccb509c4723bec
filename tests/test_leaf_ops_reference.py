"""CPU: the references of tests/test_gpu_leaf_ops.py checked against each other.  Every hand-written float32 restatement of a
backward formula (tests/_leaf_refs.py, `*_f32`) must agree with float64 torch.autograd through the FORWARD formula on the same
special-value inputs the GPU tests use -- a wrong restatement would otherwise bless a wrong kernel -- and the soundness walk of
mcquic_amd.autograd in front of a deferred backward is exercised on CPU graphs."""
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
