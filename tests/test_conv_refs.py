"""CPU: the references of tests/_conv_refs.py against torch's own operations and float64 autograd, so that a GPU test built on
them cannot bless a kernel with a reference that is wrong the same way.

  * out64 of every epilogue equals the torch operation (F.silu, torch.sigmoid, F.pixel_shuffle) or autograd through the forward
    formula (x rsqrt(s), x sqrt(s), a sigmoid(s) + x for the three backward pairs; z silu(m) for * silu'(m));
  * out_f32 stays within a few float32 roundings of out64 in out_scale64's scale (a restatement with a wrong constant or a dropped
    res_scale would be off by far more);
  * conv_seq_f32 agrees with conv64 within the chain's standard bound (K + 1) 2^-24 conv_scale64;
  * dgrad2_weight's filter, stored through PixelShuffle(2), is autograd's input gradient of the stride-2 convolution."""
import os

import pytest
import torch
import torch.nn.functional as F

import _conv_refs as C
import _leaf_refs as R

U = 2.0 ** -24            # unit roundoff of float32


def _sides(shape, seed):
    t = lambda i, s=1.0: R.randn(shape, seed + i, s)          # noqa: E731
    return dict(res=t(1), mul=t(2), dsilu_mul=t(3, 2.0), gate_mul=t(4, 2.0), gate_id=t(5, 0.5), gdn_mul=t(6, 2.0), igdn_mul=t(7, 2.0), m=t(8, 2.0), g=t(9))


def _close64(a, b, what):
    assert torch.allclose(a, b, rtol=1e-12, atol=1e-14), f"{what}: {float((a - b).abs().max()):.3e}"


def test_out64_is_the_torch_operation():
    shape = (2, 8, 5, 7)
    v = R.randn(shape, 1, 2.0)
    sd = _sides(shape, 10)
    vd = v.double()
    pick = lambda *ks: {k: sd[k] for k in ks}                  # noqa: E731
    _close64(C.out64(v, {}, {})[0], vd, "plain")
    assert C.out64(v, {}, {})[1] is None
    _close64(C.out64(v, dict(silu_out=True), {})[0], F.silu(vd), "silu_out")
    y, tw = C.out64(v, dict(dual_silu=True), {})
    _close64(y, vd, "dual y")
    _close64(tw, F.silu(vd), "dual twin")
    for scale in (1.0, -1.0, 0.5):
        y, tw = C.out64(v, dict(res_scale=scale, dual_silu=True), pick("res"))
        _close64(y, vd + scale * sd["res"].double(), f"res {scale}")
        _close64(tw, F.silu(vd + scale * sd["res"].double()), f"res {scale} twin")
    _close64(C.out64(v, dict(silu_out=True), pick("res"))[0], F.silu(vd + sd["res"].double()), "res + silu_out")
    _close64(C.out64(v, {}, pick("mul"))[0], sd["mul"].double() * vd, "mul")
    y, tw = C.out64(v, dict(dual_silu=True), pick("gate_mul", "gate_id"))
    gate = sd["gate_mul"].double() * torch.sigmoid(vd) + sd["gate_id"].double()
    _close64(y, gate, "gate")
    _close64(tw, F.silu(gate), "gate twin")
    # * silu'(m) (+ res): autograd through z silu(m) with the incoming gradient v
    m = sd["dsilu_mul"].double().requires_grad_()
    F.silu(m).backward(vd)
    _close64(C.out64(v, {}, pick("dsilu_mul"))[0], m.grad, "dsilu_mul")
    _close64(C.out64(v, dict(res_scale=0.5), pick("dsilu_mul", "res"))[0], m.grad + 0.5 * sd["res"].double(), "dsilu_mul + res")
    # GDN / IGDN forward on a positive v
    vp = v.abs() + 1.0
    _close64(C.out64(vp, {}, pick("gdn_mul"))[0], sd["gdn_mul"].double() * torch.rsqrt(vp.double()), "gdn")
    _close64(C.out64(vp, {}, pick("igdn_mul"))[0], sd["igdn_mul"].double() * torch.sqrt(vp.double()), "igdn")


def test_out64_shuffle_is_pixel_shuffle_then_the_sides():
    v = R.randn((2, 8, 3, 5), 2)
    big = (2, 2, 6, 10)
    sd = dict(dsilu_mul=R.randn(big, 3, 2.0), res=R.randn(big, 4))
    ps = F.pixel_shuffle(v.double(), 2)
    _close64(C.out64(v, dict(shuffle2=True), {})[0], ps, "shuffle")
    m = sd["dsilu_mul"].double().requires_grad_()
    F.silu(m).backward(ps)
    _close64(C.out64(v, dict(shuffle2=True), dict(dsilu_mul=sd["dsilu_mul"]))[0], m.grad, "shuffle + dsilu_mul")
    _close64(C.out64(v, dict(shuffle2=True), sd)[0], m.grad + sd["res"].double(), "shuffle + dsilu_mul + res")
    assert torch.equal(C.out_f32(v, dict(shuffle2=True), {})[0], F.pixel_shuffle(v, 2))


@pytest.mark.parametrize("kind", ["gdn", "igdn", "gate"])
def test_out64_backward_pairs_are_autograd(kind):
    shape = (2, 8, 5, 7)
    sd = dict(m=R.randn(shape, 5, 2.0), g=R.randn(shape, 6))
    s = R.randn(shape, 7, 2.0)
    if kind != "gate":
        s = s.abs() + 1.0
    md, sdd = sd["m"].double().requires_grad_(), s.double().requires_grad_()
    if kind == "gdn":
        fwd = md * torch.rsqrt(sdd)
    elif kind == "igdn":
        fwd = md * torch.sqrt(sdd)
    else:
        fwd = md * torch.sigmoid(sdd) + torch.zeros_like(md)
    fwd.backward(sd["g"].double())
    o1, o2 = C.out64(s, dict(bwd=kind), sd)
    _close64(o1, md.grad, f"{kind}: first output")
    _close64(o2, sdd.grad, f"{kind}: d s")


EPILOGUES = [({}, ()), (dict(silu_out=True), ()), (dict(dual_silu=True), ()), (dict(res_scale=-1.0), ("res",)), (dict(res_scale=0.5, dual_silu=True), ("res",)),
             (dict(dual_silu=True), ("res",)), (dict(silu_out=True), ("res",)), ({}, ("dsilu_mul",)), ({}, ("dsilu_mul", "res")), ({}, ("mul",)),
             ({}, ("gdn_mul",)), ({}, ("igdn_mul",)), ({}, ("gate_mul", "gate_id")), (dict(dual_silu=True), ("gate_mul", "gate_id")),
             (dict(shuffle2=True), ()), (dict(shuffle2=True), ("dsilu_mul",)), (dict(shuffle2=True, res_scale=0.5), ("dsilu_mul", "res")),
             (dict(bwd="gdn"), ("m", "g")), (dict(bwd="igdn"), ("m", "g")), (dict(bwd="gate"), ("m", "g"))]


@pytest.mark.parametrize("case", EPILOGUES, ids=lambda c: "+".join(sorted(c[0]) + list(c[1])) or "plain")
def test_out_f32_restates_out64(case):
    """A sanity tie, not the check of out_f32's rounding sequence: 64 units of roundoff in out_scale64's scale (|v| standing in for
    the scale of v) hold every epilogue -- the worst here is silu'(m) at 8 < m < 17, a ~17 ulp formula (tests/test_gpu_leaf_ops.py) --
    and catch a dropped res_scale, a wrong constant or a swapped operand, which are off by a fraction of the result.  A missing
    rounding step or a fused multiply-add would pass: those are held by the GPU tests' torch.equal against out_f32 on the kernel's own
    accumulator (tests/test_gpu_conv_epilogues.py), which is also what pins the library's -ffp-contract=off.  Sides of a PixelShuffle
    store have the shuffled shape."""
    ep, keys = case
    shape = (2, 8, 9, 11)
    v = R.special_x(2 * 8 * 9 * 11, 21).view(shape) * 0.2
    if any(k in keys for k in ("gdn_mul", "igdn_mul")) or ep.get("bwd") in ("gdn", "igdn"):
        v = v.abs() + 1.0
    allsd = _sides((2, 2, 18, 22) if ep.get("shuffle2") else shape, 30)
    sd = {k: allsd[k] for k in keys}
    want, got, scale = C.out64(v, ep, sd), C.out_f32(v, ep, sd), C.out_scale64(v, v.abs(), ep, sd)
    for w, g, s in zip(want, got, scale):
        assert (w is None) == (g is None) == (s is None)
        if w is not None:
            assert g.dtype == torch.float32 and g.shape == w.shape == s.shape
            assert C.rel_err(g, w, s) <= 64 * U, f"{C.rel_err(g, w, s) / U:.1f} u"


CONVS = [(2, 20, 40, 7, 9, 3, 1, None), (2, 20, 40, 7, 10, 3, 2, "silu"), (2, 20, 40, 7, 9, 1, 1, "square"), (2, 128, 24, 3, 3, 3, 1, None), (1, 5, 3, 4, 4, 3, 2, None)]


@pytest.mark.parametrize("case", CONVS)
def test_conv_seq_f32_is_within_the_chain_bound(case):
    n, cin, cout, h, w, ks, stride, pro = case
    x, wt, b = R.randn((n, cin, h, w), 41), R.randn((cout, cin, ks, ks), 42, (cin * ks * ks) ** -0.5), R.randn((cout,), 43, 0.1)
    want, scale = C.conv64(x, wt, b, stride, pro), C.conv_scale64(x, wt, b, stride, pro)
    got = C.conv_seq_f32(x, wt, b, stride, pro)
    assert got.shape == want.shape and got.dtype == torch.float32
    k = cin * ks * ks
    bound = (k + 1) * U            # (first order: every term passes through at most K additions, the bias' included, and its own product)
    assert C.rel_err(got, want, scale) <= bound, f"{C.rel_err(got, want, scale) / U:.1f} u > {k + 1} u"
    assert C.rel_err(got, want, scale) > 0.0                   # (a float64 result in disguise would be no yardstick)
    assert bool((scale >= want.abs()).all())


def test_conv64_prologues():
    x, wt = R.randn((1, 3, 4, 5), 51), R.randn((2, 3, 3, 3), 52)
    _close64(C.conv64(x, wt, None, 1, "silu"), F.conv2d(F.silu(x.double()), wt.double(), padding=1), "silu_in")
    _close64(C.conv64(x, wt[:, :, :1, :1], None, 1, "square"), F.conv2d(x.double() ** 2, wt[:, :, :1, :1].double()), "square_in")


@pytest.mark.parametrize("hw", [(3, 5), (4, 4)])
def test_dgrad2_weight_is_the_stride2_input_gradient(hw):
    cout, cin = 6, 5
    h, w = hw
    wt, dy = R.randn((cout, cin, 3, 3), 61), R.randn((2, cout, h, w), 62)
    xin = R.randn((2, cin, 2 * h, 2 * w), 63).double().requires_grad_()
    F.conv2d(xin, wt.double(), None, stride=2, padding=1).backward(dy.double())
    wd = C.dgrad2_weight(wt)
    assert wd.shape == (4 * cin, cout, 3, 3)
    assert bool((wd[:, :, 0, :] == 0).all()) and bool((wd[:, :, :, 0] == 0).all())          # only the lower-right 2 x 2 taps
    _close64(C.out64(C.conv64(dy, wd, None), dict(shuffle2=True), {})[0], xin.grad, "stride-2 input gradient")


def test_library_is_built_without_contraction():
    """out_f32 rounds every product and every sum separately; that is the kernel's arithmetic only while the library is compiled
    with -ffp-contract=off."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "mcquic_amd", "build.py")) as f:
        assert '"-ffp-contract=off"' in f.read()
