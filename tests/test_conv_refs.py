"""CPU: the references of tests/_conv_refs.py against torch's own operations and float64 autograd, so that a GPU test built on
them cannot bless a kernel with a reference that is wrong the same way.

  * out64 of every epilogue equals the torch operation (F.silu, torch.sigmoid, F.pixel_shuffle) or autograd through the forward
    formula (x rsqrt(s), x sqrt(s), a sigmoid(s) + x for the three backward pairs; z silu(m) for * silu'(m));
  * out_f32 stays within a few float32 roundings of out64 in out_scale64's scale (a restatement with a wrong constant or a dropped
    res_scale would be off by far more);
  * conv_seq_f32 agrees with conv64 within the chain's standard bound (K + 1) 2^-24 conv_scale64;
  * dgrad2_weight's filter, stored through PixelShuffle(2), is autograd's input gradient of the stride-2 convolution;
  * the fused 1x1 layer's references (post64 / post_f32 / post_scale64, the sub-pixel row order) on the very inputs
    tests/test_gpu_conv_post_epilogues.py launches: post64 is the oracle's GDN / IGDN and F.conv2d + sigmoid composed in float64,
    post_f32 restates it, the row order reproduces F.pixel_shuffle, and every GDN / IGDN case has s >= 1;
  * the Winograd restatements (wino1d_f32 / wino2d_f32) in float64 ARE the convolution at every geometry and channel count
    tests/test_gpu_conv_other_kernels.py launches, and on the exact cases (exact_case) the float32 restatement, the float64 one,
    conv64 and the int64 convolution are the same integers: the exact cases are exact for the reference alone."""
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


# ---- the fused 1x1 layer behind a 3x3 convolution (MCQ_CONV_POST_*) ------------------------------------------------------------------------
POST_SMALL = ("odd7x9", "s2_7x10", "tiny3x3", "sub5x7", "sub3x3")
POST_VARIANTS = ("dense",) + C.POST_EXACT


def _post_v(gname, pro=None, bias3=True):
    """(v64, its scale, the one-chain float32 v) of the GPU test's 3x3 layer at `gname`, shuffled where the geometry is."""
    g = C.POST_GEOMS[gname]
    x, w, b = C.post_problem(gname, bias3)
    vs = (C.conv64(x, w, b, g["stride"], pro), C.conv_scale64(x, w, b, g["stride"], pro), C.conv_seq_f32(x, w, b, g["stride"], pro))
    return tuple(F.pixel_shuffle(t, 2) for t in vs) if g["sub"] else vs


def _rel64(a, b):
    return float(((a - b).abs() / b.abs().clamp_min(1e-300)).max())


@pytest.mark.parametrize("gname", POST_SMALL)
@pytest.mark.parametrize("inverse", [False, True], ids=["gdn", "igdn"])
def test_post64_is_the_oracles_gdn(gname, inverse):
    """post64 against oracle.mcquic_ref.gdn on the GPU test's own v, w1 and b1 (the oracle's reparametrisation max(p, 0)^2 - 0 fed
    with float64 square roots: one float64 rounding), both directions, to 1e-12 relative; s >= 1 in every case."""
    from oracle import mcquic_ref as O
    kind = "igdn" if inverse else "gdn"
    v = _post_v(gname)[0]
    zero = torch.zeros(1, dtype=torch.float64)
    for variant in POST_VARIANTS:
        w1, b1 = C.post_layer(kind, variant)
        sd = {"g.gamma": torch.sqrt(w1.double()), "g.beta": torch.sqrt(b1.double()), "g.beta_reparam.eps": zero, "g.gamma_reparam.eps": zero,
              "g.beta_reparam.lowerBound.bound": zero, "g.gamma_reparam.lowerBound.bound": zero}
        got, twin = C.post64(v, kind, w1, b1)
        assert twin is None and _rel64(got, O.gdn(sd, "g.", v, inverse)) <= 1e-12, f"{variant}"
        s = F.conv2d(v * v, w1.double()[..., None, None], b1.double())
        assert float(s.min()) >= 1.0, f"{variant}: s = {float(s.min())}"
    w1, _ = C.post_layer(kind, "dense", bias1=False)             # (no GPU row runs GDN without its bias; the reference takes None all the same)
    assert _rel64(C.post64(v, kind, w1, None)[0], v * F.conv2d(v * v, w1.double()[..., None, None]) ** (0.5 if inverse else -0.5)) <= 1e-12


@pytest.mark.parametrize("gname", ["odd7x9", "tiny3x3"])
def test_post64_gate_is_conv2d_sigmoid_composed(gname):
    """a * sigmoid(F.conv2d(v + res_scale res, w1, b1)) + x in float64, with and without the residual and the 1x1 bias; the twin is
    F.silu of it."""
    v = _post_v(gname)[0]
    sd = C.post_sides(("res", "gate_mul", "gate_id"), v.shape)
    a, xid, res = sd["gate_mul"].double(), sd["gate_id"].double(), sd["res"].double()
    for variant in POST_VARIANTS:
        for bias1 in ((True, False) if variant == "dense" else (True,)):
            w1, b1 = C.post_layer("gate", variant, bias1)
            b1d = None if b1 is None else b1.double()
            for scale in (None, 1.0, -1.0, 0.5):
                sides = {k: t for k, t in sd.items() if k != "res" or scale is not None}
                vv = v if scale is None else v + scale * res
                want = a * torch.sigmoid(F.conv2d(vv, w1.double()[..., None, None], b1d)) + xid
                got, twin = C.post64(v, "gate", w1, b1, sides, 1.0 if scale is None else scale)
                assert _rel64(got, want) <= 1e-12 and _rel64(twin, F.silu(want)) <= 1e-12, f"{variant} bias1={bias1} res_scale={scale}"


def test_post_order_is_the_accumulator_order():
    """k-step t = 16 mb + r holds the channels 32 mb + (r & 3) + 8 (r >> 2) and that + 4: written out for the first steps of two bands."""
    assert C.POST_ORDER[:10] == (0, 4, 1, 5, 2, 6, 3, 7, 8, 12) and C.POST_ORDER[30:34] == (27, 31, 32, 36)
    assert sorted(C.POST_ORDER) == list(range(128))


POST_CPU_CASES = [(k, g) for k in ("gdn", "igdn", "gate") for g in POST_SMALL if not (k == "gate" and C.POST_GEOMS[g]["stride"] == 2)]


@pytest.mark.parametrize("kind,gname", POST_CPU_CASES, ids=[f"{k}-{g}" for k, g in POST_CPU_CASES])
def test_post_f32_restates_post64(kind, gname):
    """The same sanity tie as test_out_f32_restates_out64, same 64 units of roundoff: post_f32 against post64 in post_scale64's
    scale, on the close alone (v exact) and on the whole launch (the one-chain v against conv64), at every res_scale the GPU rows
    use.  A chain of 129 additions is bounded by 129 u of its magnitude sum and lands at 2 - 6 u; a dropped res_scale, bias or
    square is off by a fraction of the result.  The restatement must also differ from float64 (else it is no yardstick)."""
    v64, vscale, vseq = _post_v(gname)
    v32 = v64.float()
    names = ("res", "gate_mul", "gate_id") if kind == "gate" else ()
    sd = C.post_sides(names, v64.shape)
    for variant, scales in (("dense", (1.0, -1.0, 0.5)), ("perm", (1.0,))):
        w1, b1 = C.post_layer(kind, variant)
        for rs in scales if kind == "gate" else (1.0,):
            for v_in, v_ref, sc_in in ((v32, v32, v32.abs()), (vseq, v64, vscale)):
                want, got, scale = C.post64(v_ref, kind, w1, b1, sd, rs), C.post_f32(v_in, kind, w1, b1, sd, rs), C.post_scale64(v_ref, sc_in, kind, w1, b1, sd, rs)
                for w, g, s in zip(want, got, scale):
                    assert (w is None) == (g is None) == (s is None)
                    if w is not None:
                        assert g.dtype == torch.float32 and g.shape == w.shape == s.shape and bool((s >= w.abs()).all())
                        assert 0.0 < C.rel_err(g, w, s) <= 64 * U, f"{variant} res_scale={rs}: {C.rel_err(g, w, s) / U:.1f} u"


def test_post_f32_chain_is_exact_on_integers():
    """The chain starts from the bias, squares for GDN / IGDN and takes every channel once: on integers small enough for float32 to
    hold every partial sum, s is the float64 sum, so the result is the float32 close of that s bit for bit (a chunk boundary inside
    the pixels included)."""
    gen = lambda seed: torch.Generator().manual_seed(seed)          # noqa: E731
    vi = torch.randint(1, 4, (2, 128, 3, 5), generator=gen(7)).float() * (2 * torch.randint(0, 2, (2, 128, 3, 5), generator=gen(6)).float() - 1)
    wi, bi = torch.randint(0, 3, (128, 128), generator=gen(8)).float(), torch.randint(1, 6, (128,), generator=gen(9)).float()
    s = (torch.einsum("oc,nchw->nohw", wi.double(), vi.double() ** 2) + bi.double().reshape(1, 128, 1, 1)).float()
    assert torch.equal(C.post_f32(vi, "igdn", wi, bi, chunk=7)[0], vi * R.sqrt_f32(s))
    assert torch.equal(C.post_f32(vi, "gdn", wi, None)[0], vi * R.div_f32(1.0, R.sqrt_f32(s - bi.reshape(1, 128, 1, 1))))
    one = dict(gate_mul=torch.ones_like(vi), gate_id=torch.zeros_like(vi), res=torch.ones_like(vi))
    wg = torch.randint(-2, 3, (128, 128), generator=gen(10)).float()
    sg = (torch.einsum("oc,nchw->nohw", wg.double(), vi.double() - 2.0) + bi.double().reshape(1, 128, 1, 1)).float()
    assert torch.equal(C.post_f32(vi, "gate", wg, bi, one, -2.0)[0], R.gate_f32(one["gate_mul"], sg, one["gate_id"]))


def test_post_res_scale_and_bias_are_live():
    """A reference that ignored res_scale, the residual or either bias would tie the GPU test to nothing: each changes post64."""
    v = _post_v("odd7x9")[0]
    sd = C.post_sides(("res", "gate_mul", "gate_id"), v.shape)
    w1, b1 = C.post_layer("gate")
    base = C.post64(v, "gate", w1, b1, sd, 1.0)[0]
    for other in (C.post64(v, "gate", w1, b1, sd, 0.5)[0], C.post64(v, "gate", w1, b1, sd, -1.0)[0], C.post64(v, "gate", w1, None, sd, 1.0)[0],
                  C.post64(v, "gate", w1, b1, {k: t for k, t in sd.items() if k != "res"})[0]):
        assert float((other - base).abs().max()) > 1e-3


@pytest.mark.parametrize("gname", ["sub5x7", "sub3x3"])
def test_subpixel_rows_reproduce_pixel_shuffle(gname):
    """The layer in sub-pixel-major row order, read back through from_subpixel_rows, is F.pixel_shuffle of the layer as given: in
    float64 to the last bit (the rows are the same sums), and row 128 T + c is channel 4 c + T."""
    x, w, b = C.post_problem(gname)
    ws, bs = C.to_subpixel_rows(w, b)
    assert ws.shape == w.shape and bs.shape == b.shape
    for t, c in ((0, 0), (1, 0), (2, 5), (3, 127)):
        assert torch.equal(ws[128 * t + c], w[4 * c + t]) and bs[128 * t + c] == b[4 * c + t]
    want = F.pixel_shuffle(C.conv64(x, w, b), 2)
    assert torch.equal(C.from_subpixel_rows(C.conv64(x, ws, bs)), want)
    assert C.to_subpixel_rows(w, None)[1] is None
    v = R.randn((2, 512, 3, 5), 3)
    rows = C.to_subpixel_rows(v.transpose(0, 1), None)[0].transpose(0, 1)
    assert torch.equal(C.from_subpixel_rows(rows), F.pixel_shuffle(v, 2))


def test_post_exact_layers_are_permutations_times_powers_of_two():
    for kind in ("gdn", "igdn", "gate"):
        seen = []
        for variant in C.POST_EXACT:
            w1, b1 = C.post_layer(kind, variant)
            nz = w1 != 0
            assert bool((nz.sum(0) == 1).all()) and bool((nz.sum(1) == 1).all())
            mant, _ = torch.frexp(w1[nz])
            assert bool((mant == 0.5).all()) and bool((b1 == (0.0 if kind == "gate" else 1.0)).all())
            src = nz.float().argmax(1)
            if variant.startswith("shift"):
                assert torch.equal(src, (torch.arange(128) + int(variant[5:])) % 128)
            seen.append(src)
        assert not any(torch.equal(seen[3], s) for s in seen[:3])


# ---- the other kernels' references: conv_head16_kernel and the Winograd forms ----------------------------------------------------------------
OTHER_CASES = [(k, gn, ci, co) for k in ("wino1d", "wino32", "wino16") for gn in C.WINO_GEOMS
               for ci, co in sorted({(ci, co) for ci, co, _ in C.OTHER_CHANNELS[k]})]


@pytest.mark.parametrize("kernel", ("wino1d", "wino32", "wino16"))
def test_winograd_restatements_in_float64_are_the_convolution(kernel):
    """wino1d_f32 / wino2d_f32 with dtype=float64 against conv64 within 1e-12 of conv_scale64, with and without bias, on every
    (geometry, Cin, Cout) of the GPU test: what makes them references.  The float32 form stays within the chain's standard bound
    (the sum of the products' magnitudes is below the walk of _wino over magnitudes, a few times conv_scale64)."""
    form = C.OTHER_FORM[kernel]
    fn = C.wino1d_f32 if form == "wino1d" else C.wino2d_f32
    ran = 0
    for k, gn, ci, co in OTHER_CASES:
        if k != kernel:
            continue
        for bias in (True, False):
            x, w, b = C.other_problem(kernel, gn, ci, co, bias)
            ref, scale = C.conv64(x, w, b), C.conv_scale64(x, w, b)
            got = fn(x, w, b, dtype=torch.float64)
            assert got.dtype == torch.float64 and got.shape == ref.shape
            err = float(((got - ref).abs() / scale).max())
            assert err <= 1e-12, f"{kernel} {gn} Cin={ci} Cout={co} bias={bias}: {err:.3e} of conv_scale64"
            ran += 1
        x, w, b = C.other_problem(kernel, gn, ci, co)
        f32 = fn(x, w, b)
        assert f32.dtype == torch.float32 and torch.equal(f32, C.other_yardstick(kernel, x, w, b))
        top, _, _ = C._wino(form, x, w, b, torch.float64, bound=True)
        assert float(((f32.double() - C.conv64(x, w, b)).abs() / top).max()) <= (3 * ci + 8) * U
    assert ran == 2 * len(C.WINO_GEOMS) * len({(ci, co) for ci, co, _ in C.OTHER_CHANNELS[kernel]})


def test_winograd_restatement_catches_a_wrong_transform_row():
    """The restatement is not the convolution by accident: with two rows of G swapped it is off by more than 1e-2 of conv_scale64."""
    x, w, b = C.other_problem("wino32", "odd7x9", 24, 128)
    ref, scale = C.conv64(x, w, b), C.conv_scale64(x, w, b)
    keep = C.WINO_G
    try:
        C.WINO_G = (keep[0], keep[2], keep[1], keep[3])
        bad = C.wino2d_f32(x, w, b, dtype=torch.float64)
    finally:
        C.WINO_G = keep
    assert float(((bad - ref).abs() / scale).max()) > 1e-2


# (kernel, geometry, Cin, Cout, seed) exactly as tests/test_gpu_conv_other_kernels.py::test_exact builds them: the seed is the index
# of the channel configuration, a forced tile being a configuration of its own
EXACT_CASES = [(k, gn, ci, co, i) for k in ("head16", "wino1d", "wino32", "wino16") for gn in (C.HEAD_GEOMS if k == "head16" else C.WINO_GEOMS)
               for i, (ci, co, _) in enumerate(C.OTHER_CHANNELS[k])]


@pytest.mark.parametrize("kernel", ("head16", "wino1d", "wino32", "wino16"))
def test_exact_cases_are_exact_for_the_references(kernel):
    """On every exact case the GPU test launches: float32 restatement == float64 restatement == conv64 == F.conv2d in int64, all
    with torch.equal (the builder has asserted its bound on every intermediate; this is the same statement by computation)."""
    form = C.OTHER_FORM[kernel]
    ran = 0
    for k, gn, ci, co, seed in EXACT_CASES:
        if k != kernel:
            continue
        h, wd = C.OTHER_GEOMS[gn]
        x, w, b, res = C.exact_case(form, ci, co, h, wd, seed=seed)
        for t in (x, w, b, res):
            assert t.dtype == torch.float32 and torch.equal(t, t.round())
        assert x.shape == (2, ci, h, wd) and res.shape == (2, co, h, wd)
        if form == "wino1d":
            assert torch.equal(w % 2, torch.zeros_like(w))
        if form == "wino2d":
            assert torch.equal(w % 4, torch.zeros_like(w))
        want = F.conv2d(x.long(), w.long(), b.long(), padding=1)
        v64 = C.conv64(x, w, b)
        assert torch.equal(v64, want.double()), f"{kernel} {gn}: conv64 is not the integer convolution"
        if form == "direct":
            f32, f64 = C.conv_seq_f32(x, w, b), v64
        else:
            f32, f64 = C._wino(form, x, w, b, torch.float32), C._wino(form, x, w, b, torch.float64)
        assert torch.equal(f32.double(), f64), f"{kernel} {gn}: the float32 restatement rounds"
        assert torch.equal(f64, v64), f"{kernel} {gn}: the float64 restatement is not conv64"
        # ... and the epilogues the exact launches carry stay integers below 2^24: - res, and the PixelShuffle store
        assert float((v64.abs() + res.double().abs()).max()) < C.EXACT_LIMIT
        y, _ = C.out_f32(f32, dict(res_scale=-1.0), dict(res=res))
        assert torch.equal(y.long(), want - res.long())
        ran += 1
    assert ran == len([c for c in EXACT_CASES if c[0] == kernel])


def test_exact_case_refuses_what_is_not_exact():
    """The builder asserts its bound rather than trusting it: a centre pixel under nine taps of a million channels (mean |x| |w| about 2) passes 2^24."""
    with pytest.raises(AssertionError):
        C.exact_case("direct", 1000000, 1, 3, 3, n=1)
