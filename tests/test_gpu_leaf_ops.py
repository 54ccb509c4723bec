"""GPU: the leaf kernels of the training step, one by one, against references written from the mathematics (tests/_leaf_refs.py;
nothing there calls this library, and tests/test_leaf_ops_reference.py holds those references to float64 autograd on the CPU).

The fused-form tests elsewhere (test_gpu_step_ops.py) compare a fused launch with these kernels bit for bit; the model-level
gradient tests see them through `max abs / max abs` bars of 1e-5.  Neither notices a wrong constant, a wrong branch of the
LowerBound rule at p == bound or a dropped tail element.  Here:
  * exact ops (layout changes, gathers): torch.equal with torch's own permutation;
  * ops without a transcendental: torch.equal with the float32 restatement in the kernel's operation order (the library is built
    with -ffp-contract=off; float divide and square root are correctly rounded by default);
  * ops with expf: error in float32 ulps at the float64 value (R.ulp_err), allowed 4x the worst error of the same formula
    evaluated op by op in float32 on the CPU over the same inputs -- the factor GRAD_BARS and the MS-SSIM tests use; it covers a
    faithfully rounded expf against a correctly rounded one.  Measured on an MI355X (profiles/r07_leaf_op_errors.json): see each test;
  * reductions: the standard bound of their summation order, derived in the test, and the same bits when repeated.
The second half runs the ops on non-contiguous and 4-byte-aligned views of the same values."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _leaf_refs as R
from _record import record

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -24            # unit roundoff of float32


def _flat_cases():
    """(n, shape) of every flat-op launch: the sizes around the launch geometry, then one network-sized activation."""
    out = [(n, (n,)) for n in R.FLAT_SIZES]
    n = 1
    for d in R.NET_SHAPE:
        n *= d
    return out + [(n, R.NET_SHAPE)]


def _ulp_bar(key, gpu, cpu):
    """Record both figures, then hold the kernel to 4x the float32 formula's own worst error."""
    record(key, gpu_ulp=gpu, cpu_f32_formula_ulp=cpu, bar_ulp=4.0 * cpu)
    print(f"{key}: gpu {gpu:.3f} ulp, float32 formula on the CPU {cpu:.3f} ulp, bar {4.0 * cpu:.3f}")
    assert gpu <= 4.0 * cpu, f"{key}: {gpu:.3f} ulp > 4 x {cpu:.3f} ulp"


def _worst(got, want64, scale64=None):
    got = got.cpu()
    assert torch.isfinite(got).all(), "non-finite result"
    return float(R.ulp_err(got, want64, scale64).max())


# ---- ops with expf ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_other", [False, True])
def test_silu_bwd(dev, with_other):
    """dy silu'(x) (+ other) against float64 autograd through x sigmoid(x); x over [-30, 30] with +-87, +-100 (expf(-x) overflows in
    sigmoidf_: the result must stay finite), +-0 and the zero of silu' (x = -1.2785: measured in ulps of |dy| within 1/4 of it; with
    `other` in ulps of the larger operand of the closing addition).  The float32 formula itself is a ~17 ulp one (for 8 < x < 17.4
    the factor 1 - s carries the absolute error of s times x); measured (profiles/r07_leaf_op_errors.json, leaf_silu_bwd[*]): formula on the CPU 16.53 / 16.83 ulp without / with `other`, the
    kernel the same 16.53 / 16.83 (the same worst element); bars 66.1 / 67.3."""
    from mcquic_amd import ops
    gpu = cpu = 0.0
    for i, (n, shape) in enumerate(_flat_cases()):
        x, dy = R.special_x(n, 100 + i).view(shape), R.randn(shape, 200 + i)
        other = R.randn(shape, 300 + i, 0.5) if with_other else None
        want, scale = R.silu_bwd64(x, dy, other), R.silu_bwd_scale64(x, dy, other)
        got = ops.silu_bwd(x.to(dev), dy.to(dev), None if other is None else other.to(dev))
        assert got.shape == x.shape
        gpu = max(gpu, _worst(got, want, scale))
        cpu = max(cpu, _worst(R.silu_bwd_f32(x, dy, other), want, scale))
    _ulp_bar(f"leaf_silu_bwd[other={with_other}]", gpu, cpu)


def test_gate_bwd(dev):
    """(dout s, dout a s (1 - s)), s = sigmoid(b), against float64 autograd through a sigmoid(b) + x, b like test_silu_bwd's x.
    db for b > 0 is measured in ulps of |dout a| / 4 (R.gate_bwd_db_scale64: 1 - s cancels).  Measured (profiles/r07_leaf_op_errors.json,
    leaf_gate_bwd_*): da formula 2.90 ulp, kernel 2.88, bar 11.6; db formula 5.83, kernel 5.83, bar 23.3."""
    from mcquic_amd import ops
    g_da = g_db = c_da = c_db = 0.0
    for i, (n, shape) in enumerate(_flat_cases()):
        a, b, dout = R.randn(shape, 400 + i, 2.0), R.special_x(n, 500 + i).view(shape), R.randn(shape, 600 + i)
        da64, db64 = R.gate_bwd64(a, b, dout)
        sc = R.gate_bwd_db_scale64(a, b, dout)
        da, db = ops.gate_bwd(a.to(dev), b.to(dev), dout.to(dev))
        fa, fb = R.gate_bwd_f32(a, b, dout)
        g_da, g_db = max(g_da, _worst(da, da64)), max(g_db, _worst(db, db64, sc))
        c_da, c_db = max(c_da, _worst(fa, da64)), max(c_db, _worst(fb, db64, sc))
    _ulp_bar("leaf_gate_bwd_da", g_da, c_da)
    _ulp_bar("leaf_gate_bwd_db", g_db, c_db)


def test_gate_forward_and_twin(dev):
    """a sigmoid(b) + x in float64 (ulps of the larger operand of the addition) and the SiLU twin of `dual_silu=True` against float64
    silu of the stored result.  Measured (profiles/r07_leaf_op_errors.json, leaf_gate_fwd*): gate formula 2.45 ulp, kernel 2.45, bar 9.8; twin
    formula 2.28, kernel 3.10 (mcq_silu's compensated exp2 / rcp, csrc/mcq_common.h), bar 9.1."""
    from mcquic_amd import ops
    g_o = g_t = c_o = c_t = 0.0
    for i, (n, shape) in enumerate(_flat_cases()):
        a, b, x = R.randn(shape, 700 + i, 2.0), R.special_x(n, 800 + i).view(shape), R.special_x(n, 900 + i).view(shape) * 0.5
        want, sc = R.gate64(a, b, x), R.gate_scale64(a, b, x)
        out = ops.gate(a.to(dev), b.to(dev), x.to(dev), dual_silu=True)
        twin = ops.silu_twin(out)
        assert twin is not None and twin.shape == out.shape
        plain = ops.gate(a.to(dev), b.to(dev), x.to(dev))
        assert torch.equal(plain, out) and ops.silu_twin(plain) is None
        o = out.cpu()
        g_o, c_o = max(g_o, _worst(o, want, sc)), max(c_o, _worst(R.gate_f32(a, b, x), want, sc))
        g_t, c_t = max(g_t, _worst(twin, R.silu64(o))), max(c_t, _worst(R.silu_f32(o), R.silu64(o)))
    _ulp_bar("leaf_gate_fwd", g_o, c_o)
    _ulp_bar("leaf_gate_fwd_twin", g_t, c_t)


# ---- ops without a transcendental: the same bits as the float32 restatement -----------------------------------------------------------------
@pytest.mark.parametrize("inverse", [False, True])
def test_gdn_bwd_prep(dev, inverse):
    """(dy f(s), dy x f'(s)), f = s^-1/2 (GDN) / s^1/2 (IGDN), s from 1e-6 to 1e3: bit-equal to 1 / sqrt(s) and the products in the
    kernel's order (root and quotient correctly rounded: R.sqrt_f32 / R.div_f32, not ATen's vectorised float32 sqrt), and -- so that the restatement cannot bless a wrong constant -- within 8 ulp of float64 autograd through
    x s^(+-1/2) (at most seven roundings of half an ulp, the root's and the quotient's entering rs^3 three times: 4.5 ulp to first
    order; the CPU file holds the restatement to the same 8)."""
    from mcquic_amd import ops
    for i, (n, shape) in enumerate(_flat_cases()):
        x, s, dy = (t.view(shape) for t in R.gdn_inputs(n, 1000 + 3 * i))
        dxd, ds = ops.gdn_bwd_prep(x.to(dev), s.to(dev), dy.to(dev), inverse)
        fx, fs = R.gdn_bwd_prep_f32(x, s, dy, inverse)
        assert torch.equal(dxd.cpu(), fx), f"dxd n={n}: {_worst(dxd, fx.double()):.2f} ulp from the restatement"
        assert torch.equal(ds.cpu(), fs), f"ds n={n}: {_worst(ds, fs.double()):.2f} ulp from the restatement"
        w_x, w_s = R.gdn_bwd_prep64(x, s, dy, inverse)
        assert _worst(dxd, w_x) <= 8.0 and _worst(ds, w_s) <= 8.0


def test_nonneg_reparam_forward(dev):
    """max(p, bound)^2 - pedestal, single and multi-parameter launches, bit-equal to the float32 restatement (two roundings) and
    within 2 ulp (of the larger of the square and the pedestal) of float64."""
    from mcquic_amd import ops
    cases = [(n, 0.1 + 0.05 * i, 2.0 ** -36 * (i + 1)) for i, n in enumerate(R.FLAT_SIZES)] + [(128 * 128, 2.0 ** -18, 2.0 ** -36)]
    ps = []
    for i, (n, bound, ped) in enumerate(cases):
        p, _ = R.reparam_inputs(n, 1100 + 2 * i, bound)
        ps.append(p)
        got = ops.nonneg_reparam(p.to(dev), bound, ped)
        assert torch.equal(got.cpu(), R.reparam_f32(p, bound, ped)), f"n={n}"
        assert _worst(got, R.reparam64(p, bound, ped), R.f32(ped).double().expand(n)) <= 2.0
    # all of them in one multi launch, and 70 parameters (more than the 64 a launch's table holds) in two
    many = [(ps[i % len(ps)], cases[i % len(cases)][1], cases[i % len(cases)][2]) for i in range(70)]
    for group in ([(p, c[1], c[2]) for p, c in zip(ps, cases)], many):
        src = [p.to(dev) for p, _, _ in group]
        outs = [torch.full_like(t, float("nan")) for t in src]
        ops.nonneg_reparam_multi_(src, outs, [b for _, b, _ in group], [e for _, _, e in group])
        for (p, b, e), o in zip(group, outs):
            assert torch.equal(o.cpu(), R.reparam_f32(p, b, e)), f"multi n={p.numel()}"


def test_nonneg_reparam_backward(dev):
    """g = 2 max(p, bound) dfolded, passed where p >= bound or g < 0 (the LowerBound rule), else 0 -- with elements at p == bound
    exactly, one float32 below and above it, below it with a gradient of each sign, and gradients of +-0: bit-equal to the float32
    restatement, and the same pass / block decision as float64 autograd on EVERY element."""
    from mcquic_amd import ops
    runs = []
    for i, n in enumerate(R.FLAT_SIZES + (128 * 128,)):
        bound = 0.1 + 0.05 * i
        p, d = R.reparam_inputs(n, 1200 + 2 * i, bound)
        got = ops.nonneg_reparam_bwd(p.to(dev), d.to(dev), bound).cpu()
        want32, want64 = R.reparam_bwd_f32(p, d, bound), R.reparam_bwd64(p, d, bound)
        assert torch.equal(got, want32), f"n={n}"
        assert torch.equal(got == 0, want64 == 0), f"n={n}: a different branch of the rule than float64 autograd"
        assert _worst(got, want64) <= 2.0
        runs.append((p, d, bound, want32))
    # the two-parameter launch: every pairing of a short and a long tensor (the kernel indexes both through one grid)
    for (p0, d0, b0, w0), (p1, d1, b1, w1) in zip(runs, runs[::-1]):
        o0, o1 = ops.nonneg_reparam_bwd2(p0.to(dev), d0.to(dev), b0, p1.to(dev), d1.to(dev), b1)
        assert torch.equal(o0.cpu(), w0) and torch.equal(o1.cpu(), w1), f"bwd2 n=({p0.numel()}, {p1.numel()})"


@pytest.mark.parametrize("alpha,beta", [(1.0, -1.0), (0.3, -1.7), (-2.5, 0.0), (0.0, 1.0 / 3.0), (1e-3, 1e3)])
def test_axpby(dev, alpha, beta):
    """alpha a + beta b: two products and a sum, each rounded once -- bit-equal to that in float32; the SiLU twin of `dual_silu`
    within 4x the float32 formula's error of float64 silu of the stored result (as test_gate_forward_and_twin; measured, leaf_axpby_twin[*]:
    formula 1.95 ... 2.35 ulp, kernel 2.28 ... 3.12, bars 7.8 ... 9.4)."""
    from mcquic_amd import ops
    g_t = c_t = 0.0
    for i, (n, shape) in enumerate(_flat_cases()):
        if n > 2 ** 20 + 3 and (alpha, beta) != (0.3, -1.7):
            continue                                              # (the network-sized tensor once)
        a, b = R.special_x(n, 1300 + i).view(shape), R.randn(shape, 1400 + i, 3.0)
        want = R.axpby_f32(a, b, alpha, beta)
        out = ops.axpby(a.to(dev), b.to(dev), alpha, beta, dual_silu=True)
        assert torch.equal(out.cpu(), want), f"n={n}"
        assert torch.equal(ops.axpby(a.to(dev), b.to(dev), alpha, beta), out)
        o = out.cpu()
        g_t, c_t = max(g_t, _worst(ops.silu_twin(out), R.silu64(o))), max(c_t, _worst(R.silu_f32(o), R.silu64(o)))
    _ulp_bar(f"leaf_axpby_twin[{alpha:g},{beta:g}]", g_t, c_t)


def test_add_and_add3(dev):
    """a + b and (a + b) + c in that order (operands of mixed magnitude, so the order shows), all four n % 4 (the kernels take four
    elements per thread and a scalar tail), bit-equal to float32 torch; add's SiLU twin as above (measured, leaf_add_twin: formula 2.26 ulp, kernel 3.15, bar 9.0)."""
    from mcquic_amd import ops
    cases = _flat_cases() + [(n, (n,)) for n in (2, 4, 5, 6, 7, 8, 1024, 1025, 1026)]
    assert {n % 4 for n, _ in cases} == {0, 1, 2, 3}
    g_t = c_t = 0.0
    for i, (n, shape) in enumerate(cases):
        a, b, c = R.randn(shape, 1500 + i, 100.0), R.randn(shape, 1600 + i), R.randn(shape, 1700 + i, 1e-2)
        s = ops.add(a.to(dev), b.to(dev), dual_silu=True)
        assert torch.equal(s.cpu(), a + b), f"add n={n}"
        assert torch.equal(ops.add(a.to(dev), b.to(dev)), s)
        got3 = ops.add3(a.to(dev), b.to(dev), c.to(dev)).cpu()
        assert torch.equal(got3, R.add3_f32(a, b, c)), f"add3 n={n}"
        if n >= 255:
            assert not torch.equal(got3, a + (b + c)), "the operands do not tell the two orders apart"
        o = s.cpu()
        g_t, c_t = max(g_t, _worst(ops.silu_twin(s), R.silu64(o))), max(c_t, _worst(R.silu_f32(o), R.silu64(o)))
    _ulp_bar("leaf_add_twin", g_t, c_t)


@pytest.mark.parametrize("want_db", [False, True])
def test_mse_bwd(dev, want_db):
    """da = (a - b) * (float(2 / n) * dloss), db = -da, with dloss != 1: bit-equal to that in float32 and within 3 ulp of float64
    autograd through mean((a - b)^2)."""
    from mcquic_amd import ops
    for i, (n, shape) in enumerate(_flat_cases()):
        a, b = R.rand(shape, 1800 + i), R.rand(shape, 1900 + i)
        dl = torch.tensor(0.37 * (i + 1), dtype=R.F32)
        da, db = ops.mse_bwd(a.to(dev), b.to(dev), dl.to(dev), want_db=want_db)
        fa, fb = R.mse_bwd_f32(a, b, dl)
        assert torch.equal(da.cpu(), fa), f"n={n}"
        assert (db is None) == (not want_db)
        if want_db:
            assert torch.equal(db.cpu(), fb)
        if n <= 2 ** 20 + 3:
            da64, _ = R.mse_bwd64(a, b, dl)
            assert _worst(da, da64) <= 3.0


# ---- layout ops: exact -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES + ((2, 128, 16, 16),))
def test_pixel_unshuffle2(dev, shape):
    from mcquic_amd import ops
    n, c, h, w = shape
    x = R.randn((n, c, 2 * h, 2 * w), 2000)
    got = ops.pixel_unshuffle2(x.to(dev))
    assert torch.equal(got.cpu(), F.pixel_unshuffle(x, 2))


@pytest.mark.parametrize("shape", R.SHAPES + ((2, 128, 16, 16), (1, 31, 3, 11), (2, 65, 33, 1)))
def test_nchw_to_nhwc(dev, shape):
    """The 32 x 32-tile transpose, with C and HW that are no multiples of the tile: torch's permute exactly; `square=True`: x * x,
    one rounding, exactly; and the two-tensor entry point (different channel counts and map sizes in one launch) through the C ABI."""
    from mcquic_amd import _lib, ops
    n, c, h, w = shape
    x = R.randn(shape, 2100, 3.0)
    assert torch.equal(ops.nchw_to_nhwc(x.to(dev)).cpu(), x.permute(0, 2, 3, 1).contiguous())
    assert torch.equal(ops.nchw_to_nhwc(x.to(dev), square=True).cpu(), (x * x).permute(0, 2, 3, 1).contiguous())
    cy, hy, wy = c + 7, max(1, h // 2), w + 3
    y = R.randn((n, cy, hy, wy), 2101)
    for square in (0, 1):
        guard = 64
        xo = torch.full((guard + x.numel() + guard,), 7.5, device=dev)
        yo = torch.full((guard + y.numel() + guard,), -3.25, device=dev)
        xd, yd = x.to(dev), y.to(dev)
        rc = _lib.load().mcq_nchw_to_nhwc_pair_f32(xd.data_ptr(), xo[guard:].data_ptr(), c, h * w, square, yd.data_ptr(), yo[guard:].data_ptr(),
                                                  cy, hy * wy, n, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        torch.cuda.synchronize()
        xs = x * x if square else x
        assert torch.equal(xo[guard:guard + x.numel()].cpu().view(n, h, w, c), xs.permute(0, 2, 3, 1).contiguous())
        assert torch.equal(yo[guard:guard + y.numel()].cpu().view(n, hy, wy, cy), y.permute(0, 2, 3, 1).contiguous())
        for t, fill in ((xo, 7.5), (yo, -3.25)):
            assert bool((t[:guard] == fill).all()) and bool((t[-guard:] == fill).all()), "written outside the output"


def test_gather_flat(dev):
    """mcq_gather_flat_f32 with tables built the way parallel.GraphedTrainStep builds them (sizes, running offsets, one block per
    4096-element chunk of each tensor): torch.cat of the flattened sources, exactly, for tensor sizes on both sides of a chunk and
    nothing written past the end."""
    from mcquic_amd import _lib
    lib = _lib.load()
    chunk = lib.mcq_adam_chunk()
    assert chunk == 4096
    sizes = [1, 4095, 4096, 4097, 3, 8192, 8193, 2 * 4096 + 255, 128 * 128 * 9, 7]
    srcs = [R.randn((n,), 2200 + i).to(dev) for i, n in enumerate(sizes)]
    offs, at, blk_t, blk_f = [], 0, [], []
    for i, n in enumerate(sizes):
        offs.append(at)
        at += n
        for first in range(0, n, chunk):
            blk_t.append(i)
            blk_f.append(first)
    guard = 64
    flat = torch.full((at + guard,), 7.5, device=dev)
    ptrs = torch.tensor([t.data_ptr() for t in srcs], dtype=torch.int64).to(dev)
    offs_d, numel_d = torch.tensor(offs, dtype=torch.int64).to(dev), torch.tensor(sizes, dtype=torch.int64).to(dev)
    bt, bf = torch.tensor(blk_t, dtype=torch.int32).to(dev), torch.tensor(blk_f, dtype=torch.int64).to(dev)
    rc = lib.mcq_gather_flat_f32(ptrs.data_ptr(), flat.data_ptr(), offs_d.data_ptr(), numel_d.data_ptr(), bt.data_ptr(), bf.data_ptr(), len(blk_t),
                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(flat[:at], torch.cat([t.reshape(-1) for t in srcs]))
    assert bool((flat[at:] == 7.5).all())


# ---- reductions: derived bounds --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", R.SHAPES + ((2, 128, 16, 16), (17, 3, 20, 20), (1, 4, 64, 64)))
def test_channel_sum(dev, shape):
    """Sum over batch and pixels per channel.  The kernel adds in float32 in a fixed order: each of 256 threads its strided share
    of a batch chunk, an 8-level tree, then the chunks in order; with k the longest chain of additions behind an output
    (R.channel_sum_chain, from the launcher's chunk rule) the standard bound is |got - want| <= k 2^-24 sum |x|.  Batches 2, 17
    and 35 take 2 and 16 chunks.  The same bits on a second call.  Measured (leaf_channel_sum[*]): at most 0.11 of the bound."""
    from mcquic_amd import ops
    n, c, h, w = shape
    x = R.randn(shape, 2300, 2.0) + 0.25
    got = ops.channel_sum(x.to(dev))
    assert got.shape == (c,)
    k, chunks = R.channel_sum_chain(n, h * w)
    assert chunks == (1 if n == 1 else min(n, 16))
    want = x.double().sum(dim=(0, 2, 3))
    bound = k * EPS32 * x.double().abs().sum(dim=(0, 2, 3))
    err = (got.cpu().double() - want).abs()
    record(f"leaf_channel_sum[{n}x{c}x{h}x{w}]", worst_err_over_bound=float((err / bound).max()), chain=k)
    assert bool((err <= bound).all()), f"{float((err / bound).max()):.3f} of the bound"
    assert torch.equal(ops.channel_sum(x.to(dev)), got)


def test_mse_and_sumsq(dev):
    """mean((a - b)^2) and sum(x^2): the kernels square in float32 and add in double -- every term carries at most three float32
    roundings (the difference, the square, the final cast of the total) and all terms are non-negative, so
    |got - want| <= 4 * 2^-24 * want.  The same bits on a second call.  Measured (leaf_mse_sumsq): 0.56 * 2^-24 at worst."""
    from mcquic_amd import ops
    worst = 0.0
    for i, (n, shape) in enumerate(_flat_cases()):
        a, b = R.rand(shape, 2400 + i), R.rand(shape, 2500 + i, 0.5)
        ad, bd = a.to(dev), b.to(dev)
        got = ops.mse(ad, bd)
        want = ((a.double() - b.double()) ** 2).mean()
        e1 = abs(float(got.cpu().double() - want)) / float(want)
        assert e1 <= 4 * EPS32, f"mse n={n}: {e1 / EPS32:.2f} x 2^-24"
        assert torch.equal(ops.mse(ad, bd), got)
        sq = ops.sumsq(ad)
        want = (a.double() ** 2).sum()
        e2 = abs(float(sq.cpu().double() - want)) / float(want)
        assert e2 <= 4 * EPS32, f"sumsq n={n}: {e2 / EPS32:.2f} x 2^-24"
        assert torch.equal(ops.sumsq(ad), sq)
        worst = max(worst, e1, e2)
    record("leaf_mse_sumsq", worst_relative_error_in_eps=worst / EPS32, bar_in_eps=4.0)


def test_clip_by_norm(dev):
    """norm = sqrtf(sumsq) exactly (correctly rounded square root of the kernel's own sum) and within 3 * 2^-24 of the float64 norm
    (sumsq's 4 * 2^-24 halved by the root, plus the root's rounding); x scaled by max_norm / (norm + eps), bit-equal to that in
    float32; `max_norm` above the norm and a NaN norm leave x bit-identical."""
    from mcquic_amd import ops
    for i, (n, shape) in enumerate(_flat_cases()):
        x = R.randn(shape, 2600 + i, 0.7)
        want_norm = float(x.double().pow(2).sum().sqrt())
        xd = x.to(dev)
        sq = ops.sumsq(xd).cpu()
        norm = ops.clip_by_norm_(xd, 0.5 * want_norm, 1e-6).cpu()
        assert torch.equal(norm, R.sqrt_f32(sq)), f"n={n}"
        assert abs(float(norm) - want_norm) <= 3 * EPS32 * want_norm
        assert torch.equal(xd.cpu(), R.clip_f32(x, norm, 0.5 * want_norm, 1e-6)), f"n={n}"
        assert not torch.equal(xd.cpu(), x)
        # above the norm: untouched
        yd = x.to(dev)
        assert torch.equal(ops.clip_by_norm_(yd, 2.0 * want_norm + 1.0, 1e-6).cpu(), norm)
        assert torch.equal(yd.cpu(), x)
        # a NaN in the buffer: the norm is NaN, nothing is scaled
        z = x.clone()
        z.view(-1)[n // 2] = float("nan")
        zd = z.to(dev)
        assert torch.isnan(ops.clip_by_norm_(zd, 1e-3, 1e-6).cpu())
        assert torch.equal(zd.cpu().view(torch.int32), z.view(torch.int32))


# ---- the same values behind other layouts ---------------------------------------------------------------------------------------------------
# Every op takes its tensors through ops._dev (a non-contiguous tensor is copied) -- the first two views of R.views_of test that path.
# The third, a contiguous view one float into its allocation, reaches the kernel as it is unless the wrapper says otherwise.
def _same(fn, tensors, dev, what):
    """fn(*views) == fn(*fresh) bit for bit, for each kind of view of ALL tensors and of each tensor alone."""
    fresh = [t.to(dev) for t in tensors]
    want = fn(*fresh)
    want = want if isinstance(want, (tuple, list)) else (want,)
    kinds = [name for name, _ in R.views_of(fresh[0])]
    for k, kind in enumerate(kinds):
        for which in [None] + (list(range(len(fresh))) if len(fresh) > 1 else []):
            args = [R.views_of(t)[k][1] if which in (None, j) else t for j, t in enumerate(fresh)]
            got = fn(*args)
            got = got if isinstance(got, (tuple, list)) else (got,)
            for g, w_ in zip(got, want):
                if g is None and w_ is None:
                    continue
                assert torch.equal(g, w_), f"{what}: {kind} view of {'all' if which is None else which}"
            for a, t in zip(args, fresh):
                assert torch.equal(a, t), f"{what}: an input was written"


@pytest.mark.parametrize("shape", [(2, 6, 5, 7), (1, 4, 16, 16), (4099,), (2, 64, 32, 32)])
def test_views_add_add3(dev, shape):
    """add_kernel / add3_kernel read a, b (, c) with 128-bit loads (four floats per thread) and never look at the address: they are
    written for 16-byte-aligned tensors.  ops.add / ops.add3 therefore copy an operand whose address is not (ops._dev16); a
    contiguous view one float into its allocation takes that path."""
    from mcquic_amd import ops
    a, b, c = R.randn(shape, 1), R.randn(shape, 2), R.randn(shape, 3)
    _same(lambda p, q: ops.add(p, q), [a, b], dev, "add")
    _same(lambda p, q: (lambda s: (s, ops.silu_twin(s)))(ops.add(p, q, dual_silu=True)), [a, b], dev, "add + twin")
    _same(lambda p, q, r: ops.add3(p, q, r), [a, b, c], dev, "add3")
    off = R.views_of(a.to(dev))[-1][1]
    assert off.data_ptr() % 16 == 4 and ops._dev16(off, "a").data_ptr() % 16 == 0 and ops._dev16(a.to(dev), "a").data_ptr() % 16 == 0


@pytest.mark.parametrize("shape", [(2, 6, 5, 7), (4099,), (2, 64, 32, 32)])
def test_views_elementwise_and_mse(dev, shape):
    """silu_bwd_kernel, axpby_kernel, mse_partial_kernel and mse_bwd_kernel read one float per access: any float-aligned address is
    what they are written for, nothing to fall back to."""
    from mcquic_amd import ops
    a, b, c = R.randn(shape, 4), R.randn(shape, 5), R.randn(shape, 6)
    _same(lambda x, dy: ops.silu_bwd(x, dy), [a, b], dev, "silu_bwd")
    _same(lambda x, dy, o: ops.silu_bwd(x, dy, o), [a, b, c], dev, "silu_bwd + other")
    _same(lambda p, q: (lambda s: (s, ops.silu_twin(s)))(ops.axpby(p, q, 0.3, -1.7, dual_silu=True)), [a, b], dev, "axpby")
    _same(lambda p, q: ops.mse(p, q), [a, b], dev, "mse")
    dl = torch.tensor(0.5, device=dev)
    _same(lambda p, q: ops.mse_bwd(p, q, dl, want_db=True), [a, b], dev, "mse_bwd")


@pytest.mark.parametrize("shape,groups", [((2, 32, 8, 8), 32), ((2, 8, 6, 6), 2), ((1, 6, 5, 7), 3), ((2, 4, 17, 19), 2), ((1, 32, 64, 64), 32)])
def test_views_group_norm(dev, shape, groups):
    """norm.hip reads x (and dy) with 128-bit loads where the run's address is 16-byte aligned and falls back to 4-byte loads where
    it is not (run_moments, gn_load_chunk; its stores go to fresh outputs).  The fallback must be the same arithmetic: the chunked
    kernels (planes of >= 256 pixels) fill the same registers either way; the one-workgroup kernels' moments are summed quad by
    quad on both paths whenever the run is whole quads (before this test existed the fallback summed element by element, and a
    4-byte-aligned view got other bits than its copy).  Forward with statistics and twin, then backward with parameter gradients."""
    from mcquic_amd import ops
    c = shape[1]
    x, dy = R.randn(shape, 7, 2.0) + 0.5, R.randn(shape, 8)
    wt, bs = (R.rand((c,), 9) + 1.5).to(dev), R.rand((c,), 10).to(dev)

    def fwd(t):
        y, mean, rstd = ops.group_norm(t, wt, bs, groups, dual_silu=True, want_stats=True)
        return y, ops.silu_twin(y), mean, rstd

    _same(fwd, [x], dev, "group_norm")
    _, _, mean, rstd = fwd(x.to(dev))
    _same(lambda t, d: ops.group_norm_bwd(t, d, wt, mean, rstd, groups), [x, dy], dev, "group_norm_bwd")
    # and the forward is GroupNorm, at the bar of test_gpu_step_ops.py::test_group_norm_large_runs (equal views prove nothing if both are wrong)
    want = F.group_norm(x.double(), groups, wt.cpu().double(), bs.cpu().double(), 1e-5)
    assert float((fwd(x.to(dev))[0].cpu().double() - want).abs().max()) <= 5e-6 * max(1.0, float(want.abs().max()))


def test_views_sqdiff_and_ms_ssim_loss(dev):
    """sqdiff_sum_u8_kernel reads 16 bytes per load only where both images are 16-byte aligned and their size is a multiple of 16
    (metrics.hip: `vec4`), byte by byte otherwise -- exact integer sums either way; the MS-SSIM loss kernels (msssim_loss.hip) read
    one float per access."""
    from mcquic_amd import ops
    g = torch.Generator().manual_seed(11)
    for shape in ((2, 3, 16, 24), (2, 3, 15, 7)):                  # (the first is whole 16-byte groups: the vector path when aligned)
        x, y = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8), torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
        _same(lambda p, q: ops.sqdiff_sum(p, q), [x, y], dev, "sqdiff_sum")
        want = ((x.long() - y.long()) ** 2).sum(dim=(1, 2, 3))
        assert torch.equal(ops.sqdiff_sum(x.to(dev), y.to(dev)).cpu(), want)
    a, b = R.rand((2, 3, 163, 167), 12), R.rand((2, 3, 163, 167), 13)
    _same(lambda p, q: ops.ms_ssim_loss(p, q), [a, (a + 0.1 * b).clamp(-1, 1)], dev, "ms_ssim_loss")


def test_views_vq_assign(dev):
    """vq_assign_kernel reads the latent one float per lane through buffer loads (the 128-bit loads are on the packed codebook,
    which the library allocates itself)."""
    from mcquic_amd import ops
    cb = ops.PackedCodebook(R.randn((2, 64, 8), 14, 0.5).to(dev))
    x = R.randn((2, 16, 9, 11), 15, 0.5)
    _same(lambda t: ops.vq_assign(t, cb), [x], dev, "vq_assign")


@pytest.mark.parametrize("tile", [0, 0x42, 0x442])
def test_views_conv2d(dev, tile):
    """The convolution reads x one float per lane, but its epilogues read output-shaped side tensors two floats at a time in the
    pixel-pair tile (0x442: `8 adjacent, 8-byte aligned bytes`) and four through the PixelShuffle store, without looking at the
    address: written for 16-byte-aligned tensors (torch's allocations).  ops.conv2d therefore copies x / res / mul / gate_id whose
    address is not (ops._dev16); the views below take that path.  x, res and dsilu_mul, each alone and together."""
    from mcquic_amd import ops
    n, cin, cout, h, w = 2, 128, 128, 12, 16
    x, res, mul = R.randn((n, cin, h, w), 16), R.randn((n, cout, h, w), 17), R.randn((n, cout, h, w), 18)
    wt, b = R.randn((cout, cin, 3, 3), 19, 1.0 / (cin * 9) ** 0.5), R.randn((cout,), 20, 0.1)
    pk = ops.PackedConv(wt.to(dev), b.to(dev))
    _same(lambda t: ops.conv2d(t, pk, 1, tile=tile), [x], dev, "conv x")
    _same(lambda t, r: ops.conv2d(t, pk, 1, res=r, tile=tile), [x, res], dev, "conv x, res")
    _same(lambda t, r, m: ops.conv2d(t, pk, 1, res=r, dsilu_mul=m, tile=tile), [x, res, mul], dev, "conv x, res, dsilu_mul")
    want = F.conv2d(x.double(), wt.double(), b.double(), padding=1) * (lambda s: s * (1 + mul.double() * (1 - s)))(torch.sigmoid(mul.double())) + res.double()
    got = ops.conv2d(x.to(dev), pk, 1, res=res.to(dev), dsilu_mul=mul.to(dev), tile=tile).cpu().double()
    assert float((got - want).abs().max()) <= 3e-6 * float(want.abs().max())
