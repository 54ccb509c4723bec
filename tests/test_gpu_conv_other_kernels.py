"""GPU: the four convolution kernels tests/test_gpu_conv_epilogues.py does not reach -- conv_head16_kernel (csrc/conv_head16.h: the
decoder's image head, <= 16 output channels on the 16x16x4 instruction, PixelShuffle store) and the three Winograd forms: F(2, 3)
along x (MCQ_CONV_WINOGRAD: launch_wino<4> / launch_wino<2> of conv_mfma_kernel), F(2x2, 3x3) on 32x32x2 (MCQ_CONV_WINOGRAD2D,
csrc/conv_wino32.hip) and on 16x16x4 (MCQ_CONV_WINOGRAD2D16, csrc/conv_wino16.hip) -- against the float64 references of
tests/_conv_refs.py (held to conv64 / the int64 convolution on the CPU by tests/test_conv_refs.py on the inputs launched here).

tests/test_gpu_ops.py holds these kernels at max |err| <= tol max |ref| against float32 F.conv2d (tol 2e-6 for the head, 1e-5 / 2e-5
for the Winograd forms), which a wrong transform row on a half-empty edge tile, a dropped res_scale or a side tensor read at the
wrong address passes.  Here every launch goes through ops._conv_desc + mcq_conv2d_f32 (the launch, guard and bar helpers of
tests/test_gpu_conv_epilogues.py) with y and the twin between guard bands, x / bias / the operand stream / every side tensor compared
with a clone afterwards, the descriptor's flags seen by a spy (the kernel meant is the kernel run) and no section of the general
operand stream recorded under either pointer a fall-back could have read from -- the layer's general stream and the stream the
descriptor names (mcq_conv_sections_used == 0 for both: neither conv_mfma_kernel's direct form nor conv_t16_kernel ran; for the
Winograd forms the routing rests on this, the flags and the exact cases together).  Geometries and
channel counts: C.OTHER_GEOMS / C.OTHER_CHANNELS, N = 2, the smallest at which each index can go wrong.

  (i)   test_exact: integer inputs for which every intermediate of the direct AND of the Winograd arithmetic is an integer below
        2^24 (C.exact_case asserts the bound): the result must be the integer convolution bit for bit, with bias, with - res, and
        through the PixelShuffle store.  The indexing test: no tolerance.
  (ii)  test_random, the whole launch: e_hip = max |got - out64(conv64, sides)| / out_scale64 against e_ref, the same figure for the
        float32 restatement of the SAME algorithm (conv_seq_f32 for head16, wino1d_f32 / wino2d_f32 for the Winograd forms: ONE
        sequential chain over the channels); e_hip <= max(4 e_ref, 1.2e-7).
  (iii) test_random, the epilogue alone: the same kernel without epilogue flags gives v_gpu; the epilogue launch equals
        out_f32(v_gpu, sides) bit for bit where no expf is involved, else lies within 4x the float32 formula's own ulp error.
  (iv)  test_multi_problem_launches: 2 and mcq_conv2d_max_multi() problems with tensors of their own: the single launches' bits.
  (v)   test_winograd_refusals / test_head16_steps_aside: what the launcher refuses (MCQ_EINVAL before any write, in agreement
        with mcq_conv2d_winograd_ok) and where the head kernel hands over to the general one.
  (vi)  test_dgrad_winograd_pack: the input-gradient pack is the forward pack of the transposed, flipped weight, bit for bit.

The number of launches every test made is asserted against a literal.  head16's routing: nothing names the kernel that ran, so
besides sections_used == 0 its result must DIFFER in bits from tile 0x12's on a random case (another summation order: four channels
per k-step) and equal it on an exact case.  The 64- and the 128-row instance of F(2, 3) sum in the same order and cannot be told
apart from outside: the forced tile 0x22 is held to the same bars, not shown to be another kernel.

Measured on an MI355X (profiles/r15_conv_other_kernels_errors.json, entries conv_other[<kernel>][<geometry>][<row>], the worst over
the channel configurations; a failure names the configuration):
the one-chain restatement IS a yardstick for all four kernels, the Winograd forms included -- nobody had measured that.  Worst
e_hip / e_ref over the launches of a class: head16 2.13 (bias on tiny2x2, at Cin 6 -> Cout 3: 8.2e-8 against 3.9e-8, both below the
floor; above the floor 1.72), F(2, 3) 1.35 (res+silu_out on row1x9; twin 1.35, res+dual_silu on odd7x9), 32x32x2 1.36 (res+silu_out
on odd7x9; twin 1.28), 16x16x4 1.45 (res_scale-1 on row1x9; twin 1.46, res+dual_silu on odd7x9); the largest e_hip is 3.3e-7
(head16 + silu_in on wide9x35) next to an e_ref of 3.4e-7, for the Winograd forms 2.4e-7 next to 2.8e-7 (F(2, 3) silu_out on
col5x1).  No kernel needs the factor 4.  (iii): every expf-free launch equals the float32 restatement on its own accumulator bit
for bit; with expf the worst is the formula's own on * silu'(m) (8.16 = 8.16 ulp), and 2.42 ulp for a twin next to silu_f32's 1.93
(16x16x4 on wide9x35).  conv_head16_kernel's `4 q + r < Cout` guard on its bias read protects the read alone: rows >= Cout of the accumulator
are written by no store of the kernel, so no output depends on what is read there and no test of outputs can hold that guard."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _conv_refs as C
import _leaf_refs as R
from _record import record
from test_gpu_conv_epilogues import FILL_TWIN, FILL_Y, FLOOR_B, _Worst, _check_a, _guarded, _guards_ok, _launch

pytestmark = pytest.mark.gpu

KERNELS = ("head16", "wino1d", "wino32", "wino16")
LEVEL = dict(head16=None, wino1d=1, wino32=2, wino16=2)         # `winograd=` of ops.PackedConv / ops._conv_desc


def _wino_flags():
    from mcquic_amd import ops
    return dict(head16=0, wino1d=ops.CONV_WINOGRAD, wino32=ops.CONV_WINOGRAD2D, wino16=ops.CONV_WINOGRAD2D16), \
        ops.CONV_WINOGRAD | ops.CONV_WINOGRAD2D | ops.CONV_WINOGRAD2D16


def _row(name, ep=None, sides=()):
    return dict(name=name, ep=ep or {}, sides=tuple(sides))


W16_ROWS = [
    _row("silu_out", dict(silu_out=True)),
    _row("res", sides=("res",)),
    _row("res_scale-1", dict(res_scale=-1.0), ("res",)),
    _row("res_scale0.5", dict(res_scale=0.5), ("res",)),
    _row("dual_silu", dict(dual_silu=True)),
    _row("res+dual_silu", dict(dual_silu=True, res_scale=-1.0), ("res",)),
    _row("res+silu_out", dict(silu_out=True, res_scale=0.5), ("res",)),
    _row("shuffle2", dict(shuffle2=True)),
]
WINO_ROWS = W16_ROWS[:-1] + [
    _row("mul", sides=("mul",)),
    _row("gate", sides=("gate_mul", "gate_id")),
    _row("dsilu_mul", sides=("dsilu_mul",)),
    _row("dsilu_mul+res", dict(res_scale=-1.0), ("dsilu_mul", "res")),
    _row("shuffle2", dict(shuffle2=True)),
]
HEAD_ROWS = [_row("shuffle2", dict(shuffle2=True))]                # (on each of: bias, silu_in + bias, no bias)
ROWS = dict(head16=HEAD_ROWS, wino1d=WINO_ROWS, wino32=WINO_ROWS, wino16=W16_ROWS)
HEAD_VARIANTS = ((None, True), ("silu", True), (None, False))      # (prologue, bias)
# launches of the kernel under test per geometry, written out: (channel configurations) x (the plain launch + the rows);
# head16: 3 variants x (plain + shuffle2) at Cout 12 / 16, the plain launch alone at Cout 3
RANDOM_RUNS = dict(head16=4 * 6 + 2 * 3, wino1d=8 * 13, wino32=4 * 13, wino16=4 * 9)
EXACT_RUNS = dict(head16=4 * 2 + 2 * 1, wino1d=8 * 3, wino32=4 * 3, wino16=4 * 3)
assert [len(C.OTHER_CHANNELS[k]) for k in KERNELS] == [6, 8, 4, 4] and (len(WINO_ROWS), len(W16_ROWS)) == (12, 8)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
def _pack(dev, kernel, w, b):
    from mcquic_amd import ops
    pk = ops.PackedConv(w.to(dev), None if b is None else b.to(dev), winograd=LEVEL[kernel])
    if kernel == "wino32":                                          # (the binding prefers the 16x16x4 instance where Cin % 16 == 0)
        pk.wino16 = None
    want = dict(head16=None, wino1d=pk.wino, wino32=pk.wino2d, wino16=pk.wino16)[kernel]
    assert (want is not None) == (kernel != "head16") and (kernel != "wino1d" or pk.wino2d is None)
    return pk, (pk.wp if want is None else want)


class _Case:
    """One layer at one geometry: what _launch needs (xd, pk, stride, pro), its CPU references and v_gpu of the kernel under test."""

    def __init__(self, dev, kernel, gname, cin, cout, pro=None, bias=True, exact=None, variant=0):
        self.kernel, self.gname, self.stride, self.pro = kernel, gname, 1, pro
        h, w = C.OTHER_GEOMS[gname]
        if exact is None:
            self.x, self.w, self.b = C.other_problem(kernel, gname, cin, cout, bias, variant)
            self.res = None
        else:
            self.x, self.w, self.b, self.res = C.exact_case(C.OTHER_FORM[kernel], cin, cout, h, w, seed=exact)
        self.pk, self.stream = _pack(dev, kernel, self.w, self.b)
        self.xd = self.x.to(dev)
        self.v64 = C.conv64(self.x, self.w, self.b, 1, pro)
        self.plain, self._sides, self._refs = {}, {}, None

    def refs(self):
        if self._refs is None:
            self.vscale = C.conv_scale64(self.x, self.w, self.b, 1, self.pro)
            self.vseq = C.other_yardstick(self.kernel, self.x, self.w, self.b, self.pro)
            self._refs = True
        return self

    def sides(self, names, shuffle):
        key = (names, shuffle)
        if key not in self._sides:
            n, c, h, w = self.v64.shape
            shape = (n, c // 4, 2 * h, 2 * w) if shuffle else (n, c, h, w)
            scale = dict(res=1.0, mul=1.0, dsilu_mul=2.0, gate_mul=2.0, gate_id=0.5)
            self._sides[key] = {k: R.randn(shape, 177 + 13 * i + c, scale[k]) for i, k in enumerate(names)}
        return self._sides[key]


_CASES = {}


def _case(dev, *key):
    if key not in _CASES:
        _CASES[key] = _Case(dev, *key)
    return _CASES[key]


def _run(case, tile, ep, sides, what):
    """One launch of the kernel under test: guard bands (inside _launch), flags, no general-kernel section recorded under the layer's
    general stream or under the stream the descriptor names, inputs unchanged."""
    from mcquic_amd import _lib, ops
    dev = case.xd.device
    flag, mask = _wino_flags()
    sides_dev = {k: t.to(dev) for k, t in sides.items()}
    watched = [("x", case.xd), ("stream", case.stream)] + list(sides_dev.items()) + ([] if case.pk.bias is None else [("bias", case.pk.bias)])
    clones = [(k, t, t.clone()) for k, t in watched]
    seen, orig = [], ops._conv_desc

    def spy(*a, **kw):
        out = orig(*a, **kw)
        seen.append((int(out[0].flags), int(out[0].w_packed or 0), int(out[0].tile)))
        return out

    ops._conv_desc = spy
    try:
        kw = dict(ep) if LEVEL[case.kernel] is None else dict(ep, winograd=LEVEL[case.kernel])
        rc, y, second, sec = _launch(case, tile, kw, sides_dev)
    finally:
        ops._conv_desc = orig
    assert rc == 0, f"{what}: status {rc}"
    assert len(seen) == 1 and seen[0][0] & mask == flag[case.kernel], f"{what}: flags {seen[0][0]:#x}"
    assert seen[0][1] == case.stream.data_ptr() and seen[0][2] == tile, f"{what}: operand stream / tile of the descriptor"
    sec_stream = int(_lib.load().mcq_conv_sections_used(case.stream.data_ptr()))
    assert sec == 0 and sec_stream == 0, f"{what}: the general kernel's operand section {sec:#x} / {sec_stream:#x} was read"
    for k, t, c in clones:
        assert torch.equal(t, c), f"{what}: input {k} modified"
    return y, second


def _check_whole(fig, cls, what, case, ep, sides, y, second):
    """(ii): the whole launch against float64, the yardstick from the float32 restatement of the same algorithm."""
    case.refs()
    want = C.out64(case.v64, ep, sides)
    scale = C.out_scale64(case.v64, case.vscale, ep, sides)
    ref = C.out_f32(case.vseq, ep, sides)
    for out, got, w64, sc, rf in zip(("y", "second"), (y, second), want, scale, ref):
        if w64 is None:
            continue
        e_hip, e_ref = C.rel_err(got, w64, sc), C.rel_err(rf, w64, sc)
        fig.put(cls, **{f"{out}_e_hip": e_hip, f"{out}_e_ref": e_ref, f"{out}_ratio": e_hip / max(e_ref, 1e-30)})
        if e_hip > max(4.0 * e_ref, FLOOR_B):
            fail_at = _unravel(int(((got.double() - w64).abs() / sc.clamp_min(R.TINY)).argmax()), got.shape)
            fig.fail.append(f"(ii) {what} {out}: e_hip {e_hip:.3e} > max(4 x e_ref {e_ref:.3e}, {FLOOR_B}), worst at (n, c, y, x) = {fail_at}")


def _unravel(i, shape):
    at = []
    for s in reversed(shape):
        at.append(i % s)
        i //= s
    return tuple(reversed(at))


def _first_diff(a, b):
    return _unravel(int((a != b).flatten().nonzero()[0]), a.shape), int((a != b).sum())


def _configs(kernel):
    """(cin, cout, tile, prologue, bias) the kernel runs at every geometry."""
    if kernel == "head16":
        return [(ci, co, t, pro, bias) for ci, co, t in C.OTHER_CHANNELS[kernel] for pro, bias in HEAD_VARIANTS]
    return [(ci, co, t, None, True) for ci, co, t in C.OTHER_CHANNELS[kernel]]


def _geoms(kernel):
    return C.HEAD_GEOMS if kernel == "head16" else C.WINO_GEOMS


KG = [(k, g) for k in KERNELS for g in _geoms(k)]


# ---- (i) exact cases ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,gname", KG, ids=[f"{k}-{g}" for k, g in KG])
def test_exact(dev, kernel, gname):
    """(i) of the module docstring.  A failure names the first pixel and channel that differ."""
    runs = 0
    for n_cfg, (cin, cout, tile) in enumerate(C.OTHER_CHANNELS[kernel]):
        case = _case(dev, kernel, gname, cin, cout, None, True, n_cfg)
        want = case.v64
        assert float(want.abs().max()) < C.EXACT_LIMIT and torch.equal(want, want.round())
        rows = [("bias", {}, {}, want)]
        if kernel != "head16":                                      # (a residual takes the head to the general kernel: test_head16_steps_aside)
            rows.append(("res_scale-1", dict(res_scale=-1.0), dict(res=case.res), want - case.res.double()))
        if cout % 4 == 0:
            rows.append(("shuffle2", dict(shuffle2=True), {}, F.pixel_shuffle(want, 2)))
        for name, ep, sides, w64 in rows:
            what = f"{kernel} {gname} {cin}->{cout} tile={tile:#x} {name}"
            y, _ = _run(case, tile, ep, sides, what)
            runs += 1
            assert y.shape == w64.shape
            if not torch.equal(y.double(), w64):
                at, count = _first_diff(y.double(), w64)
                raise AssertionError(f"{what}: {count} elements differ from the integer convolution, first at (n, c, y, x) = {at}: "
                                     f"{float(y[at])} against {float(w64[at])}")
    assert runs == EXACT_RUNS[kernel], f"{kernel} {gname}: {runs} launches, the table says {EXACT_RUNS[kernel]}"


# ---- (ii) + (iii) random cases ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,gname", KG, ids=[f"{k}-{g}" for k, g in KG])
def test_random(dev, kernel, gname):
    """(ii) and (iii) of the module docstring on every channel configuration and epilogue row of the kernel at one geometry."""
    fig, runs = _Worst(f"{kernel}][{gname}", "conv_other", "(iii)"), 0
    biased = {}
    for cin, cout, tile, pro, bias in _configs(kernel):
        case = _case(dev, kernel, gname, cin, cout, pro, bias)
        cls = f"{cin}->{cout}" + (f"@{tile:#x}" if tile else "") + ("+silu_in" if pro else "") + ("" if bias else "-bias")
        what = f"{kernel} {gname} {cls}"
        if tile not in case.plain:
            case.plain[tile] = _run(case, tile, {}, {}, what + " plain")[0]
        v_gpu = case.plain[tile]
        runs += 1
        head = ("silu_in" if pro else "bias" if bias else "no_bias") if kernel == "head16" else ""
        _check_whole(fig, head or "plain", what + " plain", case, {}, {}, v_gpu, None)
        if kernel == "head16" and pro is None:                      # the bias is the last addition: without it the accumulator itself
            if bias:
                biased[(cin, cout)] = (v_gpu, case.b)
            else:
                vb, b = biased[(cin, cout)]
                assert torch.equal(v_gpu + b.reshape(1, -1, 1, 1), vb), f"{what}: accumulator + bias is not the biased launch"
        for row in ROWS[kernel]:
            if row["ep"].get("shuffle2") and cout % 4:
                continue
            sides = case.sides(row["sides"], bool(row["ep"].get("shuffle2")))
            y, second = _run(case, tile, row["ep"], sides, f"{what} {row['name']}")
            runs += 1
            rcls = f"{head}+{row['name']}" if head else row["name"]
            _check_a(fig, rcls, f"{what} {row['name']}", row["ep"], sides, v_gpu, y, second)
            _check_whole(fig, rcls, f"{what} {row['name']}", case, row["ep"], sides, y, second)
    fig.close()
    assert runs == RANDOM_RUNS[kernel], f"{kernel} {gname}: {runs} launches, the table says {RANDOM_RUNS[kernel]}"


# ---- (iv) multi-problem launches -------------------------------------------------------------------------------------------------------------
MULTI = [("wino1d", 20, 64), ("wino1d", 20, 128), ("wino32", 24, 128), ("wino16", 16, 128)]


@pytest.mark.parametrize("kernel,cin,cout", MULTI, ids=[f"{k}-{ci}-{co}" for k, ci, co in MULTI])
def test_multi_problem_launches(dev, kernel, cin, cout):
    """mcq_conv2d_multi_f32 with 2 and with mcq_conv2d_max_multi() problems at odd7x9, + 0.5 res and the twin: every problem has its
    own x, weights, bias and residual, every y and twin lies between guard bands, and each equals the single launch bit for bit."""
    from mcquic_amd import _lib, ops
    lib = _lib.load()
    cap = int(lib.mcq_conv2d_max_multi())
    flag, mask = _wino_flags()
    ep = dict(res_scale=0.5, dual_silu=True)
    cases = [_case(dev, kernel, "odd7x9", cin, cout, None, True, None, v) for v in range(cap)]
    singles, sides_dev = [], []
    for c in cases:
        sides = c.sides(("res",), False)
        singles.append(_run(c, 0, ep, sides, f"{kernel} single"))
        sides_dev.append({k: t.to(dev) for k, t in sides.items()})
    assert not torch.equal(singles[0][0], singles[1][0])
    launches = 0
    for k in (2, cap):
        built, bufs = [], []
        for c, sd in zip(cases[:k], sides_dev):
            d, y, y2, keep = ops._conv_desc(c.xd, c.pk, 1, winograd=LEVEL[kernel], **ep, **sd)
            assert int(d.flags) & mask == flag[kernel]
            ybuf, yv = _guarded(y.numel(), FILL_Y, dev)
            tbuf, tv = _guarded(y.numel(), FILL_TWIN, dev)
            d.y, d.y_silu = yv.data_ptr(), tv.data_ptr()
            built.append((d, keep))
            bufs.append((ybuf, yv, tbuf, tv, y.shape))
        clones = [(t, t.clone()) for c, sd in zip(cases[:k], sides_dev) for t in (c.xd, c.stream, c.pk.bias, sd["res"])]
        rc = lib.mcq_conv2d_multi_f32((_lib.ConvDesc * k)(*[b[0] for b in built]), k, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        assert rc == 0, f"{kernel} x{k}: status {rc}"
        launches += 1
        for i, ((ybuf, yv, tbuf, tv, shape), (sy, st)) in enumerate(zip(bufs, singles)):
            assert _guards_ok(ybuf, yv.numel(), FILL_Y) and _guards_ok(tbuf, tv.numel(), FILL_TWIN), f"{kernel} x{k}: guard band of problem {i} written"
            assert torch.equal(yv.view(shape).cpu(), sy), f"{kernel} x{k}: y of problem {i} differs from its single launch"
            assert torch.equal(tv.view(shape).cpu(), st), f"{kernel} x{k}: the twin of problem {i} differs from its single launch"
        assert all(torch.equal(t, c) for t, c in clones), f"{kernel} x{k}: an input was modified"
    assert launches == 2


# ---- (v) refusals and the query ----------------------------------------------------------------------------------------------------------------
def test_winograd_refusals(dev):
    """mcq_conv2d_winograd_ok against the status of mcq_conv2d_f32 on raw descriptors, every output pre-filled and compared: the query
    answers by the launcher's own rules (wino_taken, csrc/conv_launch.hip), so on every case here -- the shape rules, the flag
    combinations, each instance's channel multiples, wino16's epilogue set -- it says 0 exactly where the launch is MCQ_EINVAL
    with nothing written, and 1 where it runs.  Every pointer is a real allocation large enough for
    the shape named, so a refusal that failed to happen would still stay inside memory the test owns."""
    from mcquic_amd import _lib, ops
    lib = _lib.load()
    w1, w2, w16 = ops.CONV_WINOGRAD, ops.CONV_WINOGRAD2D, ops.CONV_WINOGRAD2D16
    base = dict(N=2, Cin=128, H=8, W=8, Cout=128, ks=3, stride=1)
    x = torch.zeros((2, 128, 8, 8), device=dev)
    wbuf = torch.zeros(1 << 21, device=dev)                         # larger than any operand stream of a 128 -> 128 layer, all zeros
    side = torch.zeros(2 * 128 * 8 * 8, device=dev)
    numel = 2 * 128 * 8 * 8
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def status(flags, **over):
        g = dict(base, **over)
        ybuf, yv = _guarded(numel, FILL_Y, dev)
        tbuf, tv = _guarded(numel, FILL_TWIN, dev)
        d = _lib.ConvDesc(x.data_ptr(), wbuf.data_ptr(), None, yv.data_ptr(), tv.data_ptr(), side.data_ptr(), side.data_ptr(), side.data_ptr(),
                          g["N"], g["Cin"], g["H"], g["W"], g["Cout"], g["ks"], g["stride"], flags, 1.0, 0)
        rc = lib.mcq_conv2d_f32(ctypes.byref(d), stream)
        torch.cuda.synchronize()
        untouched = bool((ybuf == FILL_Y).all() & (tbuf == FILL_TWIN).all())
        ok = int(lib.mcq_conv2d_winograd_ok(g["N"], g["Cin"], g["H"], g["W"], g["Cout"], g["ks"], g["stride"], flags))
        return rc, untouched, ok

    checked = 0
    for wf in (w1, w2, w16):
        rc, untouched, ok = status(wf)                              # the control: the query grants it and it runs (zero weights: y = 0)
        assert (rc, untouched, ok) == (0, False, 1), f"flag {wf:#x}: the plain launch"
        denied = [("Cout % 64", wf, dict(Cout=96)), ("stride 2", wf, dict(stride=2)), ("1x1", wf, dict(ks=1)),
                  ("SILU_IN", wf | ops.CONV_SILU_IN, {}), ("SQUARE_IN", wf | ops.CONV_SQUARE_IN, {})]
        for what, flags, over in denied:
            rc, untouched, ok = status(flags, **over)
            assert ok == 0 and rc == _lib.MCQ_EINVAL and untouched, f"{what} under flag {wf:#x}: query {ok}, status {rc}, untouched {untouched}"
            checked += 1
        beyond = [("SHUFFLE2 + RESIDUAL", wf | ops.CONV_SHUFFLE2 | ops.CONV_RESIDUAL, {}),
                  ("SHUFFLE2 + DSILU_MUL", wf | ops.CONV_SHUFFLE2 | ops.CONV_DSILU_MUL, {}),
                  ("TAPS_LR", wf | ops.CONV_TAPS_LR, {}), ("SILU_OUT + DUAL_SILU", wf | ops.CONV_SILU_OUT | ops.CONV_DUAL_SILU, {}),
                  ("POST_GDN", wf | ops.CONV_POST_GDN, {}), ("GATE_BWD", wf | ops.CONV_GATE_BWD, {})]
        for what, flags, over in beyond:
            rc, untouched, ok = status(flags, **over)
            assert ok == 0 and rc == _lib.MCQ_EINVAL and untouched, f"{what} under flag {wf:#x}: query {ok}, status {rc}, untouched {untouched}"
            checked += 1
    beyond = [("two flags", w1 | w2, {}), ("two flags", w1 | w16, {}), ("two flags", w2 | w16, {}), ("three flags", w1 | w2 | w16, {}),
              ("WINOGRAD2D Cout % 128", w2, dict(Cout=64)), ("WINOGRAD2D Cin % 8", w2, dict(Cin=20)),
              ("WINOGRAD2D16 Cout % 128", w16, dict(Cout=64)), ("WINOGRAD2D16 Cin % 16", w16, dict(Cin=24)),
              ("WINOGRAD2D16 + MUL", w16 | ops.CONV_MUL, {}), ("WINOGRAD2D16 + GATE", w16 | ops.CONV_GATE, {}),
              ("WINOGRAD2D16 + DSILU_MUL", w16 | ops.CONV_DSILU_MUL, {})]
    for what, flags, over in beyond:
        rc, untouched, ok = status(flags, **over)
        assert ok == 0 and rc == _lib.MCQ_EINVAL and untouched, f"{what}: query {ok}, status {rc}, untouched {untouched}"
        checked += 1
    assert checked == 3 * 11 + 11
    # ... and it grants what each instance carries: those launches run (zero weights, zero side tensors)
    granted = [("64 rows", w1, dict(Cout=64)), ("no flag asks about MCQ_CONV_WINOGRAD", 0, {}), ("SHUFFLE2", w1 | ops.CONV_SHUFFLE2, {}),
               ("MUL", w2 | ops.CONV_MUL, {}), ("DSILU_MUL + RESIDUAL", w2 | ops.CONV_DSILU_MUL | ops.CONV_RESIDUAL, {}),
               ("RESIDUAL + DUAL_SILU", w16 | ops.CONV_RESIDUAL | ops.CONV_DUAL_SILU, {}), ("SHUFFLE2", w16 | ops.CONV_SHUFFLE2, {}),
               ("Cin % 16", w16, dict(Cin=16)), ("Cin % 8", w2, dict(Cin=24))]
    for what, flags, over in granted:
        rc, untouched, ok = status(flags, **over)
        assert (rc, untouched, ok) == (0, False, 1), f"{what} under flags {flags:#x}: status {rc}, untouched {untouched}, query {ok}"
    # the binding steps aside where the 16x16x4 instance has no epilogue: `mul` on a layer packed for it runs the 32x32x2 instance
    c16 = _case(dev, "wino16", "odd7x9", 16, 128, None, True)
    mul = c16.sides(("mul",), False)["mul"].to(dev)
    d, _, _, _ = ops._conv_desc(c16.xd, c16.pk, 1, mul=mul, winograd=2)
    assert int(d.flags) & (w1 | w2 | w16) == w2 and int(d.w_packed) == c16.pk.wino2d.data_ptr()
    d, _, _, _ = ops._conv_desc(c16.xd, c16.pk, 1, res=mul, winograd=2)
    assert int(d.flags) & (w1 | w2 | w16) == w16 and int(d.w_packed) == c16.pk.wino16.data_ptr()


def test_head16_steps_aside(dev):
    """conv_head16_kernel takes a <= 16-channel 3x3 stride-1 layer only with tile 0, one problem and nothing but the PixelShuffle /
    SiLU prologue: a forced tile, a residual, stride 2 or two problems run the general kernel (its 32-row operand section is read)
    and return tile 0x12's bits -- the launcher's own choice for these shapes.  And the routing of the head itself: no general
    section read, bits that DIFFER from tile 0x12's on a random case and equal them on an exact one."""
    from mcquic_amd import _lib, ops
    lib = _lib.load()
    case = _case(dev, "head16", "odd7x9", 128, 12, None, True)
    head = _run(case, 0, {}, {}, "head16")[0]
    rc, g12, _, sec = _launch(case, 0x12, {}, {})
    assert rc == 0 and sec == 4, f"forced tile: status {rc}, section {sec:#x}"
    assert not torch.equal(head, g12), "tile 0 returned the general kernel's bits: did conv_head16_kernel run?"
    exact = _case(dev, "head16", "odd7x9", 128, 12, None, True, 1)
    rc, e12, _, sec = _launch(exact, 0x12, {}, {})
    assert rc == 0 and sec == 4 and torch.equal(_run(exact, 0, {}, {}, "head16 exact")[0], e12)
    res = {"res": case.sides(("res",), False)["res"].to(dev)}
    rc, r0, _, sec0 = _launch(case, 0, dict(res_scale=0.5), res)
    rc2, r12, _, _ = _launch(case, 0x12, dict(res_scale=0.5), res)
    assert (rc, rc2, sec0) == (0, 0, 4) and torch.equal(r0, r12), "a residual must take the general kernel"
    case.stride = 2
    try:
        rc, s0, _, sec0 = _launch(case, 0, {}, {})
        rc2, s12, _, _ = _launch(case, 0x12, {}, {})
    finally:
        case.stride = 1
    assert (rc, rc2, sec0) == (0, 0, 4) and s0.shape == (2, 12, 4, 5) and torch.equal(s0, s12), "stride 2 must take the general kernel"
    other = _case(dev, "head16", "odd7x9", 128, 12, None, True, None, 1)
    rc, o12, _, _ = _launch(other, 0x12, {}, {})
    assert rc == 0
    built, bufs = [], []
    for c in (case, other):
        d, y, _, keep = ops._conv_desc(c.xd, c.pk, 1)
        ybuf, yv = _guarded(y.numel(), FILL_Y, dev)
        d.y = yv.data_ptr()
        built.append((d, keep))
        bufs.append((ybuf, yv, y.shape))
    ops.section_trace(True)
    rc = lib.mcq_conv2d_multi_f32((_lib.ConvDesc * 2)(*[b[0] for b in built]), 2, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    secs = [ops.sections_used(c.pk) for c in (case, other)]
    ops.section_trace(False)
    assert rc == 0 and secs == [4, 4], f"two problems: status {rc}, sections {secs}"
    for (ybuf, yv, shape), want in zip(bufs, (g12, o12)):
        assert _guards_ok(ybuf, yv.numel(), FILL_Y) and torch.equal(yv.view(shape).cpu(), want), "two problems must take the general kernel"


# ---- (vi) the input-gradient pack ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cout,cin", [(128, 64), (64, 192)])
def test_dgrad_winograd_pack(dev, cout, cin):
    """mcq_pack_conv_dgrad_weight_winograd_f32(w) against mcq_pack_conv_weight_winograd_f32 of the explicitly transposed and
    flipped weight: the same values through the same float64 transform give the same bits, in every float of the stream (both
    buffers pre-filled with the same sentinel); and it is what ops.PackedConv.dgrad(w, 1, winograd=True) carries."""
    from mcquic_amd import _lib, ops
    lib = _lib.load()
    w = R.randn((cout, cin, 3, 3), 71 + cout, (cin * 9) ** -0.5)
    wd, keep = w.to(dev), w.clone()
    wt = w.transpose(0, 1).flip(2, 3).contiguous().to(dev)         # [cin, cout, 3, 3]: the stride-1 input-gradient convolution's filter
    n = int(lib.mcq_packed_conv_winograd_floats(cin, cout))
    assert n > 0
    a, b = torch.full((n,), FILL_Y, device=dev), torch.full((n,), FILL_Y, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.mcq_pack_conv_dgrad_weight_winograd_f32(wd.data_ptr(), cout, cin, a.data_ptr(), stream) == 0
    assert lib.mcq_pack_conv_weight_winograd_f32(wt.data_ptr(), cin, cout, b.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(a, b) and float(a.abs().max()) > 0 and not bool((a == FILL_Y).any())
    assert torch.equal(wd.cpu(), keep)
    pk = ops.PackedConv.dgrad(wd, 1, winograd=True)
    assert (pk.cout, pk.cin) == (cin, cout) and torch.equal(pk.wino, a)
