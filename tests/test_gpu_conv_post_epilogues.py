"""GPU: the fused 1x1 layer behind a 3x3 convolution -- the POST section of conv_mfma_kernel (MCQ_CONV_POST_GDN / _IGDN / _GATE, the
operand order of pack_post1x1_kernel) -- against the float64 references of tests/_conv_refs.py (post64 / post_f32 / post_scale64, held
to the oracle's GDN and to F.conv2d + sigmoid on the CPU by tests/test_conv_refs.py on the very inputs launched here).

The section is the eighth separately written epilogue path of the kernel (tests/test_gpu_conv_epilogues.py pins the other seven): its
own bias add, its own residual read with res_scale, a 64-step contraction over the accumulator registers in their order, three
element-wise closes, a second output address scheme (the four waves of a workgroup store to sub-pixel (2 y + dy, 2 x + dx)), side
loads double-buffered by band.  tests/test_gpu_post.py holds it at max |err| <= 4e-6 max |ref| with one channel count, res_scale 1
and every bias present, which a dropped res_scale, a side value from the wrong band buffer on one band or a twin written over y
passes.  Here every row of ROWS (one keyword set of ops._conv_desc) runs at every geometry of its list (C.POST_GEOMS: the smallest at
which each index can go wrong, N = 2, tile 0x41 forced) and every launch is held to:

  1. y (and the twin) between guard bands, intact afterwards; in gate rows without dual_silu a twin-sized guarded buffer the launch
     is never told about stays untouched and y holds no twin values (it is compared with the gate, not its SiLU); every input --
     x, both operand streams, both biases, the side tensors between bands of a 1e3 sentinel -- equals its clone afterwards;
  2. (a) the close alone: v_gpu = the same 3x3 layer on tile 0x41 without POST flags (accumulator + bias as this instance sums it);
     e_hip_a = max |got - post64(v_gpu)| / post_scale64 against e_seq_a, the same figure for post_f32(v_gpu) -- s as ONE float32
     chain of 128 additions from the bias in the kernel's channel order -- e_hip_a <= max(4 e_seq_a, 1.2e-7).  On the exact rows
     (w1 = a permutation times powers of two: s is the same in any order, a weight in the wrong lane or k-step is an O(1) error)
     the output is held to float32 ulps at the float64 value within 4x the worst ulp error of post_f32 over the same inputs; the
     twin to 4x silu_f32's worst ulp error on the stored y, as the dual_silu rows of tests/test_gpu_conv_epilogues.py;
  3. (b) the whole launch: e_hip = max |got - post64(conv64(x, w, b))| / scale against e_seq of post_f32(conv_seq_f32(...)),
     e_hip <= max(4 e_seq, 1.2e-7);
  4. status MCQ_OK, the 128-row operand section, the POST flag seen by a spy on ops._conv_desc; the number of launches that ran the
     fused instance is asserted against a literal per row.

test_chip_filling_launch takes the fused form by the launcher's own choice (ops.post_ok == 1, no forced tile): the forced launch's
bits, and both bars.  test_post_refusals: the combinations conv_validate / conv_launch refuse, with the output untouched.

Measured on an MI355X (profiles/r14_conv_post_errors.json, 42 entries conv_post[<row>][<geometry>]): the one-chain sum IS a yardstick
for this contraction, and a tight one.  (a): on every GDN / IGDN row e_hip_a equals e_seq_a to the last digit (2.7e-7 .. 5.2e-7: the
64-step MFMA chain lands on the sequential chain's own error), on the gate rows e_hip_a / e_seq_a is 0.87 .. 1.28 (1.37e-7 against
1.07e-7, gate on tiny3x3); the exact rows return the float32 formula's worst ulp error to the digit (GDN 1.50 = 1.50, IGDN 1.47 =
1.47, gate 2.27 = 2.27 ulp), the twin at most 1.25 x silu_f32's (2.44 against 1.95 ulp at the chip-filling map).  (b): e_hip / e_seq
is at most 1.43 for y (gate+res on tiny3x3, 5.3e-8 against 3.7e-8, both below the floor; above the floor 1.31, one permutation of
gdn-exact at stride 2, and 1.23, igdn+shuffle2 on sub5x7, 1.78e-7 against 1.44e-7) and 1.17 for the twin; the largest e_hip is 3.3e-7 (chip:gdn+silu_in) next to an e_seq of 3.3e-7.  No row
needs the factor 4.  Three temporary mutations of the kernel, tried against this file: `p.res_scale *` dropped from the gate's
residual add fails the three res_scale != 1 rows and the chip-filling gate (tests/test_gpu_post.py passes it whole); m[0] for every
band fails all ten gate tests; T >> 1 and T & 1 swapped in opix fails the two shuffle rows, igdn-exact and the chip-filling IGDN."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _conv_refs as C
import _leaf_refs as R
from _record import record
from test_gpu_conv_epilogues import FILL_TWIN, FILL_Y, FLOOR_B, GUARD, _guarded, _launch, _ulps

pytestmark = pytest.mark.gpu

TILE = 0x41                     # the 128 x 32 wave tile: the only instance that carries the POST section; forced, it fuses on any map size
SENTINEL = 1.0e3                # on both sides of every side tensor: a read past its ends changes the result by far more than any bar
SECTION_128 = 1                 # ops.sections_used: the 128-row section of the operand stream
SMALL, UNSHUFFLED, SUB = ("odd7x9", "s2_7x10", "tiny3x3"), ("odd7x9", "tiny3x3"), ("sub5x7", "sub3x3")


def _row(name, kind, geoms, runs, pro=None, bias3=True, bias1=True, res=None, dual=False, variants=("dense",)):
    return dict(name=name, kind=kind, geoms=geoms, runs=runs, pro=pro, bias3=bias3, bias1=bias1, res=res, dual=dual, variants=variants)


# `runs`: launches of the fused instance the row must make = geometries x variants (written out, not computed)
ROWS = [
    _row("gdn", "gdn", SMALL, 3),
    _row("gdn+silu_in", "gdn", SMALL, 3, pro="silu"),
    _row("gdn-bias3", "gdn", SMALL, 3, bias3=False),                         # P_bias == nullptr: the zero-record descriptor on P_wp
    _row("igdn", "igdn", UNSHUFFLED, 2),
    _row("igdn+silu_in", "igdn", UNSHUFFLED, 2, pro="silu"),
    _row("igdn+shuffle2", "igdn", SUB, 2),                                   # post_sub: Cout 512 in sub-pixel-major rows
    _row("igdn+shuffle2+silu_in", "igdn", SUB, 2, pro="silu"),
    _row("gate", "gate", UNSHUFFLED, 2),                                     # no res, no twin
    _row("gate+res", "gate", UNSHUFFLED, 2, res=1.0),
    _row("gate+res_scale-1", "gate", UNSHUFFLED, 2, res=-1.0),
    _row("gate+res_scale0.5", "gate", UNSHUFFLED, 2, res=0.5),
    _row("gate+dual_silu", "gate", UNSHUFFLED, 2, dual=True),
    _row("gate+res_scale0.5+dual_silu", "gate", UNSHUFFLED, 2, res=0.5, dual=True),
    _row("gate-bias1", "gate", UNSHUFFLED, 2, bias1=False),                  # post_b == nullptr
    _row("gate-bias3", "gate", UNSHUFFLED, 2, bias3=False),
    # the exact rows: a cyclic shift by 1, 4 and 32 and a seeded permutation, each times powers of two
    _row("gdn-exact", "gdn", ("odd7x9", "s2_7x10"), 8, variants=C.POST_EXACT),
    _row("igdn-exact", "igdn", ("odd7x9", "sub3x3"), 8, variants=C.POST_EXACT),
    _row("gate-exact", "gate", UNSHUFFLED, 8, dual=True, variants=C.POST_EXACT),
]
assert len(C.POST_EXACT) == 4 and sum(r["runs"] for r in ROWS) == 57          # 3 x 3 + 12 x 2 + 3 x 8


# ---- cases: inputs, packed weights and CPU references, built once and shared ---------------------------------------------------------------
_CASES, _POSTS = {}, {}


class _Case:
    """The producing 3x3 layer at one geometry: what _launch of tests/test_gpu_conv_epilogues.py needs (xd, pk, stride, pro), its three
    CPU references in the output's (shuffled) shape, and v_gpu of tile 0x41."""

    def __init__(self, dev, gname, pro, bias3):
        from mcquic_amd import ops
        g = C.POST_GEOMS[gname]
        self.g, self.stride, self.pro, self.sub = g, g["stride"], pro, g["sub"]
        self.x, self.w, self.b = C.post_problem(gname, bias3)
        wp, bp = C.to_subpixel_rows(self.w, self.b) if self.sub else (self.w, self.b)
        self.pk = ops.PackedConv(wp.to(dev), None if bp is None else bp.to(dev))
        self.xd = self.x.to(dev)
        refs = (C.conv64(self.x, self.w, self.b, self.stride, pro), C.conv_scale64(self.x, self.w, self.b, self.stride, pro),
                C.conv_seq_f32(self.x, self.w, self.b, self.stride, pro))
        self.v64, self.vscale, self.vseq = (F.pixel_shuffle(t, 2) for t in refs) if self.sub else refs
        self._v_gpu = None

    def v_gpu(self):
        """The same layer, tile and prologue without POST flags, as the (shuffled) map the close works on."""
        if self._v_gpu is None:
            rc, v, _, sec = _launch(self, TILE, {}, {})
            assert rc == 0 and sec == SECTION_128, f"plain launch: status {rc}, operand section {sec:#x}"
            self._v_gpu = C.from_subpixel_rows(v) if self.sub else v
            assert self._v_gpu.shape == self.v64.shape
        return self._v_gpu


def _case(dev, gname, pro, bias3):
    key = (gname, pro, bias3)
    if key not in _CASES:
        _CASES[key] = _Case(dev, *key)
    return _CASES[key]


def _post(dev, kind, variant, bias1):
    """(w1, b1 on the CPU, ops.PackedPost of them)."""
    from mcquic_amd import ops
    key = (kind, variant, bias1)
    if key not in _POSTS:
        w1, b1 = C.post_layer(kind, variant, bias1)
        _POSTS[key] = (w1, b1, ops.PackedPost(w1.reshape(128, 128, 1, 1).to(dev), None if b1 is None else b1.to(dev)))
    return _POSTS[key]


def _side_names(row):
    return () if row["kind"] != "gate" else (("res",) if row["res"] is not None else ()) + ("gate_mul", "gate_id")


def _sides_between_sentinels(sides, dev):
    """Every side tensor inside a buffer of SENTINEL (the views are 16-byte aligned, so ops hands them on as they are)."""
    bufs, views = {}, {}
    for k, t in sides.items():
        bufs[k] = torch.full((GUARD + t.numel() + GUARD,), SENTINEL, device=dev)
        views[k] = bufs[k][GUARD:GUARD + t.numel()].view(t.shape)
        views[k].copy_(t)
        assert views[k].data_ptr() % 16 == 0
    return bufs, views


class _Spy:
    """Wraps ops._conv_desc: the flags of every descriptor built."""

    def __init__(self, monkeypatch):
        from mcquic_amd import ops
        self.flags, real = [], ops._conv_desc

        def spy(*a, **kw):
            out = real(*a, **kw)
            self.flags.append(int(out[0].flags))
            return out
        monkeypatch.setattr(ops, "_conv_desc", spy)


def _fused(dev, case, row, post, sides, spy, tile=TILE):
    """One launch of the row's keyword set -> (y, twin or None), item 1 and item 4 of the module docstring asserted."""
    from mcquic_amd import ops
    w1, b1, pp = post
    ep = {f"post_{row['kind']}": pp}
    if case.sub:
        ep["shuffle2"] = True
    if row["dual"]:
        ep["dual_silu"] = True
    if row["res"] is not None:
        ep["res_scale"] = row["res"]
    bufs, views = _sides_between_sentinels(sides, dev)
    inputs = [("x", case.xd), ("w_packed", case.pk.wp), ("post_w", pp.wp)] + [(k, b) for k, b in bufs.items()]
    inputs += [(k, t) for k, t in (("bias", case.pk.bias), ("post_bias", pp.bias)) if t is not None]
    clones = [(k, t, t.clone()) for k, t in inputs]
    unused = _guarded(case.v64.numel(), FILL_TWIN, dev)[0] if row["kind"] == "gate" and not row["dual"] else None
    seen = len(spy.flags)
    rc, y, twin, sec = _launch(case, tile, ep, views)               # (asserts the guard bands of y and of the twin)
    flag = {"gdn": ops.CONV_POST_GDN, "igdn": ops.CONV_POST_IGDN, "gate": ops.CONV_POST_GATE}[row["kind"]]
    assert rc == 0, f"status {rc}"
    assert sec == SECTION_128, f"operand section {sec:#x}"
    assert len(spy.flags) == seen + 1 and spy.flags[-1] & flag, "the descriptor carries no POST flag"
    assert (twin is not None) == row["dual"] and y.shape == case.v64.shape
    assert unused is None or bool((unused == FILL_TWIN).all()), "a twin was stored although none was asked for"
    for k, t, c in clones:
        assert torch.equal(t, c), f"input {k} modified"
    return y, twin


# ---- the two bars --------------------------------------------------------------------------------------------------------------------------
class _Figures:
    """The figures of one (row, geometry), worst over the variants; recorded, then the failures of a row asserted together."""

    def __init__(self, row, gname, fails):
        self.key, self.fig, self.fails = f"conv_post[{row}][{gname}]", {}, fails

    def put(self, **vals):
        for k, v in vals.items():
            self.fig[k] = max(self.fig.get(k, 0.0), float(v))

    def bar(self, what, hip, seq):
        """e_hip <= max(4 e_seq, 1.2e-7); both sides kept."""
        self.put(**{f"{what}_e_hip": hip, f"{what}_e_seq": seq, f"{what}_ratio": hip / max(seq, R.TINY)})
        if hip > max(4.0 * seq, FLOOR_B):
            self.fails.append(f"{self.key} {what}: e_hip {hip:.3e} > max(4 x e_seq {seq:.3e}, {FLOOR_B})")

    def ulp_bar(self, what, gpu, cpu):
        self.put(**{f"{what}_gpu_ulp": gpu, f"{what}_cpu_ulp": cpu})
        if gpu > 4.0 * cpu:
            self.fails.append(f"{self.key} {what}: {gpu:.2f} ulp > 4 x {cpu:.2f} ulp of the float32 formula")

    def close(self):
        ratios = [v for k, v in self.fig.items() if k.endswith("_ratio")]
        record(self.key, value=max(ratios) if ratios else 0.0, bar=4.0, **self.fig)
        print(self.key + ": " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(self.fig.items())))


def _check(fig, case, row, post, sides, y, twin, exact):
    w1, b1, _ = post
    kind, rs = row["kind"], (1.0 if row["res"] is None else row["res"])
    # (a) the close on this instance's own accumulator
    v = case.v_gpu()
    want, f32, scale = C.post64(v, kind, w1, b1, sides, rs), C.post_f32(v, kind, w1, b1, sides, rs), C.post_scale64(v, v.abs(), kind, w1, b1, sides, rs)
    if exact:
        fig.ulp_bar("a_y", _ulps(y, want[0], scale[0]), _ulps(f32[0], want[0], scale[0]))
    else:
        fig.bar("a_y", C.rel_err(y, want[0], scale[0]), C.rel_err(f32[0], want[0], scale[0]))
    if twin is not None:                                            # the twin is silu of the STORED y
        w_t = R.silu64(y)
        fig.ulp_bar("a_twin", _ulps(twin, w_t, None), _ulps(R.silu_f32(y), w_t, None))
    # (b) the whole launch
    want, seq = C.post64(case.v64, kind, w1, b1, sides, rs), C.post_f32(case.vseq, kind, w1, b1, sides, rs)
    scale = C.post_scale64(case.v64, case.vscale, kind, w1, b1, sides, rs)
    fig.bar("b_y", C.rel_err(y, want[0], scale[0]), C.rel_err(seq[0], want[0], scale[0]))
    if twin is not None:
        fig.bar("b_twin", C.rel_err(twin, want[1], scale[1]), C.rel_err(seq[1], want[1], scale[1]))


@pytest.mark.parametrize("row", ROWS, ids=[r["name"] for r in ROWS])
def test_conv_post_epilogue(dev, row, monkeypatch):
    """One keyword set at every geometry (and variant) of its row: items 1 - 4 of the module docstring.  Measured
    (profiles/r14_conv_post_errors.json): e.g. gate+res_scale0.5+dual_silu on odd7x9 (a) 1.37e-7 against 1.17e-7, twin 2.15 ulp against
    the formula's 1.86, (b) 4.7e-8 = 4.7e-8; igdn+shuffle2 on sub5x7 (a) 3.38e-7 = 3.38e-7, (b) 1.78e-7 against 1.44e-7."""
    spy, fails, runs = _Spy(monkeypatch), [], 0
    for gname in row["geoms"]:
        case = _case(dev, gname, row["pro"], row["bias3"])
        sides = C.post_sides(_side_names(row), case.v64.shape)
        fig = _Figures(row["name"], gname, fails)
        for variant in row["variants"]:
            post = _post(dev, row["kind"], variant, row["bias1"])
            try:
                y, twin = _fused(dev, case, row, post, sides, spy)
            except AssertionError as e:
                raise AssertionError(f"{row['name']} {gname} {variant}: {e}") from e
            runs += 1
            _check(fig, case, row, post, sides, y, twin, variant != "dense")
        fig.close()
    assert not fails, "\n  ".join([row["name"] + ":"] + fails)
    assert runs == row["runs"], f"{row['name']}: {runs} fused launches ran, the table says {row['runs']}"


CHIP = [_row("chip:gdn+silu_in", "gdn", ("chip128x256",), 2, pro="silu"),
        _row("chip:igdn+shuffle2+silu_in", "igdn", ("chip_sub128x128",), 2, pro="silu"),
        _row("chip:gate+res_scale0.5+dual_silu", "gate", ("chip128x256",), 2, res=0.5, dual=True)]


@pytest.mark.parametrize("row", CHIP, ids=[r["name"] for r in CHIP])
def test_chip_filling_launch(dev, row, monkeypatch):
    """2048 wave tiles (2 x 128 x 256 pixels; 128 x 128 pixels through the shuffle's four row tiles): ops.post_ok answers 1 and the
    launcher takes the fused form on its own, tile = 0.  The same bits as the forced launch of the same inputs, and both bars."""
    from mcquic_amd import ops
    gname, = row["geoms"]
    spy, fails, runs = _Spy(monkeypatch), [], 0
    case = _case(dev, gname, row["pro"], row["bias3"])
    assert ops.post_ok(case.xd, case.pk, case.stride, row["kind"], shuffle2=case.sub) == 1
    sides = C.post_sides(_side_names(row), case.v64.shape)
    post = _post(dev, row["kind"], "dense", True)
    got = {}
    for tile in (0, TILE):
        got[tile] = _fused(dev, case, row, post, sides, spy, tile)
        runs += 1
    assert torch.equal(got[0][0], got[TILE][0]) and (got[0][1] is None or torch.equal(got[0][1], got[TILE][1])), "the forced launch's bits differ"
    fig = _Figures(row["name"], gname, fails)
    _check(fig, case, row, post, sides, *got[0], False)
    fig.close()
    assert not fails, "\n  ".join([row["name"] + ":"] + fails)
    assert runs == row["runs"] == 2
    _CASES.pop((gname, row["pro"], row["bias3"]))                   # (8 M-element references: not kept for the rest of the session)


# ---- what the launcher refuses -------------------------------------------------------------------------------------------------------------
def _refused(dev, x, pk, stride, n_desc=1, **kw):
    """(status, flags, were both buffers left untouched) of one launch (of `n_desc` copies of the problem in one multi-problem
    launch) with y and a twin-sized buffer between guard bands."""
    from mcquic_amd import _lib, ops
    built = [ops._conv_desc(x, pk, stride, tile=TILE, **kw) for _ in range(n_desc)]
    bufs = []
    for d, y, y2, _keep in built:
        ybuf, yv = _guarded(y.numel(), FILL_Y, dev)
        tbuf, tv = _guarded(y.numel(), FILL_TWIN, dev)
        d.y = yv.data_ptr()
        if y2 is not None:
            d.y_silu = tv.data_ptr()
        bufs += [(ybuf, FILL_Y), (tbuf, FILL_TWIN)]
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    if n_desc == 1:
        rc = _lib.load().mcq_conv2d_f32(ctypes.byref(built[0][0]), stream)
    else:
        rc = _lib.load().mcq_conv2d_multi_f32((_lib.ConvDesc * n_desc)(*[b[0] for b in built]), n_desc, stream)
    torch.cuda.synchronize()
    return rc, built[0][0].flags, all(bool((buf == fill).all()) for buf, fill in bufs)


def test_post_refusals(dev):
    """What conv_validate / conv_launch refuse of the POST flags comes back as MCQ_EINVAL (RuntimeError / ValueError from ops.conv2d)
    with the guarded output untouched: a multi-problem launch, the input-gradient stream of a stride-2 layer (four-tap walk), the
    gate at stride 2 or without its multiplier or identity, GDN through the PixelShuffle store, IGDN through it with Cout 128."""
    from mcquic_amd import _lib, ops
    c1, c2, cs = _case(dev, "odd7x9", None, True), _case(dev, "s2_7x10", None, True), _case(dev, "sub5x7", None, True)
    on = lambda t: t.to(dev)                                         # noqa: E731
    gdn, igdn, gate = (_post(dev, k, "dense", True)[2] for k in ("gdn", "igdn", "gate"))
    s1 = {k: on(t) for k, t in C.post_sides(("gate_mul", "gate_id"), c1.v64.shape).items()}
    s2 = {k: on(t) for k, t in C.post_sides(("gate_mul", "gate_id"), c2.v64.shape).items()}
    lr = ops.PackedConv.dgrad(on(R.randn((20, 128, 3, 3), 1, 0.05)), 2)          # [512, 20, 3, 3], zero outside the lower-right 2 x 2 taps
    assert lr.lr_taps and (lr.cout, lr.cin) == (512, 20)
    # (every row is accepted once its fault is taken away: the rows of test_conv_post_epilogue are those launches)
    refused = [
        ("multi-problem launch", c1, c1.pk, dict(post_gdn=gdn), 2),
        ("dgrad(w, 2) stream", cs, lr, dict(post_igdn=igdn, shuffle2=True), 1),
        ("gate at stride 2", c2, c2.pk, dict(post_gate=gate, **s2), 1),
        ("gate without gate_mul", c1, c1.pk, dict(post_gate=gate, gate_id=s1["gate_id"]), 1),
        ("gate without gate_id", c1, c1.pk, dict(post_gate=gate, gate_mul=s1["gate_mul"]), 1),
        ("gdn + shuffle2", cs, cs.pk, dict(post_gdn=gdn, shuffle2=True), 1),
        ("igdn + shuffle2 with Cout 128", c1, c1.pk, dict(post_igdn=igdn, shuffle2=True), 1),
    ]
    for what, case, pk, kw, n_desc in refused:
        rc, flags, untouched = _refused(dev, case.xd, pk, case.stride, n_desc, **kw)
        assert rc == _lib.MCQ_EINVAL, f"{what}: status {rc}"
        assert untouched, f"{what}: a refused launch wrote its output"
        assert flags & (ops.CONV_POST_GDN | ops.CONV_POST_IGDN | ops.CONV_POST_GATE), what
        if what.startswith("dgrad"):
            assert flags & ops.CONV_TAPS_LR, "the descriptor does not name the four-tap walk"
        if n_desc == 1:
            with pytest.raises((RuntimeError, ValueError)):
                ops.conv2d(case.xd, pk, case.stride, tile=TILE, **kw)
    rc, _, untouched = _refused(dev, c1.xd, c1.pk, 1, 1, post_gdn=gdn)          # (the same helper does launch what is valid)
    assert rc == 0 and not untouched
