"""GPU: the MS-SSIM loss kernels (csrc/msssim_loss.hip) element by element against tests/_msssim_refs.py -- the kernels' own float32
operation order restated on the CPU, held to the oracle and to float64 autograd by tests/test_msssim_refs.py -- at the shapes where
an index can go wrong: a second (third, ... 18th) column tile at EVERY pyramid level (a level has one only from 129 columns on, so
levels 1..4 need W >= 257 / 513 / 1025 / 2049: no test had run those blocks), row seams at every level, ragged tiles of one row and
of one column, exact multiples of the tile, odd sides at every level, a second plane, a second block of the per-plane kernels
(> 64 planes) and the second lap of msl_combine_kernel's 256-stride loop (> 256 planes).

Every launch goes through the C ABI with buffers of exactly the bytes the *_bytes functions return, each between guard bands that
must be untouched; outputs, `saved` and the workspaces are pre-filled with NaN, so that a float read before it is written or an
output left unwritten ends in a non-finite result, which fails; inputs are compared with clones.

  (a) saved   the bits of the restated pyramids.
  (b) values  the float32 maps are restated exactly and their mean is taken exactly (math.fsum, one division); the kernel's value
              must be the float32 rounding of that mean.  Allowance: the kernel sums the n map values in float64 in a fixed tree and
              divides once; any order of n - 1 float64 additions is within (n - 1) 2^-53 sum |v| of the exact sum, the division, the
              reference's fsum and its division add one 2^-53 each: A = (n + 3) 2^-53 mean |v| (n <= 311211: 3.5e-11 relative, a
              thousandth of half a float32 spacing).  A value passes when it lies between the roundings of mean - A and mean + A.
  (c) loss    against 1 - mean prod relu(v)^w in float64 on the kernel's own values, in spacings of 1 (2^-23); bar: 4x the worst error
              of the same formula op by op in float32 on the CPU (powf, the product level by level) over the same values, at least one
              spacing -- the _ulp_bar rule of tests/test_gpu_leaf_ops.py, worst over all shapes on both sides.
  (d) da, db  crafted values of exactly 1 (pow(1, w) = 1: the scales are the CPU's bits), dloss = 1 and -3: the bits of the restatement;
              the da-only call the same bits.
  (e) da, db  true values: |got - restated| <= c 2^-24 S, S the float64 sum of the magnitudes of the element's terms
              (_msssim_refs.backward), c = 64.  Derivation, u = 2^-24: the two sides differ only in the per-level scale s, by at most one
              float32 spacing (2u relative) where the device's float64 pow and the host's round apart.  Each gradient-map entry is
              fl(s g): 2u from s plus one rounding a side, 4u |g|.  The transposed blur carries that through linearly (4u B'|g|) and
              adds its own roundings, 11 products and 10 sums a pass, two passes: 22u B'|g| a side to first order, 44u for the two.
              d = (b0 + (2x) b1) + y b2: two products and two sums, 3u a side, 6u; + dnext * 0.25: one sum a side, 2u.  56u in all,
              relative to the level's share of S; the pool adjoint hands the coarser levels' shares on unchanged.  c = 64 leaves an
              eighth for the second-order terms.
  (f) da, db  against float64 autograd: e = max |err| / S per region class (_msssim_refs.region_classes), e_hip <= max(4 e_f32, 1.2e-7),
              e_f32 the restatement's own figure; the strips, both (offset, data range) pairs.  (The float32 maps carry the cancellation
              E[x^2] - mu^2: e_f32 is 1e-6 .. 1e-4, which is why (d) and (e) exist.)
  (g)         a plane whose level-2 value is relu'd away has exactly zero gradients, the other plane the restatement's bits;
              dloss = 0 gives zeros.

Measured on an MI355X (profiles/r12_msssim_leaf_errors.json, keys msssim_leaf[...]): (a) and (d) equal on every shape; (b) 0 of 160 values
off the nearest float32; (c) 0.99 spacings, the float32 formula's own 0.99; (e) 0 of 4.97 M elements differ at all (the device's pow and
the host's rounded alike); (f) e_hip = e_f32 to every digit.  No kernel needed a change: the cause of a future mismatch belongs next to
the test that finds it."""
import ctypes

import numpy as np
import pytest
import torch

import _msssim_refs as R
import test_msssim_refs as T
from _record import record

pytestmark = pytest.mark.gpu

GUARD = 1 << 16                 # floats either side of every buffer
SENTINEL = 7.5
U = 2.0 ** -24
C_E = 64.0                      # (e), derived in the module docstring
FLOOR_F = 1.2e-7                # (f): two float32 roundings
PAIRS = ((1.0, 2.0), (0.5, 1.0))
# (N, C, H, W), backward run too
CASES = {
    "wide": ((1, 1, 161, 2071), True),       # 18 / 9 / 5 / 3 / 2 column tiles at levels 0..4, the last one 2 wide; the level-4 map one row high
    "tall": ((1, 1, 2071, 161), True),       # row seams at every level
    "ragged": ((1, 2, 171, 258), True),      # an 11th row tile of one row, a second column tile of one column at level 1, a second plane
    "even": ((1, 1, 170, 256), True),        # Ho = 160 and a level-1 map of 118 columns: no ragged tile
    "n65": ((65, 1, 161, 161), True),        # a second block of msl_dv_kernel / msl_finish_kernel
    "p258": ((86, 3, 161, 161), False),      # the second lap of msl_combine_kernel
}
BWD = [k for k, v in CASES.items() if v[1]]
_RUNS = {}


class _Buf:
    """`nbytes` of device memory filled with `fill` between two guard bands."""

    def __init__(self, nbytes, dev, fill=float("nan")):
        assert nbytes > 0 and nbytes % 4 == 0
        self.n = nbytes // 4
        self.all = torch.full((2 * GUARD + self.n,), SENTINEL, device=dev)
        self.t = self.all[GUARD:GUARD + self.n]
        self.t.fill_(fill)

    def set(self, src):
        self.t.copy_(torch.as_tensor(src).reshape(-1))
        return self

    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def intact(self):
        return bool((self.all[:GUARD] == SENTINEL).all() & (self.all[GUARD + self.n:] == SENTINEL).all())


def _sizes(shape):
    from mcquic_amd import _lib
    lib = _lib.load()
    n, c, h, w = shape
    sb, wf, wb = (lib.mcq_ms_ssim_loss_saved_bytes(n, c, h, w), lib.mcq_ms_ssim_loss_workspace_bytes(n, c, h, w, 0),
                  lib.mcq_ms_ssim_loss_workspace_bytes(n, c, h, w, 1))
    assert sb == 4 * R.saved_layout(n * c, h, w)[2] and wf == R.workspace_bytes(n * c, h, w, 0) and wb == R.workspace_bytes(n * c, h, w, 1)
    return lib, sb, wf, wb


def _finish(rc, what, bufs, inputs):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                       # a device fault: nothing more of this session may touch the GPU
        pytest.exit(f"{what}: {e}", returncode=3)
    assert rc == 0, f"{what}: status {rc}"
    for name, b in bufs.items():
        assert b.intact(), f"{what}: guard band of `{name}` written"
    for name, (b, clone) in inputs.items():
        assert torch.equal(b.t, clone), f"{what}: input `{name}` changed"


def _forward(dev, shape, a, b, offset, data_range):
    """One mcq_ms_ssim_loss_f32 launch -> (loss, values [5, P], saved) on the CPU."""
    lib, sb, wf, _ = _sizes(shape)
    n, c, h, w = shape
    p = n * c
    A, B = _Buf(a.nbytes, dev).set(a), _Buf(b.nbytes, dev).set(b)
    ca, cb = A.t.clone(), B.t.clone()
    out = dict(loss=_Buf(4, dev), values=_Buf(5 * p * 4, dev), saved=_Buf(sb, dev), workspace=_Buf(wf, dev))
    rc = lib.mcq_ms_ssim_loss_f32(A.ptr(), B.ptr(), offset, data_range, out["loss"].ptr(), out["values"].ptr(), out["saved"].ptr(),
                                  out["workspace"].ptr(), n, c, h, w, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _finish(rc, f"forward {shape}", dict(out, a=A, b=B), dict(a=(A, ca), b=(B, cb)))
    loss, values, saved = out["loss"].t.cpu(), out["values"].t.cpu().view(5, p), out["saved"].t.cpu()
    assert torch.isfinite(loss).all() and torch.isfinite(values).all() and torch.isfinite(saved).all(), f"forward {shape}: non-finite result"
    return float(loss), values.numpy(), saved.numpy()


def _backward(dev, shape, a, b, offset, data_range, values, saved, dloss, want_db=True):
    """One mcq_ms_ssim_loss_bwd_f32 launch -> (da, db or None) [P, H, W] on the CPU."""
    lib, sb, _, wb = _sizes(shape)
    n, c, h, w = shape
    ins = dict(a=_Buf(a.nbytes, dev).set(a), b=_Buf(b.nbytes, dev).set(b), values=_Buf(values.nbytes, dev).set(values),
               saved=_Buf(sb, dev).set(saved), dloss=_Buf(4, dev).set(np.float32([dloss])))
    clones = {k: (v, v.t.clone()) for k, v in ins.items()}
    out = dict(da=_Buf(a.nbytes, dev), workspace=_Buf(wb, dev))
    if want_db:
        out["db"] = _Buf(a.nbytes, dev)
    rc = lib.mcq_ms_ssim_loss_bwd_f32(ins["a"].ptr(), ins["b"].ptr(), offset, data_range, ins["values"].ptr(), ins["saved"].ptr(),
                                      ins["dloss"].ptr(), out["da"].ptr(), out["db"].ptr() if want_db else None, out["workspace"].ptr(),
                                      n, c, h, w, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _finish(rc, f"backward {shape}", dict(out, **ins), clones)
    da = out["da"].t.cpu().view(n * c, h, w)
    db = out["db"].t.cpu().view(n * c, h, w) if want_db else None
    assert torch.isfinite(da).all() and (db is None or torch.isfinite(db).all()), f"backward {shape}: non-finite gradient"
    return da.numpy(), (None if db is None else db.numpy())


def _run(dev, name, pair):
    """Inputs, the restated forward and the device's forward of one (case, pair), once."""
    key = (name, pair)
    if key not in _RUNS:
        shape = CASES[name][0]
        n, c, h, w = shape
        r, i = T.inputs(n, c, h, w, half=pair[0] != 1.0)
        a, b = T.planes(r), T.planes(i)
        sel = None if n * c <= 65 else [0, 1, 63, 64, 255, 256, 257]          # (b) on both laps; (a) and (c) on every plane
        if n * c == 65:
            sel = [0, 31, 63, 64]                                             # both blocks of msl_finish_kernel
        ref = R.forward(a, b, pair[0], pair[1], planes=sel)
        loss, values, saved = _forward(dev, shape, a, b, pair[0], pair[1])
        _RUNS[key] = dict(shape=shape, r=r, i=i, a=a, b=b, ref=ref, sel=sel if sel is not None else list(range(n * c)), loss=loss,
                          values=values, saved=saved)
    return _RUNS[key]


def _tag(name, pair):
    return f"{name},off{pair[0]:g},L{pair[1]:g}"


@pytest.mark.parametrize("pair", PAIRS, ids=str)
@pytest.mark.parametrize("name", list(CASES))
def test_forward_saved_and_values(dev, name, pair):
    """(a) and (b).  Measured (msssim_leaf[fwd,...]): every `saved` float equal; of the values (5 per plane), `off_nearest` are not
    the float32 nearest to the exact mean -- 0 on every shape at both pairs -- and `worst_units`, the largest |value - mean| in units of
    half a float32 spacing (of the rounded mean: 1.0 where that is the power of two above), never exceeds 1."""
    k = _run(dev, name, pair)
    assert np.array_equal(k["saved"], k["ref"]["saved"]), f"saved differs in {int((k['saved'] != k['ref']['saved']).sum())} floats"
    n, c, h, w = k["shape"]
    off_nearest, worst = 0, 0.0
    for lv, (hl, wl) in enumerate(R.pyramid_sizes(h, w)):
        count = (hl - 10) * (wl - 10)
        mean, allow = k["ref"]["mean"][lv], (count + 3) * 2.0 ** -53 * k["ref"]["absmean"][lv]
        got = k["values"][lv][k["sel"]]
        lo, hi = (mean - allow).astype(np.float32), (mean + allow).astype(np.float32)
        off_nearest += int((got != mean.astype(np.float32)).sum())
        worst = max(worst, float((np.abs(got.astype(np.float64) - mean) / (np.spacing(np.abs(mean).astype(np.float32)) / 2)).max()))
        assert ((lo <= got) & (got <= hi)).all(), f"level {lv}: values {got} are not the float32 rounding of the exact means {mean} (+- {allow})"
    record(f"msssim_leaf[fwd,{_tag(name, pair)}]", saved_floats=k["saved"].size, saved_equal=True, values_checked=5 * len(k["sel"]),
           off_nearest=off_nearest, worst_units=worst)
    print(f"{_tag(name, pair)}: saved {k['saved'].size} floats equal; values off nearest {off_nearest} of {5 * len(k['sel'])}, worst {worst:.4f} half spacings")


@pytest.mark.parametrize("pair", PAIRS, ids=str)
def test_loss_from_values(dev, pair):
    """(c), worst over the six shapes (1 .. 258 planes: a second lap of the combine loop on the last).  Measured (msssim_leaf[loss,...]):
    kernel 0.987 spacings, float32 formula on the CPU 0.987, bar 3.95 at (1, 2); 0.446, 0.446 and 1.78 at (0.5, 1)."""
    gpu = cpu = 0.0
    for name in CASES:
        k = _run(dev, name, pair)
        want = R.loss64(k["values"])
        gpu = max(gpu, abs(k["loss"] - want) / 2.0 ** -23)
        cpu = max(cpu, abs(float(R.loss_f32(k["values"])) - want) / 2.0 ** -23)
        assert 0.0 < k["loss"] < 0.5
    bar = max(4.0 * cpu, 1.0)
    record(f"msssim_leaf[loss,off{pair[0]:g},L{pair[1]:g}]", gpu_spacings=gpu, cpu_f32_formula_spacings=cpu, bar_spacings=bar)
    print(f"loss {pair}: gpu {gpu:.3f} spacings of 1, float32 formula on the CPU {cpu:.3f}, bar {bar:.3f}")
    assert gpu <= bar


def _explain(k, got, want, what, values, dloss):
    """Name the first differing element: pixel, region class, and -- from the per-level restatements -- the level."""
    n, c, h, w = k["shape"]
    bad = np.argwhere(got != want)
    p, r, col = (int(v) for v in bad[0])
    cls = R.CLASS_NAMES[R.region_classes(h, w)[r, col]]
    idx = 0 if what == "da" else 1
    parts = [R.backward(k["a"][p:p + 1], k["b"][p:p + 1], 1.0, 2.0, values[:, p:p + 1], dloss / values.shape[1], levels=(l,))[idx][0, r, col] for l in range(5)]
    diff = float(got[p, r, col]) - float(want[p, r, col])
    where = R.pixel_levels(h, w, r, col)
    marked = [l for l, _, _, seam, edge in where if seam or edge]
    level = max(marked) if marked else int(np.argmax(np.abs(parts)))
    return (f"{what}: {len(bad)} of {got.size} elements differ; first at plane {p}, pixel ({r}, {col}), class {cls}: got {got[p, r, col]!r}, "
            f"restated {want[p, r, col]!r}, diff {diff:.3e}; suspect level {level} (on a seam / edge at levels {marked}; per-level "
            f"contributions {[float(v) for v in parts]}; (level, row, column, seam, edge) {where})")


def _ones(k):
    return np.ones((5, k["a"].shape[0]), np.float32)


@pytest.mark.parametrize("name", BWD)
def test_backward_bits_with_unit_values(dev, name):
    """(d): values = 1, dloss = 1 and -3; da and db the restatement's bits, the da-only call the same da.  Measured
    (msssim_leaf[bwd_exact,...]): 0 differing elements on every shape."""
    k = _run(dev, name, PAIRS[0])
    values = _ones(k)
    differing = 0
    for dloss in (1.0, -3.0):
        da, db = _backward(dev, k["shape"], k["a"], k["b"], 1.0, 2.0, values, k["saved"], dloss)
        ra, rb, _, _ = R.backward(k["a"], k["b"], 1.0, 2.0, values, dloss)
        differing += int((da != ra).sum()) + int((db != rb).sum())
        record(f"msssim_leaf[bwd_exact,{name}]", elements=2 * da.size, differing=differing)
        assert np.array_equal(da, ra), _explain(k, da, ra, "da", values, dloss)
        assert np.array_equal(db, rb), _explain(k, db, rb, "db", values, dloss)
        assert float(np.abs(da).max()) > 0 and float(np.abs(db).max()) > 0
        if dloss == 1.0:
            da_only, none = _backward(dev, k["shape"], k["a"], k["b"], 1.0, 2.0, values, k["saved"], dloss, want_db=False)
            assert none is None and np.array_equal(da_only, da), "the da-only call gives other bits"


@pytest.mark.parametrize("name", BWD)
def test_backward_with_true_values(dev, name):
    """(e): the device's own values; |got - restated| <= 64 x 2^-24 S (derived in the module docstring).  Measured
    (msssim_leaf[bwd_true,...]): `worst` = max |diff| / (2^-24 S) and `differing`, the elements that differ at all: 0 and 0 on every shape."""
    k = _run(dev, name, PAIRS[0])
    da, db = _backward(dev, k["shape"], k["a"], k["b"], 1.0, 2.0, k["values"], k["saved"], 1.0)
    ra, rb, sa, sb = R.backward(k["a"], k["b"], 1.0, 2.0, k["values"], 1.0, with_scale=True)
    assert float(sa.min()) > 0 and float(sb.min()) > 0
    worst = max(float((np.abs(da.astype(np.float64) - ra) / (U * sa)).max()), float((np.abs(db.astype(np.float64) - rb) / (U * sb)).max()))
    differing = int((da != ra).sum()) + int((db != rb).sum())
    record(f"msssim_leaf[bwd_true,{name}]", worst=worst, bar=C_E, differing=differing, elements=2 * da.size)
    print(f"{name}: worst |diff| / (2^-24 S) {worst:.3f} (bar {C_E}), {differing} of {2 * da.size} elements differ")
    assert worst <= C_E


@pytest.mark.parametrize("pair", PAIRS, ids=str)
@pytest.mark.parametrize("name", ["wide", "tall"])
def test_backward_against_float64(dev, name, pair):
    """(f): per region class e_hip <= max(4 e_f32, 1.2e-7).  Measured (msssim_leaf[bwd_f64,...]) at offset 1, data range 2: 161 x 2071 seam
    1.66e-5 and border 2.16e-5, 2071 x 161 seam 8.8e-7 and border 9.3e-5, e_hip and e_f32 the same figure each time."""
    k = _run(dev, name, pair)
    n, c, h, w = k["shape"]
    da, db = _backward(dev, k["shape"], k["a"], k["b"], pair[0], pair[1], k["values"], k["saved"], 1.0)
    values_ref = k["ref"]["mean"].astype(np.float32)
    ra, rb, sa, sb = R.backward(k["a"], k["b"], pair[0], pair[1], values_ref, 1.0, with_scale=True)
    _, g64, gi64 = T.grads(k["r"], k["i"], pair[0], pair[1], torch.float64)
    g64, gi64, cls = T.planes(g64), T.planes(gi64), R.region_classes(h, w)

    def errs(xa, xb):
        wa = R.worst_by_class(np.abs(xa.astype(np.float64) - g64) / sa, cls)
        wb = R.worst_by_class(np.abs(xb.astype(np.float64) - gi64) / sb, cls)
        return {c_: max(wa[c_], wb[c_]) for c_ in wa}

    e_hip, e_f32 = errs(da, db), errs(ra, rb)
    fails = []
    for c_ in e_hip:
        record(f"msssim_leaf[bwd_f64,{_tag(name, pair)},{c_}]", e_hip=e_hip[c_], e_f32=e_f32[c_], bar=max(4 * e_f32[c_], FLOOR_F))
        print(f"{_tag(name, pair)} {c_}: e_hip {e_hip[c_]:.3e}, e_f32 {e_f32[c_]:.3e}")
        if e_hip[c_] > max(4 * e_f32[c_], FLOOR_F):
            fails.append((c_, e_hip[c_], e_f32[c_]))
    assert not fails, fails


def test_relu_zero_plane_and_zero_dloss(dev):
    """(g) on the two planes of `ragged`: plane 1 with v_2 = -0.1 has da = db = 0 exactly, plane 0 the restatement's bits; dloss = 0
    gives zeros everywhere."""
    k = _run(dev, "ragged", PAIRS[0])
    values = _ones(k)
    values[2, 1] = -0.1
    da, db = _backward(dev, k["shape"], k["a"], k["b"], 1.0, 2.0, values, k["saved"], 1.0)
    ra, rb, _, _ = R.backward(k["a"], k["b"], 1.0, 2.0, values, 1.0)
    assert not da[1].any() and not db[1].any() and not ra[1].any() and not rb[1].any()
    assert np.array_equal(da[0], ra[0]) and np.array_equal(db[0], rb[0]) and da[0].any() and db[0].any()
    da, db = _backward(dev, k["shape"], k["a"], k["b"], 1.0, 2.0, k["values"], k["saved"], 0.0)
    assert not da.any() and not db.any()
