"""CPU: the restatements of tests/_msssim_refs.py (the MS-SSIM loss kernels' own float32 operation order) held to what the project
already trusts -- oracle/metrics_ref.py for the pooling, the blur and the map means, float64 autograd (grads64 of
tests/test_msssim_loss_oracle.py) for the backward -- on the strip shapes of tests/test_gpu_msssim_leaf.py, so that the CPU side
covers the same tile seams.

The backward's yardstick: err = |restated - float64| / S per element, S the float64 sum of the magnitudes of the element's terms
(_msssim_refs.backward), worst per region class, at most 4x the same figure of float32 autograd through the oracle.  Measured here:
the two agree to a few per cent in every class (the float32 maps are the same bits, and their cancellation E[x^2] - mu^2 is the
error): seam 8.8e-7 (2071 x 161) .. 1.7e-5 (161 x 2071) against autograd's 8.4e-7 .. 1.7e-5, border 2.0e-6 .. 9.3e-5 against
2.1e-6 .. 9.3e-5, and 2.8e-4 on both sides at offset 0.5, data range 1.  (No pixel of these shapes is interior: a level-4 side of
11 .. 130 puts every row or column within 10 of an edge there.)

The tests of the tests: on 2071 x 161, a restatement whose transposed blur drops its last tap on the ONE seam column 118 of level 0
(0.62 % of the elements change) differs from the right one in bits, is 5.5e-5 S off float64 in the seam class where the right one is
8.8e-7 (bar 3.5e-6) and has a relative L2 error of 4.2e-5 (1.5e-5 unperturbed) -- inside the 1e-4 bar that was all
tests/test_gpu_msssim_loss.py held the gradient to."""
import numpy as np
import pytest
import torch

import _msssim_refs as R
import test_msssim_loss_oracle as O
from oracle import metrics_ref as M

U = 2.0 ** -24
# (N, C, H, W): the two strips, the ragged one-row / one-column tiles with a second plane, the exact multiples of the tile
SHAPES = [(1, 1, 161, 2071), (1, 1, 2071, 161), (1, 2, 171, 258), (1, 1, 170, 256)]
_CACHE = {}


def inputs(n, c, h, w, half=False):
    """(restored, image) float32 [n, c, h, w], F17 style (make_u8_pair scaled to [-1, 1] plus noise on `restored`); `half`: scaled
    into [-0.5, 0.5] for offset 0.5, data range 1 -- by 0.49, not by 0.5: a power of two would scale every float32 operation
    exactly and make the second pair a copy of the first."""
    seed = h * 1000 + w + n
    k = (c + 2) // 3
    r3, i3 = O.f17_inputs(seed, n * k, h, w)
    r = r3.reshape(n, k * 3, h, w)[:, :c].contiguous()
    i = i3.reshape(n, k * 3, h, w)[:, :c].contiguous()
    return (r * 0.49, i * 0.49) if half else (r, i)


def planes(t):
    return t.reshape(-1, t.shape[-2], t.shape[-1]).numpy()


def grads(restored, image, offset, data_range, dtype):
    """(v [5, N, C], d loss / d restored, d loss / d image) by autograd through the oracle in `dtype` (float64: grads64 of
    test_msssim_loss_oracle.py with the offset and the data range passed on)."""
    r = restored.detach().to(dtype).requires_grad_()
    i = image.detach().to(dtype).requires_grad_()
    if dtype == torch.float64:
        loss, v = O.ms_ssim_loss64(r, i, offset, data_range)
    else:
        x, y = r + offset, i + offset
        win, vs = M.gauss_window(), []
        for lv in range(5):
            s, cs = M.ssim_and_cs(x, y, win, data_range=data_range)
            vs.append(cs if lv < 4 else s)
            if lv < 4:
                x, y = M._halve(x), M._halve(y)
        v = torch.stack(vs)
        loss = 1.0 - torch.prod(torch.relu(v) ** torch.tensor(M.MS_WEIGHTS).view(-1, 1, 1), dim=0).mean()
    loss.backward()
    return v.detach(), r.grad, i.grad


def case(shape, offset=1.0, data_range=2.0):
    """Everything the tests of one shape share, computed once."""
    key = (shape, offset, data_range)
    if key not in _CACHE:
        n, c, h, w = shape
        r, i = inputs(n, c, h, w, half=offset != 1.0)
        a, b = planes(r), planes(i)
        fwd = R.forward(a, b, offset, data_range)
        values = fwd["mean"].astype(np.float32)
        da, db, sa, sb = R.backward(a, b, offset, data_range, values, 1.0, with_scale=True)
        v64, g64, gi64 = grads(r, i, offset, data_range, torch.float64)
        _CACHE[key] = dict(r=r, i=i, a=a, b=b, fwd=fwd, values=values, da=da, db=db, sa=sa, sb=sb, v64=v64, g64=planes(g64), gi64=planes(gi64),
                           cls=R.region_classes(h, w))
    return _CACHE[key]


def test_layout_and_taps():
    assert R.pyramid_sizes(161, 2071) == [(161, 2071), (81, 1036), (41, 518), (21, 259), (11, 130)]
    assert R.pyramid_sizes(171, 258)[1] == (86, 129) and R.pyramid_sizes(170, 256)[1] == (85, 128)
    sizes, off, fl = R.saved_layout(2, 171, 258)
    assert off[1] == 0 and off[2] == 2 * 2 * 86 * 129 and fl == 2 * 2 * sum(hh * ww for hh, ww in sizes[1:])
    assert np.array_equal(R.WIN, M.gauss_window().numpy())
    assert np.array_equal(R.LEVEL_W, np.array(M.MS_WEIGHTS, dtype=np.float32))


@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_pool_blur_and_means_follow_the_oracle(shape):
    """Pooling and blur: the oracle's bits at every level.  Map means: the exact mean of the restated float32 map against the
    oracle's float32 `.mean()` of the same map, within 32 float32 roundings of the mean of the magnitudes (a cascade sum of at most
    2^19 addends is no deeper) -- and within 4x the oracle's own float32 error (+ 1e-9) of float64."""
    k = case(shape)
    n, c, h, w = shape
    x, y = k["r"].float() + 1, k["i"].float() + 1
    win = M.gauss_window()
    for lv in range(5):
        xs = k["fwd"]["xs"][lv]
        assert np.array_equal(xs, planes(x)) and np.array_equal(k["fwd"]["ys"][lv], planes(y)), f"level {lv}: pooling"
        assert np.array_equal(R.blur_valid(xs), planes(M._blur_valid(x, win))), f"level {lv}: blur"
        s, cs = M.ssim_and_cs(x, y, win, data_range=2.0)
        v32 = planes((cs if lv < 4 else s)[..., None]).reshape(-1).astype(np.float64)
        mean, absmean = k["fwd"]["mean"][lv], k["fwd"]["absmean"][lv]
        assert (np.abs(mean - v32) <= 32 * U * absmean).all(), f"level {lv}: map mean"
        v64 = k["v64"][lv].reshape(-1).numpy()
        assert (np.abs(mean - v64) <= 4 * np.abs(v32 - v64) + 1e-9).all(), f"level {lv}: map mean against float64"
        x, y = M._halve(x), M._halve(y)
    assert float(k["v64"].min()) > 0.5, "the inputs must keep every level on the positive side of the relu"


def _errs(k, da, db):
    ea = np.abs(da.astype(np.float64) - k["g64"]) / k["sa"]
    eb = np.abs(db.astype(np.float64) - k["gi64"]) / k["sb"]
    wa, wb = R.worst_by_class(ea, k["cls"]), R.worst_by_class(eb, k["cls"])
    return {c: max(wa[c], wb[c]) for c in wa}


@pytest.mark.parametrize("shape,pair", [(s, (1.0, 2.0)) for s in SHAPES] + [(SHAPES[2], (0.5, 1.0))], ids=str)
def test_backward_is_the_right_mathematics(shape, pair):
    """The restated backward with the restated values against float64 autograd: |err| / S, worst per region class, at most 4x the
    same figure of float32 autograd through the oracle."""
    k = case(shape, *pair)
    _, g32, gi32 = grads(k["r"], k["i"], pair[0], pair[1], torch.float32)
    e_res, e_auto = _errs(k, k["da"], k["db"]), _errs(k, planes(g32), planes(gi32))
    print(shape, pair, "restated", e_res, "float32 autograd", e_auto)
    assert np.isfinite(k["da"]).all() and np.isfinite(k["db"]).all() and float(k["sa"].min()) > 0
    for c in e_res:
        assert e_res[c] <= 4 * e_auto[c], (c, e_res[c], e_auto[c])
    da_only, none, _, _ = R.backward(k["a"], k["b"], pair[0], pair[1], k["values"], 1.0, want_db=False)
    assert none is None and np.array_equal(da_only, k["da"])


@pytest.mark.parametrize("shape", SHAPES[:3], ids=str)
def test_levels_add_up(shape):
    """values = 1, dloss = 1: the whole restatement is the sum of the five per-level restatements (every other level on the exact-zero
    path), to float32 rounding: both sides carry at most 32 roundings of S (the 22 taps and the few products and sums of one level,
    one more sum per finer level), so they differ by at most 64 x 2^-24 S."""
    k = case(shape)
    ones = np.ones((5, k["a"].shape[0]), np.float32)
    da, db, sa, sb = R.backward(k["a"], k["b"], 1.0, 2.0, ones, 1.0, with_scale=True)
    parts = [R.backward(k["a"], k["b"], 1.0, 2.0, ones, 1.0, levels=(l,)) for l in range(5)]
    for got, s, idx in ((da, sa, 0), (db, sb, 1)):
        total = sum(p[idx].astype(np.float64) for p in parts)
        assert all(np.abs(p[idx]).max() > 0 for p in parts)
        assert (np.abs(got - total) <= 64 * U * s).all()


def test_a_wrong_seam_tap_is_caught_where_the_l2_bar_was_blind():
    """The tests of the tests, on the CPU and on the reference alone: on the 2071 x 161 strip, drop the last tap (weight 1.0e-3) of the
    transposed blur on column 118 of level 0, the first column of the second column tile.  Fewer than 1 % of the elements change; the
    bit equality (d) and the float64 bar (f) of tests/test_gpu_msssim_leaf.py both fail, (f) in the seam class and by more than 10x;
    the relative L2 bar of 1e-4 passes."""
    k = case(SHAPES[1])
    bad, bad_b, _, _ = R.backward(k["a"], k["b"], 1.0, 2.0, k["values"], 1.0, fault=(0, 118))
    changed = float((bad != k["da"]).mean())
    rel = float(np.linalg.norm(bad.astype(np.float64) - k["g64"]) / np.linalg.norm(k["g64"]))
    rel_ok = float(np.linalg.norm(k["da"].astype(np.float64) - k["g64"]) / np.linalg.norm(k["g64"]))
    e_bad, e_ok = _errs(k, bad, bad_b), _errs(k, k["da"], k["db"])
    print(f"changed {changed:.3%}, rel L2 {rel:.2e} (unperturbed {rel_ok:.2e}), e_bad {e_bad}, e_ok {e_ok}")
    assert 0 < changed < 0.01
    assert not np.array_equal(bad, k["da"])                                              # (d)
    assert e_bad["seam"] > 10 * max(4 * e_ok["seam"], 1.2e-7)                            # (f), with room
    assert e_bad["border"] == e_ok["border"]                                             # and only the seam class moves
    assert rel <= 1e-4                                                                   # the old bar
