"""The adaptive-quantisation leaf kernels (csrc/rate_activity.hip: `ops.activity_cells`, `ops.activity_weights`) against the float64
restatement of tests/_activity_ref.py, on the smallest geometries at which the indexing can go wrong: 128 x 128 (no padding), 130 x 200
(both axes padded, even split), 129 x 257 (127 + 127 with the odd splits 63 / 64: the reflection reaches almost the whole image), with 1
and 3 different images.

Bars.  Constant and piecewise-constant images: exact (a = -14, w = 1).  Position in the batch: image i of a batch of 3 gives the bits of
that image run alone.  Products with roi and lam: float32 (w * roi) * lam, bit for bit.  Noise against float64, with u = 2^-24:

  The kernel's sums of 256 terms are balanced trees of depth 8 (a lane adds its four values as (a + b) + (c + d), six butterfly steps add
  the lanes), so a sum carries 8 roundings.  A centred luma Y - mu then carries 3 (luma: one product, two fma) + 8 (the mean) + 1 (the
  difference) = 12 roundings of values of magnitude <= 1 (the images lie in [-1, 1]): |error| <= delta = (T + 4) u with T = 10.  That moves
  v = sum (Y - mu)^2 / 256 by at most 2 delta sqrt(v) + delta^2 (Cauchy-Schwarz); the square, the tree and the + 2^-14 add 1 + 8 + 1 = T
  relative roundings, T u v.  log2 divides by (v + 2^-14) ln 2 and rounds its own result:

      |a - a_ref| <= (2 delta sqrt(v_ref) + delta^2 + T u v_ref) / ((v_ref + 2^-14) ln 2) + 2 u |a_ref|          (tol_a)
      |w / w_ref - 1| <= ln 2 * strength * (tol_a(cell) + max tol_a) + 4 u                                        (tol_w)

  (the mean of a is off by at most the worst cell's tol_a; 4 u: the difference, the product, exp2).  A cell whose exponent lies within
  strength * (tol_a(cell) + max tol_a) of a clip boundary may fall on either side of the clamp and is excused; at most 1 % of a case's
  cells may be, which tests/test_activity_ref.py shows the float64 reference alone to satisfy on these seeds."""
import numpy as np
import pytest
import torch

import _activity_ref as AR

pytestmark = pytest.mark.gpu

STRENGTHS = (0.5, 1.0)
CLIP = 2.0


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(t):
    return t.cpu().numpy().view(np.int32)


_REFS = {}


def _ref(kind, n, h, w):
    """One seeded case, made once and left unchanged: (x, a_ref, v_ref, mask_ref)."""
    key = (kind, n, h, w)
    if key not in _REFS:
        x = AR.make_image(kind, n, h, w, seed=0)
        _REFS[key] = (x,) + AR.cells(x)
    return _REFS[key]


@pytest.mark.parametrize("h, w", AR.GEOMS)
def test_constant_images_are_exact(dev, h, w):
    from mcquic_amd import ops
    x = np.empty((3, 3, h, w), dtype=np.float32)
    x[0, 0], x[0, 1], x[0, 2] = 0.3, -0.7, 0.11
    x[1], x[2] = -1.0, 0.123456
    a, mask, err = ops.activity_cells(_t(x, dev))
    h0, w0 = -(-h // 128) * 8, -(-w // 128) * 8
    assert tuple(a.shape) == tuple(mask.shape) == (3, h0, w0) and a.dtype == torch.float32 and mask.dtype == torch.int32
    assert bool((a == -14.0).all()) and int(mask.sum()) == 0 and err.tolist() == [0, 0, 0]
    for strength in (0.0,) + STRENGTHS:
        assert bool((ops.activity_weights(a, mask, strength, CLIP) == 1.0).all())


def test_piecewise_constant_cells_are_exact(dev):
    """v = 0 in every cell (no padding here: a reflected border would cut the cells), whatever the cell's level."""
    from mcquic_amd import ops
    rng = np.random.default_rng(3)
    levels = rng.uniform(-1, 1, size=(3, 3, 16, 8)).astype(np.float32)
    x = np.repeat(np.repeat(levels, 16, axis=2), 16, axis=3)
    assert x.shape == (3, 3, 256, 128)
    a, mask, err = ops.activity_cells(_t(x, dev))
    assert bool((a == -14.0).all()) and int(mask.sum()) == 0 and int(err.sum()) == 0
    assert bool((ops.activity_weights(a, mask, 1.0, CLIP) == 1.0).all())


@pytest.mark.parametrize("h, w", AR.GEOMS)
def test_noise_cells_cost_more_lambda_than_flat_ones(dev, h, w):
    from mcquic_amd import ops
    rng = np.random.default_rng([4, h, w])
    x = np.full((2, 3, h, w), 0.25, dtype=np.float32)
    x[..., w // 2:] = rng.uniform(-1, 1, size=(2, 3, h, w - w // 2)).astype(np.float32)
    a_ref, v_ref, _ = AR.cells(x)
    flat, noise = a_ref == -14.0, a_ref > -6.0
    assert flat.sum() >= 8 and noise.sum() >= 8
    a, mask, _ = ops.activity_cells(_t(x, dev))
    for strength in STRENGTHS:
        wt = ops.activity_weights(a, mask, strength, CLIP).cpu().numpy()
        for i in range(2):
            assert wt[i][noise[i]].min() > wt[i][flat[i]].max()


@pytest.mark.parametrize("kind", AR.KINDS)
@pytest.mark.parametrize("h, w", AR.GEOMS)
def test_noise_against_float64_and_alone_against_in_a_batch(dev, h, w, kind):
    from mcquic_amd import ops
    x, a_ref, v_ref, mask_ref = _ref(kind, 3, h, w)
    xd = _t(x, dev)
    a, mask, err = ops.activity_cells(xd)
    assert int(mask.sum()) == 0 and int(err.sum()) == 0 and not mask_ref.any()
    ta = AR.tol_a(v_ref, a_ref)
    da = np.abs(a.cpu().numpy().astype(np.float64) - a_ref)
    print(f"{kind} {h}x{w}: a in [{a_ref.min():.2f}, {a_ref.max():.2f}], worst |a - a_ref| / tol {np.max(da / ta):.3f}")
    assert (da <= ta).all()
    maps = {}
    for strength in STRENGTHS:
        wt = maps[strength] = ops.activity_weights(a, mask, strength, CLIP)
        w_ref, _ = AR.weights(a_ref, mask_ref, strength, CLIP)
        rel = np.abs(wt.cpu().numpy().astype(np.float64) / w_ref - 1.0)
        tw = AR.tol_w(ta, strength)
        near = AR.near_clip(a_ref, mask_ref, ta, strength, CLIP)
        excused = (rel > tw) & near
        print(f"  strength {strength}: w in [{w_ref.min():.3f}, {w_ref.max():.3f}], worst |w / w_ref - 1| / tol {np.max(rel[~near] / tw[~near]):.3f}, "
              f"{int(excused.sum())} of {rel.size} excused")
        assert (rel[~near] <= tw[~near]).all()
        assert near.sum() <= AR.EXCUSED_CAP * near.size
    # each image alone: the bits of its rows in the batch
    for i in range(3):
        a1, mask1, err1 = ops.activity_cells(xd[i:i + 1].clone())
        assert np.array_equal(_bits(a1[0]), _bits(a[i])) and torch.equal(mask1[0], mask[i]) and err1.tolist() == [0]
        for strength in STRENGTHS:
            assert np.array_equal(_bits(ops.activity_weights(a1, mask1, strength, CLIP)[0]), _bits(maps[strength][i]))
    # n = 1 against float64 too, and a view that starts off the allocation's alignment (the 128-bit path must not be taken blindly)
    x1, a1_ref, v1_ref, _ = _ref(kind, 1, h, w)
    a1, _, _ = ops.activity_cells(_t(x1, dev))
    assert (np.abs(a1.cpu().numpy().astype(np.float64) - a1_ref) <= AR.tol_a(v1_ref, a1_ref)).all()
    shifted = torch.empty(x1.size + 1, dtype=torch.float32, device=dev)[1:].view(x1.shape)
    shifted.copy_(_t(x1, dev))
    assert shifted.data_ptr() % 16 != 0
    assert np.array_equal(_bits(ops.activity_cells(shifted)[0]), _bits(a1))


def test_non_finite_pixels_mask_their_cell(dev):
    from mcquic_amd import ops
    x, a_ref, v_ref, _ = _ref("gauss", 3, 130, 200)
    clean, _, _ = ops.activity_cells(_t(x, dev))
    x = x.copy()
    top, _, left, _ = AR.pad_split(130, 200)
    x[0, 1, 64, 100] = np.nan                                          # rows 64 and 65 are the only ones the 63 + 63 padding does not mirror:
    x[2, 2, 65, 90] = np.inf                                           # one cell each
    a_ref, v_ref, mask_ref = AR.cells(x)
    assert mask_ref[0].sum() == 1 and mask_ref[2].sum() == 1 and mask_ref[0, (64 + top) // 16, (100 + left) // 16]
    a, mask, err = ops.activity_cells(_t(x, dev))
    assert err.tolist() == [1, 0, 1] and np.array_equal(mask.cpu().numpy().astype(bool), mask_ref)
    keep = ~mask_ref
    assert bool((a[_t(mask_ref, dev)] == 0).all()) and np.array_equal(_bits(a)[keep], _bits(clean)[keep])
    wt = ops.activity_weights(a, mask, 1.0, CLIP).cpu().numpy()
    w_ref, _ = AR.weights(a_ref, mask_ref, 1.0, CLIP)
    assert (wt[mask_ref] == 1.0).all() and np.isfinite(wt).all()
    ta = AR.tol_a(v_ref, a_ref)
    near = AR.near_clip(a_ref, mask_ref, ta, 1.0, CLIP)
    ok = keep & ~near
    assert (np.abs(wt.astype(np.float64) / w_ref - 1.0)[ok] <= AR.tol_w(ta, 1.0)[ok]).all()
    assert np.array_equal(_bits(ops.activity_weights(a, mask, 1.0, CLIP)[1]), _bits(ops.activity_weights(clean, torch.zeros_like(mask), 1.0, CLIP)[1]))
    # a reflected non-finite pixel masks every cell its mirror images fall into: the reference's mask, again
    x[1, 0, 1, 1] = -np.inf
    mask_ref = AR.cells(x)[2]
    assert mask_ref[1].sum() >= 1
    a, mask, err = ops.activity_cells(_t(x, dev))
    assert err.tolist() == [1, 1, 1] and np.array_equal(mask.cpu().numpy().astype(bool), mask_ref)
    # every cell masked: abar = 0, w = 1
    a, mask, err = ops.activity_cells(torch.full((1, 3, 128, 128), float("nan"), device=dev))
    assert int(mask.sum()) == 64 and err.tolist() == [1] and bool((ops.activity_weights(a, mask, 1.0, CLIP) == 1.0).all())


def test_roi_and_lam_products_are_float32_in_the_documented_order(dev):
    from mcquic_amd import ops
    x, _, _, _ = _ref("contrast", 3, 129, 257)
    a, mask, _ = ops.activity_cells(_t(x, dev))
    n, h0, w0 = a.shape
    rng = np.random.default_rng(6)
    w32 = ops.activity_weights(a, mask, 0.5, CLIP).cpu().numpy()
    per_image = rng.uniform(0, 3, size=n).astype(np.float32)
    grid = rng.uniform(0, 3, size=(n, h0, w0)).astype(np.float32)
    lam = rng.uniform(0, 2, size=n).astype(np.float32)
    lam[1] = 0.0
    for roi, r in ((per_image, per_image[:, None, None]), (grid, grid), (None, None)):
        for lm in (None, lam):
            want = w32 if r is None else w32 * r
            want = want if lm is None else want * lm[:, None, None]
            assert want.dtype == np.float32
            got = ops.activity_weights(a, mask, 0.5, CLIP, roi=None if roi is None else _t(roi, dev), lam=None if lm is None else _t(lm, dev))
            assert np.array_equal(_bits(got), want.view(np.int32))
    # a strided view of a larger tensor as roi, and the caller's output buffer
    big = torch.full((n, h0 + 2, 2 * w0 + 3), 9.0, device=dev)
    view = big[:, 1:h0 + 1, 1:2 * w0 + 1:2]
    view.copy_(_t(grid, dev))
    out = torch.empty_like(a)
    assert ops.activity_weights(a, mask, 0.5, CLIP, roi=view, lam=_t(lam, dev), out=out) is out
    assert np.array_equal(_bits(out), ((w32 * grid) * lam[:, None, None]).view(np.int32))
    # a bad roi value keeps the existing rule: it counts as 0 and the map's error word reports it
    bad = grid.copy()
    bad[0, 0, 0], bad[2, 1, 1] = -1.0, np.inf
    got = ops.activity_weights(a, mask, 0.5, CLIP, roi=_t(bad, dev), lam=_t(lam, dev))
    levels, err = ops.rate_map_levels(got, (1.0, 1.0))
    assert err.tolist() == [1, 0, 1] and float(levels[0][0, 0, 0]) == 0.0 and float(levels[0][2, 1, 1]) == 0.0
    assert np.array_equal(_bits(levels[0][1]), _bits(out[1]))
    for kw in (dict(roi=torch.zeros((n, h0), device=dev)), dict(roi=_t(grid, dev).double()), dict(lam=torch.zeros(n + 1, device=dev)),
               dict(roi=torch.zeros(n)), dict(out=torch.empty((n, h0, w0 + 1), device=dev))):
        with pytest.raises(ValueError):
            ops.activity_weights(a, mask, 0.5, CLIP, **kw)
    for strength, clip in ((-1.0, 2.0), (float("nan"), 2.0), (1.0, 0.0), (1.0, float("inf"))):
        with pytest.raises(ValueError):
            ops.activity_weights(a, mask, strength, clip)


def test_padding_that_reflect_cannot_make_is_aligned_paddings_error(dev):
    from mcquic_amd import ops
    from mcquic_amd.modules.compressor import AlignedPadding
    x = torch.zeros((1, 3, 16, 16), device=dev)
    with pytest.raises(RuntimeError, match="Padding size should be less than the corresponding input dimension"):
        AlignedPadding()(x)
    with pytest.raises(RuntimeError, match="Padding size should be less than the corresponding input dimension"):
        ops.activity_cells(x)


def test_both_launches_capture(dev):
    from mcquic_amd import ops
    xs = [_t(_ref(kind, 3, 130, 200)[0], dev) for kind in AR.KINDS]
    lams = [torch.tensor(v, device=dev) for v in ([1.0, 0.5, 2.0], [0.0, 3.0, 0.25], [1.5, 1.0, 0.0])]
    roi = torch.rand((3, 16, 16), device=dev)
    eager = []
    for x, lam in zip(xs, lams):
        a, mask, err = ops.activity_cells(x)
        eager.append((a, mask, err, ops.activity_weights(a, mask, 1.0, CLIP, roi=roi, lam=lam)))
    static_x, static_lam = xs[0].clone(), lams[0].clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        a, mask, _ = ops.activity_cells(static_x)
        ops.activity_weights(a, mask, 1.0, CLIP, roi=roi, lam=static_lam)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        a, mask, err = ops.activity_cells(static_x)
        out = ops.activity_weights(a, mask, 1.0, CLIP, roi=roi, lam=static_lam)
    for x, lam, want in list(zip(xs, lams, eager))[1:] + [(xs[0], lams[0], eager[0])]:
        static_x.copy_(x)
        static_lam.copy_(lam)
        graph.replay()
        assert np.array_equal(_bits(a), _bits(want[0])) and torch.equal(mask, want[1]) and torch.equal(err, want[2])
        assert np.array_equal(_bits(out), _bits(want[3]))
