"""The adaptive-quantisation map without a device: the float64 restatement of tests/_activity_ref.py against its own definition (exact
values on constant images, geometric mean 1, `AlignedPadding`'s split, the masked-cell rules), the condition the GPU test's excuse rests
on (on its seeds the reference alone leaves at most 1 % of a case's cells within rounding of a clip boundary), and what the C entry
points, `ops` and `Compressor` refuse before any launch."""
import numpy as np
import pytest
import torch

import _activity_ref as AR


def test_a_constant_image_is_exact():
    for (h, w) in AR.GEOMS:
        x = np.empty((2, 3, h, w), dtype=np.float32)
        x[0, 0], x[0, 1], x[0, 2] = 0.3, -0.7, 0.11
        x[1] = -1.0
        a, v, mask = AR.cells(x)
        assert a.shape == (2, -(-h // 128) * 8, -(-w // 128) * 8) and not mask.any()
        assert (a == -14.0).all()
        for strength in (0.0, 0.5, 3.0):
            w_, out = AR.weights(a, mask, strength, 2.0)
            assert (w_ == 1.0).all() and (out == 1.0).all()


def test_the_geometric_mean_is_one_while_nothing_clips():
    x = AR.make_image("contrast", 3, 130, 200, seed=1)
    a, v, mask = AR.cells(x)
    assert a.max() - a.min() > 8                                      # (the activities do vary)
    w_, _ = AR.weights(a, mask, 0.1, 2.0)
    assert np.abs(AR.exponents(a, mask, 0.1)).max() < 2.0
    assert np.abs(np.log2(w_).mean(axis=(1, 2))).max() < 1e-12
    clipped, _ = AR.weights(a, mask, 1.0, 2.0)
    assert clipped.min() == 0.25 and clipped.max() == 4.0             # strength 1 over 9 octaves does clip, at exactly 2^-2 and 2^2


def test_the_padding_split_is_aligned_paddings():
    from mcquic_amd.modules.compressor import AlignedPadding
    for (h, w) in AR.GEOMS + ((100, 300),):
        ramp = (np.arange(h, dtype=np.float32)[:, None] * 1000 + np.arange(w, dtype=np.float32)[None, :])
        x = np.stack([ramp, ramp + 0.25, ramp + 0.5])[None]
        want = AlignedPadding()(torch.from_numpy(x)).numpy()
        assert np.array_equal(AR.padded(x), want)
        top, bottom, left, right = AR.pad_split(h, w)
        assert want.shape[-2:] == (h + top + bottom, w + left + right) and top <= bottom <= top + 1 and left <= right <= left + 1
    assert AR.pad_split(129, 257) == (63, 64, 63, 64)
    small = np.zeros((1, 3, 16, 16), dtype=np.float32)
    with pytest.raises(RuntimeError, match="Padding size should be less than the corresponding input dimension"):
        AlignedPadding()(torch.from_numpy(small))
    with pytest.raises(RuntimeError, match="Padding size should be less than the corresponding input dimension"):
        AR.padded(small)


def test_masked_cells():
    x = AR.make_image("gauss", 2, 128, 128, seed=2)
    clean = AR.cells(x)
    x[0, 1, 17, 33] = np.nan                                           # cell (1, 2) of image 0
    x[1, 2, 127, 0] = np.inf                                           # cell (7, 0) of image 1
    a, v, mask = AR.cells(x)
    assert mask.sum() == 2 and mask[0, 1, 2] and mask[1, 7, 0] and a[0, 1, 2] == 0 and a[1, 7, 0] == 0
    assert np.array_equal(a[~mask], clean[0][~mask])
    w_, out = AR.weights(a, mask, 1.0, 2.0, roi=np.asarray([2.0, 0.5]), lam=np.asarray([1.0, 3.0]))
    assert w_[0, 1, 2] == 1.0 and w_[1, 7, 0] == 1.0 and out[0, 1, 2] == 2.0 and out[1, 7, 0] == 1.5
    # the mean runs over the unmasked cells alone: the other cells' weights are those of the image with that cell left out
    keep = ~mask[0]
    assert np.allclose(np.log2(w_[0][keep]).mean(), 0.0, atol=1e-12)
    # every cell masked: abar = 0 and w = 1 everywhere; a bad roi value is NaN
    all_a, all_mask = np.zeros((1, 2, 2)), np.ones((1, 2, 2), dtype=bool)
    assert (AR.weights(all_a, all_mask, 1.0, 2.0)[0] == 1.0).all()
    _, out = AR.weights(a, mask, 1.0, 2.0, roi=np.asarray([-1.0, np.inf]))
    assert np.isnan(out).all()


@pytest.mark.parametrize("kind", AR.KINDS)
def test_the_reference_alone_stays_inside_the_excuse_cap(kind):
    """The GPU test may excuse a cell within rounding of a clip boundary; that is a condition on its cases, checked here for every one."""
    for (h, w) in AR.GEOMS:
        for n in (1, 3):
            a, v, mask = AR.cells(AR.make_image(kind, n, h, w, seed=0))
            ta = AR.tol_a(v, a)
            for strength in (0.5, 1.0):
                near = AR.near_clip(a, mask, ta, strength, 2.0)
                assert near.sum() <= AR.EXCUSED_CAP * near.size, (kind, h, w, n, strength, int(near.sum()))


def test_entry_points_refuse_bad_arguments_without_a_device():
    from ctypes import c_float, c_int32, c_int64, c_void_p
    from mcquic_amd import _lib
    lib, E, P = _lib.load(), _lib.MCQ_EINVAL, 0x1000                 # P is never dereferenced: every call below is refused first
    f = lib.mcq_activity_cells_f32
    ok = [P, 2, 130, 200, 128, P, P, P, None]
    for i in (0, 5, 6, 7):
        assert f(*[None if j == i else a for j, a in enumerate(ok)]) == E
    for i, v in ((1, 0), (2, 0), (3, -1), (4, 0), (4, 24), (2, 16), (3, 32), (2, 1)):     # (16, 32, 1: padding reflect cannot make)
        assert f(*[v if j == i else a for j, a in enumerate(ok)]) == E
    f = lib.mcq_activity_weights_f32
    ok = [P, P, 2, 8, 8, 1.0, 2.0, P, 64, 8, 1, P, P, None]
    for i in (0, 1, 12):
        assert f(*[None if j == i else a for j, a in enumerate(ok)]) == E
    for i, v in ((2, 0), (3, 0), (4, -1), (5, -0.5), (5, float("nan")), (5, float("inf")), (6, 0.0), (6, -1.0), (6, float("nan")),
                 (6, float("inf")), (8, -1), (9, -1), (10, -1)):
        assert f(*[v if j == i else a for j, a in enumerate(ok)]) == E
    V, I, L, F = c_void_p, c_int32, c_int64, c_float
    assert _lib.SYMBOLS["mcq_activity_cells_f32"] == (I, [V, I, I, I, I, V, V, V, V])
    assert _lib.SYMBOLS["mcq_activity_weights_f32"] == (I, [V, V, I, I, I, F, F, V, L, L, L, V, V, V])
    assert _lib.MCQ_ABI_VERSION == 18


def test_ops_and_the_model_refuse_before_any_launch():
    from mcquic_amd import Compressor, Neon, ops
    assert ops.activity_grid(128, 128) == (8, 8) and ops.activity_grid(130, 200) == (16, 16) and ops.activity_grid(129, 257) == (16, 24)
    with pytest.raises(RuntimeError, match="Padding size should be less than the corresponding input dimension"):
        ops.activity_grid(16, 16)
    with pytest.raises(ValueError):
        ops.activity_grid(128, 128, base=24)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.activity_cells(torch.zeros((1, 3, 128, 128)))
    with pytest.raises(ValueError):
        ops.activity_cells(torch.zeros((1, 1, 128, 128)))
    with pytest.raises(ValueError):
        ops.activity_weights(torch.zeros((1, 8, 8)), torch.zeros((1, 8, 8), dtype=torch.int32), 1.0, 2.0)
    model = Compressor(8, 2, [32, 16, 8]).eval()
    x = torch.zeros((2, 3, 128, 128))
    assert model._aqArgs(None) is None and model._aqArgs(0.5) == (0.5, 2.0) and model._aqArgs((1, 3)) == (1.0, 3.0)
    assert model._aqArgs(0.1) == (float(np.float32(0.1)), 2.0)
    for bad in (-0.5, float("nan"), float("inf"), (1.0, 0.0), (1.0, -2.0), (1.0, float("nan")), (1.0,), (1.0, 2.0, 3.0), "x", True,
                torch.ones(2)):
        for call in (lambda: model.encode(x, aq=bad), lambda: model.compress(x, aq=bad), lambda: model.activityWeights(x, bad),
                     lambda: model.encode_to_rate(x, 0.1, aq=bad), lambda: model.encode_to_rate(x, 0.1, per_image=True, aq=bad)):
            with pytest.raises(ValueError, match="aq"):
                call()
    with pytest.raises(ValueError, match="aq"):
        model.encode(x[:0], aq=0.5)
    with pytest.raises(RuntimeError, match="Padding size"):
        model.encode(torch.zeros((1, 3, 16, 16)), aq=0.5)
    with pytest.raises(RuntimeError, match="no call with `aq`"):
        model.activityError()
    neon = Neon(32, 256, [8, 4, 2, 2]).eval()
    for call in (lambda: neon.encode(x, aq=0.5), lambda: neon.compress(x, aq=0.5), lambda: neon.activityWeights(x, 0.5),
                 lambda: neon.encode_to_rate(x, 0.1, aq=0.5)):
        with pytest.raises(NotImplementedError):
            call()


def test_the_cli_takes_the_rate_knobs():
    from mcquic_amd import demo
    a = demo.parser().parse_args(["--rd-lambda", "0.1", "--aq", "0.5", "--aq-clip", "3", "in.png"])
    assert a.rd_lambda == 0.1 and a.aq == 0.5 and a.aq_clip == 3.0 and a.target_bpp is None
    assert demo.rateOptions(a) == dict(rd_lambda=0.1, target_bpp=None, aq=(0.5, 3.0))
    a = demo.parser().parse_args(["--target-bpp", "0.4", "in.png"])
    assert demo.rateOptions(a) == dict(rd_lambda=None, target_bpp=0.4, aq=None)
    for bad in (["--rd-lambda", "0.1", "--target-bpp", "0.4", "in.png"], ["--aq-clip", "3", "in.png"]):
        with pytest.raises(ValueError):
            demo.rateOptions(demo.parser().parse_args(bad))
