"""The training input transform's two HIP launches (csrc/augment.hip; ops.augment_draw / ops.augment, utils.vision,
data.transforms) against the float64 statement of the pipeline in tests/_augment_ref.py (whose resampler
tests/test_augment_ref.py pins to ATen), bit-exact where the pipeline is switched off, and the draw's distributions.

Every pass below runs under an explicit table.  Bars: the pass is float32 with powf; BARS[mode] is 4x the largest absolute
error measured on an MI355X over every case of this file for that gamma mode (the factor of the gradient bars, DESIGN.md
section 6; docs/experiments.md has the figures), and none may exceed 1e-5."""
import numpy as np
import pytest
import torch

import _augment_ref as R
from _record import record

pytestmark = pytest.mark.gpu

HS, WS, N = 61, 83, 3
#        measured max |error| on the MI355X per gamma mode (uint8 and float32 input, every case below), times 4
MEASURED = {R.SRGB_TO_LINEAR: 3.61e-7, R.LINEAR_TO_SRGB: 6.34e-7, R.POWER: 3.57e-7, R.IDENTITY: 4.06e-7}
BARS = {m: 4.0 * v for m, v in MEASURED.items()}


def _sources():
    g = torch.Generator().manual_seed(11)
    u8 = torch.randint(0, 256, (N, 3, HS, WS), generator=g, dtype=torch.uint8)
    f32 = torch.rand((N, 3, HS, WS), generator=g, dtype=torch.float32)
    return {"uint8": u8, "float32": f32}


SOURCES = _sources()


def _table(rows):
    p = R.identity_params(len(rows), (HS, WS))
    for n, row in enumerate(rows):
        for k, v in row.items():
            p[n, k] = v
    return p


def _box(top, left, h, w, **more):
    d = {R.TOP: top, R.LEFT: left, R.BOX_H: h, R.BOX_W: w}
    d.update({getattr(R, k): v for k, v in more.items()})
    return d


CASES = {
    "whole": ((32, 48), [_box(0, 0, HS, WS)] * 3),
    "borders": ((32, 48), [_box(0, 0, 40, 50), _box(HS - 37, WS - 45, 37, 45), _box(HS - 50, 0, 50, 60)]),
    "borders2": ((32, 48), [_box(0, WS - 70, 45, 70), _box(5, 0, 56, WS), _box(0, 7, HS, 64)]),
    "thin": ((32, 48), [_box(30, 5, 1, 70), _box(3, WS - 1, 50, 1), _box(HS - 1, 0, 1, 1)]),
    "up": ((32, 48), [_box(0, 0, 20, 30), _box(HS - 31, WS - 47, 31, 47), _box(17, 29, 9, 13)]),
    "mixed": ((22, 88), [_box(0, 3, 60, 70), _box(1, 0, 60, 83), _box(0, 40, 61, 20)]),           # 60 / 22 = 2.73 down, 70 / 88 up
    "mixed2": ((40, 28), [_box(0, 0, 30, 76), _box(20, 7, 39, 76), _box(0, 0, 61, 83)]),          # 76 / 28 = 2.71 down, 30 / 40 up
    "gamma": ((32, 48), [_box(2, 3, 50, 70, GAMMA_MODE=R.SRGB_TO_LINEAR), _box(2, 3, 50, 70, GAMMA_MODE=R.LINEAR_TO_SRGB),
                         _box(2, 3, 50, 70, GAMMA_MODE=R.POWER, GAMMA=0.05)]),
    "gamma2": ((32, 48), [_box(0, 0, HS, WS, GAMMA_MODE=R.POWER, GAMMA=2.0), _box(4, 4, 20, 30, GAMMA_MODE=R.IDENTITY),
                          _box(0, 0, HS, WS, GAMMA_MODE=R.POWER, GAMMA=0.731)]),
    "gain": ((32, 48), [_box(0, 0, HS, WS, GAIN0=0.8, GAIN2=1.2, GAIN_ROW=4), _box(3, 3, 40, 60, GAIN0=3.0, GAIN2=2.5, GAIN_ROW=0),
                        _box(3, 3, 40, 60, GAMMA_MODE=R.SRGB_TO_LINEAR, GAIN0=1.7, GAIN2=0.4, GAIN_ROW=1)]),
    "flips": ((32, 48), [_box(1, 2, 55, 77, HFLIP=1), _box(1, 2, 55, 77, VFLIP=1), _box(1, 2, 55, 77, HFLIP=1, VFLIP=1)]),
    "flips_gamma": ((32, 50), [_box(0, 0, HS, WS, HFLIP=1, GAMMA_MODE=R.LINEAR_TO_SRGB, GAIN0=1.3, GAIN2=0.9),
                               _box(9, 9, 30, 30, VFLIP=1, GAMMA_MODE=R.POWER, GAMMA=0.05), _box(0, 0, 60, 80, HFLIP=1, VFLIP=1)]),
    "tail": ((32, 50), [_box(0, 0, HS, WS), _box(2, 1, 57, 80), _box(0, 0, 20, 30, HFLIP=1)]),     # W % 4 != 0: the scalar-store path
    "tiles": ((130, 70), [_box(0, 0, HS, WS), _box(3, 5, 50, 70, HFLIP=1, VFLIP=1, GAMMA_MODE=R.POWER, GAMMA=2.0),
                          _box(0, 0, 30, 40, GAMMA_MODE=R.SRGB_TO_LINEAR)]),                       # two column tiles, nine row tiles
    "tiles_vec": ((20, 260), [_box(0, 0, HS, WS, HFLIP=1), _box(3, 5, 50, 70), _box(0, 0, 30, 40, VFLIP=1)]),   # two tiles of the 128-bit path
    "raw": ((32, 48), [_box(0, 0, HS, WS, OUTPUT=R.OUT_RAW, GAIN0=1.5), _box(0, 0, 40, 60, OUTPUT=R.OUT_CLAMPED, GAIN0=1.5),
                       _box(0, 0, 40, 60, OUTPUT=R.OUT_RAW, GAMMA_MODE=R.SRGB_TO_LINEAR)]),
}

_REFS = {}


def _reference(name, dtype):
    """float64 reference of a case, computed once and shared."""
    key = (name, dtype)
    if key not in _REFS:
        size, rows = CASES[name]
        ref = R.pipeline(SOURCES[dtype].numpy(), size, _table(rows))
        ref.setflags(write=False)
        _REFS[key] = ref
    return _REFS[key]


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
@pytest.mark.parametrize("name", list(CASES))
def test_pass_matches_the_float64_reference(dev, name, dtype):
    from mcquic_amd import ops
    size, rows = CASES[name]
    params = _table(rows)
    got = ops.augment(SOURCES[dtype].to(dev), size, torch.from_numpy(params).to(dev)).cpu().numpy().astype(np.float64)
    want = _reference(name, dtype)
    assert got.shape == want.shape == (N, 3) + tuple(size)
    errs = {}
    for n in range(N):
        mode = int(params[n, R.GAMMA_MODE])
        errs[mode] = max(errs.get(mode, 0.0), float(np.abs(got[n] - want[n]).max()))
    for mode, err in errs.items():
        print(f"augment {name} {dtype} gamma mode {mode}: max |error| {err:.3e}")
        record(f"augment/{name}/{dtype}/mode{mode}", value=err, bar=BARS[mode])
    for mode, err in errs.items():
        assert BARS[mode] <= 1e-5                             # (a larger bar would be a defect, not a tolerance)
        assert err <= BARS[mode], f"{name} {dtype} gamma mode {mode}: max |error| {err:.3e} > {BARS[mode]:.3e}"


# ---- exact cases -------------------------------------------------------------------------------------------------------
def _off_cpu(x: torch.Tensor) -> torch.Tensor:
    """What the reference's transform computes today, in float32 on the CPU."""
    v = x.float() / 255 if x.dtype == torch.uint8 else x
    return (v.clamp(0, 1) - 0.5) / 0.5


@pytest.mark.parametrize("dtype", ["uint8", "float32"])
@pytest.mark.parametrize("flips", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_switched_off_is_clamp_and_normalise_bit_for_bit(dev, dtype, flips):
    from mcquic_amd import ops
    x = SOURCES[dtype] if dtype == "uint8" else SOURCES[dtype] * 1.5 - 0.25           # (float: some values outside [0, 1])
    params = ops.augment_identity_params(N, (HS, WS))
    params[:, ops.AUG_HFLIP], params[:, ops.AUG_VFLIP] = flips
    got = ops.augment(x.to(dev), (HS, WS), params.to(dev)).cpu()
    want = _off_cpu(x)
    if flips[0]:
        want = want.flip(-1)
    if flips[1]:
        want = want.flip(-2)
    assert torch.equal(got, want)


def test_reference_transform_as_it_runs_today(dev):
    """getTrainingTransform(gen=True, planckian=None): no gain, no flips -- clamp and normalise, exactly."""
    from mcquic_amd.data.transforms import getTrainingTransform
    g = torch.Generator().manual_seed(3)
    x = torch.rand((4, 3, 40, 52), generator=g) * 1.6 - 0.3
    t = getTrainingTransform(gen=True, planckian=None, seed=1)
    assert torch.equal(t(x.to(dev)).cpu(), _off_cpu(x))
    assert t.last_params is not None and tuple(t.last_params.shape) == (4, 16)


def test_fused_equals_the_two_halves(dev):
    """TrainingInput under a table equals transform(preprocess(x)) under the same decisions, bit for bit; the single-stage modules
    leave the other stages alone."""
    from mcquic_amd import ops
    from mcquic_amd.data.transforms import TrainingInput, getEvalTransform, getTrainingPreprocess, getTrainingTransform
    from mcquic_amd.utils import vision
    coeffs = torch.rand((7, 2), generator=torch.Generator().manual_seed(5)) + 0.5
    x = SOURCES["uint8"].to(dev)
    pre, post = getTrainingPreprocess((32, 48), seed=2), getTrainingTransform(planckian=coeffs, seed=3)
    fused = TrainingInput.from_halves(pre, post, seed=4)
    out = fused(x)
    table = fused.last_params.clone()
    first = table.clone()
    first[:, [ops.AUG_GAIN0, ops.AUG_GAIN2]] = 1.0
    first[:, [ops.AUG_HFLIP, ops.AUG_VFLIP]] = 0.0
    first[:, ops.AUG_OUTPUT] = ops.AUG_OUT_RAW
    second = ops.augment_identity_params(N, (32, 48), dev)
    for c in (ops.AUG_GAIN0, ops.AUG_GAIN2, ops.AUG_HFLIP, ops.AUG_VFLIP):
        second[:, c] = table[:, c]
    assert torch.equal(post(pre(x, params=first), params=second), out)
    rows = table[:, ops.AUG_GAIN_ROW].cpu()
    assert bool(((rows >= 0) & (rows < 7)).all())                                  # p = 1.0: every image drew a row
    assert torch.equal(table[:, ops.AUG_GAIN0].cpu(), coeffs[rows.long(), 0])
    # single stages
    xf = SOURCES["float32"].to(dev)
    flip = vision.RandomHorizontalFlip(p=1.0, seed=1)
    assert torch.equal(flip(xf), xf.flip(-1))
    assert torch.equal(vision.RandomVerticalFlip(p=1.0, seed=1)(xf), xf.flip(-2))
    jit = vision.RandomPlanckianJitter(coeffs, p=0.0, seed=1)
    assert torch.equal(jit(xf * 1.5 - 0.25), (xf * 1.5 - 0.25).clamp(0, 1))
    crop = vision.RandomResizedCrop((32, 48), (0.75, 1.0), (0.95, 1.05), seed=1)
    assert tuple(crop(x).shape) == (N, 3, 32, 48)
    gam = vision.RandomGamma(seed=1)
    assert tuple(gam(xf).shape) == tuple(xf.shape)
    # evaluation: AlignedCrop(256) + Normalize in one launch
    big = torch.randint(0, 256, (1, 3, 300, 530), generator=torch.Generator().manual_seed(6), dtype=torch.uint8)
    ev = getEvalTransform()
    assert torch.equal(ev(big.to(dev)).cpu(), _off_cpu(ev.crop(big)))
    # the generator state is the module's: restoring it repeats the decisions
    state = {k: v.clone() for k, v in fused.state_dict().items()}
    a = fused(x)
    ta = fused.last_params.clone()
    fused.load_state_dict(state)
    b = fused(x)
    assert torch.equal(ta, fused.last_params) and torch.equal(a, b)


# ---- the draw ----------------------------------------------------------------------------------------------------------
def _rng(dev, seed=1234, offset=0):
    return torch.tensor([seed, offset], dtype=torch.int64, device=dev)


def test_draw_distributions(dev):
    from mcquic_amd import ops
    n, hs, ws, T = 4096, 512, 512, 37
    coeffs = (torch.rand((T, 2), generator=torch.Generator().manual_seed(9)) + 0.5).to(dev)
    rng = _rng(dev)
    t = ops.augment_draw(rng, n, (hs, ws), crop=((0.75, 1.0), (0.95, 1.05)), gamma=True, coeffs=coeffs, p_gain=0.5, p_hflip=0.5,
                         p_vflip=0.5).cpu().double()
    assert tuple(t.shape) == (n, 16)
    top, left, h, w = (t[:, c] for c in (ops.AUG_TOP, ops.AUG_LEFT, ops.AUG_H, ops.AUG_W))
    assert bool(((top >= 0) & (left >= 0) & (h >= 1) & (w >= 1) & (top + h <= hs) & (left + w <= ws)).all())
    assert bool((t[:, :4] == t[:, :4].round()).all())
    assert float(t[:, ops.AUG_FALLBACK].sum()) == 0
    # w and h are each rounded to the nearest integer: (w +- 0.5)(h +- 0.5) bounds the area, (w +- 0.5) / (h -+ 0.5) the aspect
    assert bool(((w + 0.5) * (h + 0.5) >= 0.75 * hs * ws).all()) and bool(((w - 0.5) * (h - 0.5) <= 1.0 * hs * ws).all())
    assert bool(((w + 0.5) / (h - 0.5) >= 0.95).all()) and bool(((w - 0.5) / (h + 0.5) <= 1.05).all())
    assert float((w * h).min()) < 0.80 * hs * ws and float((w * h).max()) > 0.95 * hs * ws        # (the range is used)
    assert float(top.max()) > 0 and float(left.max()) > 0
    modes = t[:, ops.AUG_GAMMA_MODE]
    for m in range(4):
        share = float((modes == m).double().mean())
        assert 0.20 <= share <= 0.30, (m, share)
    assert bool(((modes >= 0) & (modes <= 3)).all())
    g = t[:, ops.AUG_GAMMA][modes == ops.AUG_GAMMA_POWER]
    assert float(g.min()) >= 0.05 - 1e-7 and float(g.max()) <= 2.0 and float(g.max() - g.min()) > 1.5
    for c in (ops.AUG_HFLIP, ops.AUG_VFLIP):
        assert bool(((t[:, c] == 0) | (t[:, c] == 1)).all())
        assert 0.45 <= float(t[:, c].mean()) <= 0.55
    rows = t[:, ops.AUG_GAIN_ROW]
    drawn = rows >= 0
    assert 0.45 <= float(drawn.double().mean()) <= 0.55                            # p_gain = 0.5
    assert bool((rows[drawn] < T).all()) and bool((rows[~drawn] == -1).all()) and len(set(rows[drawn].tolist())) == T
    cc = coeffs.cpu().double()
    assert torch.equal(t[drawn][:, ops.AUG_GAIN0], cc[rows[drawn].long(), 0]) and torch.equal(t[drawn][:, ops.AUG_GAIN2], cc[rows[drawn].long(), 1])
    assert bool((t[~drawn][:, [ops.AUG_GAIN0, ops.AUG_GAIN2]] == 1).all())
    # p = 1.0: every row index lies in [0, T)
    t1 = ops.augment_draw(rng, n, (hs, ws), coeffs=coeffs, p_gain=1.0).cpu()
    assert bool(((t1[:, ops.AUG_GAIN_ROW] >= 0) & (t1[:, ops.AUG_GAIN_ROW] < T)).all())
    assert bool((t1[:, ops.AUG_H] == hs).all()) and bool((t1[:, ops.AUG_GAMMA_MODE] == ops.AUG_GAMMA_IDENTITY).all())


def test_draw_falls_back_to_the_central_crop(dev):
    from mcquic_amd import ops
    t = ops.augment_draw(_rng(dev), 4096, (100, 700), crop=((0.75, 1.0), (0.95, 1.05))).cpu()
    assert bool((t[:, ops.AUG_FALLBACK] == 1).all())
    assert bool((t[:, ops.AUG_H] == 100).all()) and bool((t[:, ops.AUG_W] == 105).all())          # aspect clamped to 1.05
    assert bool((t[:, ops.AUG_TOP] == 0).all()) and bool((t[:, ops.AUG_LEFT] == (700 - 105) // 2).all())


def test_draw_is_a_function_of_seed_and_offset(dev):
    from mcquic_amd import ops
    kw = dict(crop=((0.75, 1.0), (0.95, 1.05)), gamma=True, p_hflip=0.5, p_vflip=0.5)
    a, b = _rng(dev), _rng(dev)
    ta, tb = ops.augment_draw(a, 64, (96, 80), **kw), ops.augment_draw(b, 64, (96, 80), **kw)
    assert torch.equal(ta, tb)
    assert a.cpu().tolist()[0] == 1234 and a.cpu().tolist()[1] > 0                 # the launch moved the offset itself
    ta2 = ops.augment_draw(a, 64, (96, 80), **kw)
    assert not torch.equal(ta, ta2)
    assert torch.equal(ta2, ops.augment_draw(b, 64, (96, 80), **kw))
    assert not torch.equal(ta, ops.augment_draw(_rng(dev, seed=1235), 64, (96, 80), **kw))


# ---- errors --------------------------------------------------------------------------------------------------------------
def test_errors(dev):
    from mcquic_amd import ops
    from mcquic_amd.data.transforms import TrainingInput
    good = SOURCES["float32"].to(dev)
    params = ops.augment_identity_params(N, (HS, WS), dev)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.augment(SOURCES["float32"], (32, 48), params)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        TrainingInput((32, 48))(SOURCES["uint8"])
    with pytest.raises(TypeError, match="uint8 or float32"):
        ops.augment(good.double(), (32, 48), params)
    with pytest.raises(ValueError, match="contiguous"):
        ops.augment(good.transpose(2, 3), (32, 48), params)
    with pytest.raises(ValueError, match=r"\[N, 3, Hs, Ws\]"):
        ops.augment(good[:, :1].contiguous(), (32, 48), params)
    with pytest.raises(ValueError, match="table"):
        ops.augment(good, (32, 48), params[:, :12].contiguous())
    with pytest.raises(ValueError, match="table"):
        ops.augment(good, (32, 48), params[:2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.augment(good, (32, 48), params.cpu())
    with pytest.raises(ValueError, match=r"\[T, 2\]"):
        ops.augment_draw(_rng(dev), 4, (HS, WS), coeffs=torch.ones(5, 3, device=dev), p_gain=1.0)
    with pytest.raises(TypeError, match="rng"):
        ops.augment_draw(torch.zeros(2, dtype=torch.int64), 4, (HS, WS))
