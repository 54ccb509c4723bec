"""GPU: the MS-SSIM training loss (csrc/msssim_loss.hip through mcquic_amd.ops / autograd.MsSsimFn / loss) against F17
(tests/golden/f17_msssim_loss.npz, the reference's own loss in float32 and float64) and the float64 restatement of
tests/test_msssim_loss_oracle.py.

Bars: the forward within 4x the reference's own float32-vs-float64 difference (at least 1e-6, at most 5e-6 absolute); the
gradients' relative L2 error within 2x the reference's own float32 error (or 1e-4, whichever is larger), the crop's max-abs
error within 4x the reference's.  Determinism is bitwise, eager and replayed.
The elementwise checks (every tile seam, `saved`, guard bands) are in tests/test_gpu_msssim_leaf.py."""
import copy
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle import metrics_ref as M

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("msssim_loss_oracle", os.path.join(HERE, "test_msssim_loss_oracle.py"))
O = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(O)


def _values32(restored, image):
    """v [5, N, C] of the float32 oracle (oracle/metrics_ref.py: the kernels' operation order up to the means)."""
    x, y = restored.float() + 1, image.float() + 1
    win = M.gauss_window()
    vs = []
    for lv in range(5):
        s, cs = M.ssim_and_cs(x, y, win, data_range=2.0)
        vs.append(cs if lv < 4 else s)
        if lv < 4:
            x, y = M._halve(x), M._halve(y)
    return torch.stack(vs).double()


def _check_values(values, restored, image, v64):
    """float32 maps of a few pixels (the coarse levels) carry the cancellation of E[x^2] - mu^2: the values follow the float32
    oracle to 2e-6 and sit within 4x the oracle's own float32 error (+1e-6) of float64."""
    v32 = _values32(restored, image)
    got = values.cpu().double()
    np.testing.assert_allclose(got.numpy(), v32.numpy(), rtol=0, atol=2e-6)
    assert bool(((got - v64).abs() <= 4 * (v32 - v64).abs() + 1e-6).all())


def _rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def _cases():
    z = O.f17()
    return z, list(enumerate(z["cases"].tolist()))


def test_forward_matches_f17_and_restatement(dev):
    from mcquic_amd import ops
    z, cases = _cases()
    for i, (seed, n, h, w) in cases:
        restored, image = O.f17_inputs(seed, n, h, w)
        loss, values, saved = ops.ms_ssim_loss(restored.to(dev), image.to(dev))
        l64, v64 = O.ms_ssim_loss64(restored, image)
        measured = abs(float(z[f"loss32_{i}"][0]) - float(z[f"loss64_{i}"][0]))
        bar = min(max(4 * measured, 1e-6), 5e-6)
        got = float(loss)
        print(f"case {i}: loss {got:.9g} f64 {float(l64):.12g} |err| {abs(got - float(l64)):.2e} (bar {bar:.1e})")
        assert loss.dim() == 0 and values.shape == (5, n, 3)
        assert abs(got - float(z[f"loss64_{i}"][0])) <= bar
        assert abs(got - float(l64)) <= bar
        _check_values(values, restored, image, v64)


def _check_grad(got, g64, rel_bar, crop_bar=None, crop64=None):
    rel = _rel(got, g64)
    assert torch.isfinite(got).all()
    assert rel <= rel_bar, (rel, rel_bar)
    if crop_bar is not None:
        crop = got[0, 0, :O.CROP_ROWS, :O.CROP_COLS].double().cpu().numpy()
        err = float(np.abs(crop - crop64).max())
        assert err <= crop_bar, (err, crop_bar)
    return rel


def test_backward_matches_float64_on_f17(dev):
    from mcquic_amd import ops
    z, cases = _cases()
    for i, (seed, n, h, w) in cases:
        restored, image = O.f17_inputs(seed, n, h, w)
        r, im = restored.to(dev), image.to(dev)
        loss, values, saved = ops.ms_ssim_loss(r, im)
        one = torch.ones((), device=dev)
        da, db = ops.ms_ssim_loss_bwd(r, im, values, saved, one, want_db=True)
        _, _, g64, gi64 = O.grads64(restored, image, wrt_image=True)
        rel32 = float(z[f"rel32_{i}"][0])
        rel_bar = max(2 * rel32, 1e-4)
        crop_meas = float(np.abs(z[f"crop32_{i}"].astype(np.float64) - z[f"crop64_{i}"]).max())
        rel = _check_grad(da, g64, rel_bar, 4 * crop_meas + 1e-12, z[f"crop64_{i}"])
        relb = _check_grad(db, gi64, rel_bar)
        print(f"case {i}: da rel {rel:.2e} db rel {relb:.2e} (reference f32 {rel32:.2e})")
        da_only, none = ops.ms_ssim_loss_bwd(r, im, values, saved, one)
        assert none is None and torch.equal(da_only, da)


def test_backward_training_batch(dev):
    """8 x 3 x 256 x 256: the configs[4] training batch."""
    from mcquic_amd import ops
    z = O.f17()
    restored, image = O.f17_inputs(5, 8, 256, 256)
    r, im = restored.to(dev), image.to(dev)
    loss, values, saved = ops.ms_ssim_loss(r, im)
    da, db = ops.ms_ssim_loss_bwd(r, im, values, saved, torch.ones((), device=dev), want_db=True)
    l64, _, g64, gi64 = O.grads64(restored, image, wrt_image=True)
    assert abs(float(loss) - float(l64)) <= 5e-6
    rel_bar = max(2 * max(float(z[f"rel32_{i}"][0]) for i in range(3)), 1e-4)
    _check_grad(da, g64, rel_bar)
    _check_grad(db, gi64, rel_bar)


def test_autograd_fn_and_dloss_scaling(dev):
    from mcquic_amd import loss as L
    restored, image = O.f17_inputs(1, 2, 176, 208)
    r = restored.to(dev).requires_grad_()
    im = image.to(dev).requires_grad_()
    out = L.MsSSIM()(r, im)
    (3.0 * out).backward()                      # (an ATen mul: the gradient reaching the node is 3)
    _, _, g64, gi64 = O.grads64(restored, image, wrt_image=True)
    assert _rel(r.grad, 3 * g64) <= 1e-4 and _rel(im.grad, 3 * gi64) <= 1e-4
    r2 = restored.to(dev).requires_grad_()
    L.MsSSIM()(r2, image.to(dev)).backward()    # image needs no gradient: db is not computed
    assert _rel(r2.grad, g64) <= 1e-4


def test_relu_zero_path_is_exact(dev):
    """restored = -image: the cs means of some planes go <= 0; their gradients are exactly 0, as float64 autograd gives."""
    from mcquic_amd import ops
    _, image = O.f17_inputs(2, 4, 256, 256)
    restored = -image
    r, im = restored.to(dev), image.to(dev)
    loss, values, saved = ops.ms_ssim_loss(r, im)
    l64, v64, g64, _ = O.grads64(restored, image)
    assert bool((v64 <= 0).any()), "the case must reach the relu's zero side"
    assert torch.isfinite(loss) and abs(float(loss) - float(l64)) <= 5e-6
    da, _ = ops.ms_ssim_loss_bwd(r, im, values, saved, torch.ones((), device=dev))
    da = da.cpu()
    assert torch.isfinite(da).all()
    zero = g64 == 0
    assert bool(zero.any())
    assert bool((da[zero] == 0).all())
    if bool((~zero).any()):
        assert _rel(da[~zero], g64[~zero]) <= 1e-3


def test_identical_images_give_zero_loss(dev):
    from mcquic_amd import ops
    restored, image = O.f17_inputs(1, 2, 176, 208)
    im = image.to(dev)
    loss, values, saved = ops.ms_ssim_loss(im, im.clone())
    assert float(loss) == 0.0 and bool((values == 1).all())
    da, db = ops.ms_ssim_loss_bwd(im, im.clone(), values, saved, torch.ones((), device=dev), want_db=True)
    _, _, g64, _ = O.grads64(restored, image)
    scale = float(g64.abs().max())
    assert torch.isfinite(da).all() and torch.isfinite(db).all()
    assert float(da.abs().max()) <= 1e-3 * scale and float(db.abs().max()) <= 1e-3 * scale


def test_small_side_raises(dev):
    from mcquic_amd import ops
    from mcquic_amd import loss as L
    x = torch.zeros(1, 3, 160, 200, device=dev)
    with pytest.raises(ValueError):
        ops.ms_ssim_loss(x, x)
    with pytest.raises(ValueError):
        L.MsSSIM()(x, x)


@pytest.mark.parametrize("shape", [(2, 1, 175, 389), (1, 4, 322, 163)])
def test_other_channel_counts(dev, shape):
    from mcquic_amd import ops
    n, c, h, w = shape
    x3, _ = O.f17_inputs(h + w, n * ((c + 2) // 3), h, w)
    y3 = x3 + torch.from_numpy(np.random.default_rng(h).normal(0, 0.05, tuple(x3.shape)).astype(np.float32))
    x = x3.reshape(-1, h, w)[: n * c].reshape(n, c, h, w).contiguous()
    y = y3.reshape(-1, h, w)[: n * c].reshape(n, c, h, w).contiguous()
    loss, values, saved = ops.ms_ssim_loss(y.to(dev), x.to(dev))
    l64, v64, g64, gi64 = O.grads64(y, x, wrt_image=True)
    assert abs(float(loss) - float(l64)) <= 5e-6
    _check_values(values, y, x, v64)
    da, db = ops.ms_ssim_loss_bwd(y.to(dev), x.to(dev), values, saved, torch.ones((), device=dev), want_db=True)
    assert _rel(da, g64) <= 1e-4 and _rel(db, gi64) <= 1e-4


def test_deterministic_eager_and_replayed(dev):
    from mcquic_amd import ops
    restored, image = O.f17_inputs(1, 2, 176, 208)
    r, im = restored.to(dev), image.to(dev)
    one = torch.ones((), device=dev)

    def run():
        loss, values, saved = ops.ms_ssim_loss(r, im)
        da, db = ops.ms_ssim_loss_bwd(r, im, values, saved, one, want_db=True)
        return loss, values, da, db

    first = run()
    for _ in range(3):
        again = run()
        assert all(torch.equal(a, b) for a, b in zip(first, again))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                             # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured = run()
    for _ in range(2):
        g.replay()
        float(torch.rand(1000, device=dev).sum().item())  # eager work (fills, a small copy to the host) between replays
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(first, captured))
    g.reset()


def test_launch_census_only_library_kernels(dev):
    from torch.profiler import ProfilerActivity, profile
    from mcquic_amd import autograd as A
    from mcquic_amd import loss as L
    restored, image = O.f17_inputs(1, 2, 176, 208)
    im = image.to(dev)
    fn = L.step_loss()

    def once():
        r = restored.to(dev).requires_grad_()
        out = fn((r,), im)
        A.backward(out)
        return r

    once()
    r = restored.to(dev).requires_grad_()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn((r,), im)
        A.backward(out)
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    print(sorted(set(names)))
    assert any("msl_" in nm for nm in names), names
    bad = [nm for nm in names if "at::" in nm or "native" in nm or "memset" in nm.lower() or "fill" in nm.lower()]
    assert not bad, bad


def _uniforms(n, hw, ks, dev, seed):
    g = torch.Generator().manual_seed(seed)
    us = []
    for lv, k in enumerate(ks):
        s = hw // 16 // (2 ** lv)
        us.append((torch.rand((n, 2, s, s, k), generator=g).to(dev), torch.rand((n, 2, s, s, k), generator=g).to(dev)))
    return us


@pytest.mark.parametrize("segments", [1, 3])
def test_graphed_step_with_ms_ssim_equals_eager(dev, segments):
    from mcquic_amd import Compressor, parallel
    from mcquic_amd import loss as L
    ch, ks, hw = 32, [64, 32, 16], 192
    n, steps, lr = 2, 3, 1e-3
    torch.manual_seed(7)
    eager = Compressor(ch, 2, ks).to(dev).train()
    graphed = copy.deepcopy(eager)
    mse_model = copy.deepcopy(eager)
    xs = [(torch.rand((n, 3, hw, hw), generator=torch.Generator().manual_seed(20 + i)) * 2 - 1).to(dev) for i in range(steps)]
    us = _uniforms(n, hw, ks, dev, 5)
    loss_fn = L.step_loss()

    opt_e = torch.optim.SGD(eager.parameters(), lr=lr)
    losses_e = []
    for x in xs:
        opt_e.zero_grad(set_to_none=True)
        loss = loss_fn(eager(x, uniforms=us), x)
        loss.backward()
        opt_e.step()
        losses_e.append(float(loss.detach()))

    opt_g = torch.optim.SGD(graphed.parameters(), lr=lr)
    step = parallel.GraphedTrainStep(graphed, opt_g, xs[0], loss_fn=loss_fn, forward_kwargs={"uniforms": us}, segments=segments)
    losses_g = [float(step(x)) for x in xs]
    step.close()
    opt_m = torch.optim.SGD(mse_model.parameters(), lr=lr)
    step_m = parallel.GraphedTrainStep(mse_model, opt_m, xs[0], forward_kwargs={"uniforms": us}, segments=segments)
    for x in xs:
        step_m(x)
    step_m.close()
    torch.cuda.synchronize()

    for a, b in zip(losses_e, losses_g):
        assert abs(a - b) <= 1e-6 * max(1.0, abs(a)), (losses_e, losses_g)
    differs = 0
    for (name, pe), (_, pg), (_, pm) in zip(eager.named_parameters(), graphed.named_parameters(), mse_model.named_parameters()):
        scale = max(float(pe.detach().abs().max()), 1e-12)
        assert float((pe.detach() - pg.detach()).abs().max()) <= 2e-6 * scale, name
        if float((pm.detach() - pg.detach()).abs().max()) > 1e-5 * scale:
            differs += 1
    assert differs > 0, "the MS-SSIM term did not reach the gradient"


def test_u8_metric_unchanged(dev):
    from mcquic_amd import ops
    z = np.load(os.path.join(HERE, "golden", "f7_metrics.npz"))
    for i, (seed, n, h, w) in enumerate(z["cases"].tolist()):
        x, y = M.make_u8_pair(seed, n, h, w)
        got = ops.ms_ssim(x.to(dev), y.to(dev)).cpu()
        np.testing.assert_allclose(got.numpy(), M.ms_ssim(x, y).numpy(), rtol=0, atol=2e-6)
        np.testing.assert_allclose(got.numpy(), z[f"msssim_{i}"], rtol=0, atol=5e-6)
