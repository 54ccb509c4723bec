"""mcquic_amd.monitor.StepMeter through parallel.GraphedTrainStep(..., meter=...), on the model and shards of tests/test_gpu_ema_step.py:
Compressor(32, 2, [64, 32, 16]), two 64 x 64 images, fixed uniforms, mcquic_amd.optim.SGD, the step's own clipping.  The meter only reads:
the step with it is the step without it, bit for bit, and its rows hold what the step exposes."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
CH, KS, HW, N, LR, STEPS = 32, [64, 32, 16], 64, 2, 1e-2, 5


def _run(dev, with_meter, capture_post):
    from mcquic_amd import monitor, optim, parallel
    from test_gpu_ema_step import _setup
    model, xs, us = _setup(dev)
    meter = monitor.StepMeter(model, capacity=8, pixels=N * HW * HW) if with_meter else None
    extra = {"meter": meter} if with_meter else {}
    step = parallel.GraphedTrainStep(model, optim.SGD(model.parameters(), lr=LR, momentum=0.9), xs[0], forward_kwargs={"uniforms": us},
                                     max_grad_norm=4.0, capture_post=capture_post, **extra)
    assert (step.post is not None) == capture_post
    built = meter._buf.clone() if with_meter else None
    losses, norms = [], []
    for it in range(STEPS):
        losses.append(step(xs[it % 2]).clone())
        norms.append(step.grad_norm.clone())
    rows = meter.read() if with_meter else None
    step.invalidate()
    usage = float(model.CodeUsage)
    params = [p.detach().clone() for p in model.parameters()]
    step.close()
    return dict(losses=torch.stack(losses).cpu().numpy(), norms=torch.stack(norms).cpu().numpy(), rows=rows, usage=usage, params=params,
                built=built, meter=meter)


@pytest.fixture(scope="module")
def runs(dev):
    return {"meter": _run(dev, True, True), "plain": _run(dev, False, True), "eager": _run(dev, True, False)}


def test_the_step_with_a_meter_is_the_step_without(runs):
    a, b = runs["meter"], runs["plain"]
    assert a["losses"].tobytes() == b["losses"].tobytes() and a["norms"].tobytes() == b["norms"].tobytes()
    assert all(torch.equal(x, y) for x, y in zip(a["params"], b["params"]))


def test_constructor_leaves_the_meter_as_it_was(runs):
    built = runs["meter"]["built"].cpu().numpy()
    assert built[0] == 0 and built[1] == -1 and np.isnan(built[2:3].view(np.float32)[0]) and not built[3:].any()
    assert runs["meter"]["rows"]["steps"].tolist() == list(range(STEPS))


def test_rows_hold_what_the_step_exposes(runs):
    import _meter_ref as M
    a = runs["meter"]
    r = a["rows"]
    assert r["loss"].tobytes() == a["losses"].tobytes(), "the loss column is not step.loss"
    assert r["grad_norm"].tobytes() == a["norms"].tobytes(), "the grad_norm column is not step.grad_norm"
    assert (r["lr"] == np.float32(LR)).all() and (r["skipped"] == 0).all() and r["first_bad_step"] == -1 and r["dropped"] == 0
    assert np.float32(r["code_usage"][-1]) == np.float32(a["usage"]), "code_usage is not Compressor.CodeUsage after the same steps"
    shadow = np.float32("nan")
    for db, ema in zip(r["db"], r["db_ema"]):
        shadow = M.ema_f32(shadow, db)
        assert ema.tobytes() == shadow.tobytes()
    # every code of the batch is counted once per group: N images, hw / 16 / 2^l squared positions
    for l in range(len(KS)):
        positions = N * (HW // 16 // 2 ** l) ** 2
        assert 0 < r["hit"][-1, l] <= min(1.0, positions / KS[l]) and 0 <= r["step_entropy"][-1, l] <= np.log2(min(positions, KS[l])) + 1e-6
    assert (r["bpp"] > 0).all() and (r["ema_entropy"] > 0).all() and (r["usage"] <= 1).all()


def _opt_norm(opt):
    norm = opt.grad_norm                                      # (optim.SGD: a method; optim.Lamb: a property)
    return norm() if callable(norm) else norm


@pytest.mark.parametrize("kind", ["sgd-clips", "sgd-guards-only", "lamb"])
def test_the_optimizers_own_norm_and_skip_count_are_recorded(dev, kind):
    """Without the step's `max_grad_norm` the `grad_norm` column is the optimizer's own norm wherever it computes one -- optim.SGD with
    `max_grad_norm` or with `skip_nonfinite` alone, optim.Lamb always -- and `skipped` is the optimizer's counter, read on the device at
    every replay (it is set to 3 before the first call: a column that ignored the pointer would stay 0)."""
    from mcquic_amd import monitor, optim, parallel
    from test_gpu_ema_step import _setup
    model, xs, us = _setup(dev)
    if kind == "sgd-clips":
        opt = optim.SGD(model.parameters(), lr=LR, momentum=0.9, max_grad_norm=4.0, skip_nonfinite=True)
    elif kind == "sgd-guards-only":
        opt = optim.SGD(model.parameters(), lr=LR, momentum=0.9, skip_nonfinite=True)
    else:
        opt = optim.Lamb(model.parameters(), lr=1e-3)
    meter = monitor.StepMeter(model, capacity=8, pixels=N * HW * HW)
    step = parallel.GraphedTrainStep(model, opt, xs[0], forward_kwargs={"uniforms": us}, meter=meter)
    assert step.post is not None and step.grad_norm is None
    has_skipped = torch.is_tensor(getattr(opt, "skipped", None))
    assert has_skipped == kind.startswith("sgd")
    if has_skipped:
        opt.skipped.fill_(3)
    norms, skipped = [], []
    for it in range(3):
        step(xs[it % 2])
        norms.append(_opt_norm(opt).clone())
        skipped.append(opt.skipped.clone() if has_skipped else torch.zeros((), dtype=torch.int64, device=dev))
    r = meter.read()
    step.close()
    norms, skipped = torch.stack(norms).cpu().numpy(), torch.stack(skipped).cpu().numpy()
    assert np.isfinite(norms).all() and (norms > 0).all() and len(set(norms.tolist())) == 3
    assert r["grad_norm"].tobytes() == norms.tobytes(), (kind, r["grad_norm"], norms)
    assert r["skipped"].tolist() == skipped.tolist() == [3.0 if has_skipped else 0.0] * 3
    assert r["first_bad_step"] == -1 and r["steps"].tolist() == [0, 1, 2]


def test_eager_post_gives_the_same_rows(runs):
    a, b = runs["meter"]["rows"], runs["eager"]["rows"]
    for key in a:
        assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), key
