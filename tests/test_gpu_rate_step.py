"""GPU: the training objective with the codebook regulariser, `loss.step_loss(rate=BasicRate(g), model=model)`, eagerly and
under `parallel.GraphedTrainStep(segments=1)`, at the small training shapes of the other step tests.

Bars: the kernels' own (tests/test_gpu_codebook_cosine.py: loss 3.9e-7, gradient 1.1e-6 of the largest element, plus the ambiguous
pairs' allowance per row) and one float32 rounding, 2^-23 of the value, for each sum of two float32 numbers that this path adds
(objective + rate; the two gradients that meet on a codebook)."""
import copy

import pytest
import torch

import _cosine_ref as R
from _record import record

pytestmark = pytest.mark.gpu

CH, KS, HW, N, GAMMA = 32, [64, 32, 16], 192, 2, 1e-3
LOSS_BAR, GRAD_BAR, ULP = 3.9e-7, 1.1e-6, 2.0 ** -23


def _uniforms(dev, seed=5):
    g = torch.Generator().manual_seed(seed)
    us = []
    for lv, k in enumerate(KS):
        s = HW // 16 // (2 ** lv)
        us.append((torch.rand((N, 2, s, s, k), generator=g).to(dev), torch.rand((N, 2, s, s, k), generator=g).to(dev)))
    return us


def _setup(dev):
    from mcquic_amd import Compressor
    torch.manual_seed(7)
    model = Compressor(CH, 2, KS).to(dev).train()
    xs = [(torch.rand((N, 3, HW, HW), generator=torch.Generator().manual_seed(20 + i)) * 2 - 1).to(dev) for i in range(2)]
    return model, xs, _uniforms(dev)


def _eager(model, loss_fn, x, us):
    for p in model.parameters():
        p.grad = None
    loss = loss_fn(model(x, uniforms=us), x)
    loss.backward()
    return float(loss.detach()), [c.grad.detach().clone() for c in model.Codebooks]


def test_eager_objective_is_the_plain_one_plus_the_reference_term(dev):
    from mcquic_amd import loss as L
    model, xs, us = _setup(dev)
    refs = [R.cosine_ref(c) for c in model.Codebooks]
    twin = copy.deepcopy(model)                                 # (a training forward moves the frequency EMA: one model per run)
    plain, g_plain = _eager(model, L.step_loss(), xs[0], us)
    full, g_full = _eager(twin, L.step_loss(rate=L.BasicRate(GAMMA), model=twin), xs[0], us)
    term = GAMMA * sum(r.loss for r in refs)
    err = abs(full - (plain + term))
    bar = LOSS_BAR * term + ULP * abs(full)
    print(f"plain {plain:.9g} rate term {term:.9g} full {full:.9g} error {err:.3e} bar {bar:.3e}")
    record("rate_step.eager.loss", value=err, bar=bar)
    assert term > 100 * ULP * abs(plain), "the term is too small for this test to see it"
    assert err <= bar
    for lv, (ref, a, b) in enumerate(zip(refs, g_plain, g_full)):
        want = GAMMA * ref.grad
        dev_rows = ((b.double() - a.double()).cpu() - want).abs().amax(-1)
        allow = GRAD_BAR * float(want.abs().max()) + GAMMA * ref.slack + ULP * float(b.abs().max())
        worst = float((dev_rows - allow).max())
        print(f"level {lv}: worst row deviation {float(dev_rows.max()):.3e}, smallest allowance {float(allow.min()):.3e}, "
              f"rows with an ambiguous pair {ref.ambiguous_rows:.3f}")
        record(f"rate_step.eager.grad_level{lv}", value=float(dev_rows.max()), bar=float(allow.min()))
        assert ref.ambiguous_rows <= 0.15
        assert worst <= 0, (lv, worst)


def test_graphed_single_segment_step_with_the_rate_term(dev):
    from mcquic_amd import loss as L
    from mcquic_amd import parallel
    model, xs, us = _setup(dev)
    graphed, plain_model = copy.deepcopy(model), copy.deepcopy(model)
    eager_loss, _ = _eager(model, L.step_loss(rate=L.BasicRate(GAMMA), model=model), xs[0], us)
    plain_loss, _ = _eager(plain_model, L.step_loss(), xs[0], us)
    opt = torch.optim.SGD(graphed.parameters(), lr=1e-3)
    step = parallel.GraphedTrainStep(graphed, opt, xs[0], loss_fn=L.step_loss(rate=L.BasicRate(GAMMA), model=graphed),
                                     forward_kwargs={"uniforms": us}, segments=1)
    first = float(step(xs[0]))
    second = float(step(xs[0]))
    step.close()
    print(f"eager {eager_loss:.9g} first replay {first:.9g} second {second:.9g} (without the term {plain_loss:.9g})")
    assert abs(first - eager_loss) <= 1e-6 * max(1.0, abs(eager_loss))
    assert abs(first - plain_loss) > 10 * ULP * abs(plain_loss)                 # the term is in the captured objective
    assert torch.isfinite(torch.tensor(second)) and second != first             # the update went through


def test_three_segments_refuse_a_loss_that_reads_the_codebooks(dev):
    from mcquic_amd import loss as L
    from mcquic_amd import parallel
    model, xs, us = _setup(dev)
    opt = torch.optim.SGD(model.parameters(), lr=1e-3)
    with pytest.raises(ValueError, match="segments=1"):
        parallel.GraphedTrainStep(model, opt, xs[0], loss_fn=L.step_loss(rate=L.BasicRate(GAMMA), model=model),
                                  forward_kwargs={"uniforms": us}, segments=3)


def test_without_a_rate_the_objective_keeps_its_bits(dev):
    from mcquic_amd import loss as L
    torch.manual_seed(3)
    xHat = (torch.rand(2, 3, HW, HW, device=dev) * 2 - 1).requires_grad_()
    x = torch.rand(2, 3, HW, HW, device=dev) * 2 - 1
    fn = L.step_loss()
    assert not hasattr(fn, "single_segment")
    a = fn((xHat, None, None, None), x)
    a.backward()
    ga, xHat.grad = xHat.grad.clone(), None
    b = L._MsSsimMseFn.apply(xHat, x, 0.5, 0.5)                 # the one node the default path has always been
    b.backward()
    assert type(a.grad_fn) is type(b.grad_fn) and torch.equal(a.detach(), b.detach()) and torch.equal(ga, xHat.grad)
