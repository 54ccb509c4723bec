"""GPU: parallel.GraphedTrainStep(accumulate=k) -- k micro-batches per call, ONE update -- on the small models and the deterministic
forward (`uniforms`) of tests/test_gpu_graphed_step.py: against the plain step, against an eager twin that accumulates by hand with the
coder in deferred mode, composed with every helper of the update, and its arguments.  The arithmetic the kernels are held to is
tests/_accum_ref.py's (tests/test_gpu_accum_leaf.py: bit for bit)."""
import copy

import numpy as np
import pytest
import torch

import _accum_ref as A
from test_gpu_graphed_step import _uniforms

pytestmark = pytest.mark.gpu

CH, KS, HW, N = 32, [64, 32, 16], 64, 2


def _batch(seed, dev, n=N):
    return (torch.rand((n, 3, HW, HW), generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(dev)


def _model(dev, seed=7):
    from mcquic_amd import Compressor
    torch.manual_seed(seed)
    return Compressor(CH, 2, KS).to(dev).train()


def _opt_state(opt):
    out = [v for st in opt.state.values() for _, v in sorted(st.items()) if torch.is_tensor(v)]
    return out + [plan.step for plan in getattr(opt, "_plans", {}).values()]


def _freqs(model):
    return list(model._quantizer._entropyCoder._freqEMA)


def _close_params(a, b, bar):
    for (name, pa), (_, pb) in zip(a.named_parameters(), b.named_parameters()):
        scale = max(float(pa.detach().abs().max()), 1e-12)
        assert float((pa.detach() - pb.detach()).abs().max()) <= bar * scale, name


@pytest.mark.parametrize("kind", ["sgd", "adam"])
def test_two_of_the_same_micro_batch_is_the_plain_step(dev, kind):
    """accumulate=2 fed the same micro-batch twice against accumulate=1 on it, twin models, 3 updates.  The agreement is BIT FOR BIT, and
    torch.equal is what is asserted: the captured forward and backward under `uniforms` have no order-dependent reduction (every launch
    sums in a fixed order; the one float atomic has two addends), so both replays leave the same gradient g, and (g + g) * 0.5 is g
    exactly; the doubled counts give the same normalised frequencies (a factor of two commutes with every rounding) and (l + l) * 0.5
    is the loss."""
    from mcquic_amd import optim, parallel
    one, two = _model(dev), None
    two = copy.deepcopy(one)
    us = _uniforms(N, HW, KS, dev, 5)
    xs = [_batch(20 + i, dev) for i in range(3)]

    def make(m):
        return torch.optim.SGD(m.parameters(), lr=1e-2, momentum=0.9) if kind == "sgd" else optim.Adam(m.parameters(), lr=1e-3)
    opt1, opt2 = make(one), make(two)
    s1 = parallel.GraphedTrainStep(one, opt1, xs[0], forward_kwargs={"uniforms": us})
    s2 = parallel.GraphedTrainStep(two, opt2, xs[0], forward_kwargs={"uniforms": us}, accumulate=2)
    assert s1.accumulate == 1 and s2.accumulate == 2 and s1.post is not None and s2.post is not None
    assert len(s2.graphs) == len(s1.graphs) == 1
    before = [p.detach().clone() for p in one.parameters()]
    for x in xs:
        l1 = s1(x).clone()
        l2 = s2(torch.cat([x, x])).clone()
        assert torch.equal(l1, l2)
        assert torch.equal(s2.counts, 2 * s1.counts)
        assert torch.equal(s1.flat, s2.flat)
    s1.close()
    s2.close()
    torch.cuda.synchronize()
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, one.parameters()))
    for (name, pa), (_, pb) in zip(one.named_parameters(), two.named_parameters()):
        assert torch.equal(pa.detach(), pb.detach()), name
    sa, sb = _opt_state(opt1), _opt_state(opt2)
    assert len(sa) == len(sb) > 0 and all(torch.equal(a, b) for a, b in zip(sa, sb))
    assert all(torch.equal(a, b) for a, b in zip(_freqs(one), _freqs(two)))
    one.eval()
    two.eval()
    with torch.no_grad():
        assert all(torch.equal(a, b) for a, b in zip(one.encode(xs[0]), two.encode(xs[0])))


def test_three_distinct_micro_batches_equal_an_eager_twin(dev):
    """k = 3 against an eager twin: its coder in deferred mode, three forwards and backwards, `.grad` summed in order and multiplied by
    float32(1 / 3), ONE optimizer step, the summed counts applied once.  Parameters and `_freqEMA` to the bars of
    test_graphed_step_equals_eager_step (2e-6 of a parameter's largest magnitude; 1e-7); `step.loss` is the mean of the twin's losses by
    the accumulation rule, to 1 ulp."""
    from mcquic_amd import parallel
    from mcquic_amd.autograd import mse_loss
    k, updates, lr = 3, 3, 1e-3
    eager = _model(dev)
    graphed = copy.deepcopy(eager)
    us = _uniforms(N, HW, KS, dev, 5)
    xs = [torch.cat([_batch(100 + 10 * u + j, dev) for j in range(k)]) for u in range(updates)]
    inv = A.inv_k(k).to(dev)
    coder = eager._quantizer._entropyCoder
    coder.deferCounts(True)
    opt_e = torch.optim.SGD(eager.parameters(), lr=lr)
    params = [p for p in eager.parameters() if p.requires_grad]
    want_losses = []
    for x in xs:
        sums, counts, losses = None, None, []
        for j in range(k):
            mb = x[j * N: (j + 1) * N]
            opt_e.zero_grad(set_to_none=True)
            loss = mse_loss(eager(mb, uniforms=us)[0], mb)
            loss.backward()
            losses.append(loss.detach().cpu())
            grads = [None if p.grad is None else p.grad.detach().clone() for p in params]
            sums = grads if sums is None else [s if g is None else s + g for s, g in zip(sums, grads)]
            c = coder.countSink().clone()
            counts = c if counts is None else counts + c
        for p, s in zip(params, sums):
            p.grad = None if s is None else s * inv
        opt_e.step()
        coder.applyCounts(counts)
        want_losses.append(A.accum_all(losses))
    coder.deferCounts(False)

    step = parallel.GraphedTrainStep(graphed, torch.optim.SGD(graphed.parameters(), lr=lr), xs[0][:N], forward_kwargs={"uniforms": us}, accumulate=k)
    assert step.post is not None
    got_losses = [step(x).clone().cpu() for x in xs]
    total = int(step.counts.sum())
    step.close()
    torch.cuda.synchronize()
    assert total == k * N * 2 * sum((HW // 16 // 2 ** lv) ** 2 for lv in range(len(KS)))       # every code of every micro-batch, once
    for want, got in zip(want_losses, got_losses):
        print("loss", float(want), float(got))
        assert abs(float(got) - float(want)) <= float(np.spacing(np.float32(abs(float(want))))), (want_losses, got_losses)
    _close_params(eager, graphed, 2e-6)
    for fe, fg in zip(_freqs(eager), _freqs(graphed)):
        assert torch.allclose(fe, fg, rtol=0, atol=1e-7)


def _helpers(dev, model, x, **extra):
    from mcquic_amd import monitor, optim, parallel, schedule
    opt = optim.Adam(model.parameters(), lr=1e-3)
    ema = optim.EMA(model, decay=0.9)
    sched = schedule.CosineAnnealingWarmupRestarts(opt, 8, warmup_steps=2)
    meter = monitor.StepMeter(model, capacity=8, pixels=2 * N * HW * HW)
    step = parallel.GraphedTrainStep(model, opt, x, forward_kwargs={"uniforms": _uniforms(N, HW, KS, dev, 5)}, max_grad_norm=4.0, ema=ema,
                                     scheduler=sched, meter=meter, skip_nonfinite=True, accumulate=2, **extra)
    return dict(model=model, opt=opt, ema=ema, sched=sched, meter=meter, step=step)


def test_one_update_per_call_with_every_helper(dev):
    """scheduler, EMA, meter, guard and clip around accumulate=2: three calls are three updates, the meter's rows carry `step.loss` and
    the SUMMED counts, and an inf in ONE of the two micro-batches makes the guard skip the whole update."""
    from test_gpu_step_guard_step import _same, _state
    w = _helpers(dev, _model(dev), _batch(1, dev))
    step, guard, sched, ema, meter = w["step"], w["step"].guard, w["sched"], w["ema"], w["meter"]
    assert step.post is not None
    epoch0, ema0 = sched.last_epoch, ema.num_updates
    per_group = [2 * N * (HW // 16 // 2 ** lv) ** 2 for lv in range(len(KS))]      # codes per (level, group) in one CALL
    losses = []
    for i in range(3):
        losses.append(float(step(torch.cat([_batch(30 + 2 * i, dev), _batch(31 + 2 * i, dev)]))))
        assert meter.partials()["total"].tolist() == [c for c in per_group for _ in range(2)]
        assert int(step.counts.sum()) == 2 * sum(per_group)
    assert sched.last_epoch == epoch0 + 3 and ema.num_updates == ema0 + 3
    assert (int(guard.skip), int(guard.skipped)) == (0, 0)
    rows = meter.read()
    assert len(rows["loss"]) == 3 and rows["loss"].tolist() == [np.float32(l) for l in losses]
    assert np.isfinite(rows["grad_norm"]).all() and float(rows["grad_norm"][2]) == float(step.grad_norm)
    assert (rows["bpp"] > 0).all() and (rows["hit"] > 0).all()

    before = [t.detach().clone() for t in _state(w)]
    bad = _batch(40, dev)
    bad[1, 2, 7, 5] = float("inf")
    loss = step(torch.cat([bad, _batch(41, dev)]))                          # the FIRST micro-batch: the inf has to survive the sum
    assert not torch.isfinite(loss)
    assert _same(_state(w), before), "a skipped update leaves parameters, optimizer state, EMA, _freqEMA and schedule bit for bit"
    assert (int(guard.skip), int(guard.skipped)) == (1, 1) and not np.isfinite(float(guard.grad_norm))
    assert sched.last_epoch == epoch0 + 3 and ema.num_updates == ema0 + 3
    loss = step(torch.cat([_batch(42, dev), bad]))                          # ... and in the LAST one
    assert not torch.isfinite(loss) and _same(_state(w), before) and int(guard.skipped) == 2
    step(torch.cat([_batch(42, dev), _batch(43, dev)]))
    assert int(guard.skip) == 0 and int(guard.skipped) == 2 and not _same(_state(w), before)
    assert meter.read()["skipped"].tolist() == [1, 2, 2]
    step.close()


def test_segments_three_equals_one(dev):
    """segments=3 with accumulate=2 on one rank (three accumulating gathers, one per slice) against segments=1, at the bars of
    test_graphed_step_equals_eager_step."""
    from mcquic_amd import parallel
    a = _model(dev)
    b = copy.deepcopy(a)
    us = _uniforms(N, HW, KS, dev, 5)
    xs = [torch.cat([_batch(50 + 2 * i, dev), _batch(51 + 2 * i, dev)]) for i in range(3)]
    s1 = parallel.GraphedTrainStep(a, torch.optim.SGD(a.parameters(), lr=1e-3), xs[0][:N], forward_kwargs={"uniforms": us}, segments=1, accumulate=2)
    s3 = parallel.GraphedTrainStep(b, torch.optim.SGD(b.parameters(), lr=1e-3), xs[0][:N], forward_kwargs={"uniforms": us}, segments=3, accumulate=2)
    assert len(s1.graphs) == 1 and len(s3.graphs) == 3 and len(s3.slices) == 3 and all(sl.numel() for sl in s3.slices)
    for x in xs:
        l1, l3 = float(s1(x)), float(s3(x))
        assert abs(l1 - l3) <= 1e-6 * max(1.0, abs(l1))
        assert torch.equal(s1.counts, s3.counts)
    s1.close()
    s3.close()
    _close_params(a, b, 2e-6)
    for fa, fb in zip(_freqs(a), _freqs(b)):
        assert torch.allclose(fa, fb, rtol=0, atol=1e-7)


def test_arguments_and_shapes(dev):
    from mcquic_amd import parallel
    model = _model(dev)
    us = _uniforms(N, HW, KS, dev, 5)
    x = _batch(3, dev)
    for bad in (0, -1, 1.5, True, "2", None):
        with pytest.raises(ValueError, match="accumulate"):
            parallel.GraphedTrainStep(model, torch.optim.SGD(model.parameters(), lr=1e-3), x, forward_kwargs={"uniforms": us}, accumulate=bad)
    plain = parallel.GraphedTrainStep(model, torch.optim.SGD(model.parameters(), lr=1e-3), x, forward_kwargs={"uniforms": us}, accumulate=1)
    sink = plain.coders[0].countSink()
    assert plain.accumulate == 1 and plain.counts is sink and plain._phase is None and plain._countsAcc is None      # the old path
    plain(x)
    with pytest.raises(RuntimeError, match="captured for shards of shape"):
        plain(torch.cat([x, x]))
    plain.close()
    step = parallel.GraphedTrainStep(model, torch.optim.SGD(model.parameters(), lr=1e-3), x, forward_kwargs={"uniforms": us}, accumulate=2)
    assert step.accumulate == 2 and step.counts.data_ptr() != step.coders[0].countSink().data_ptr()
    assert tuple(step.x.shape) == (N, 3, HW, HW), "the capture shape is ONE micro-batch"
    for wrong in (x, torch.cat([x, x, x]), torch.cat([x, x])[:3]):
        with pytest.raises(RuntimeError, match=r"captured for shards of shape .*accumulate=2"):
            step(wrong)
    assert bool(torch.isfinite(step(torch.cat([x, x]))))
    step.close()


def test_transform_draws_afresh_in_every_micro_step(dev):
    """With a `transform`, x is the raw batch and every replay draws: after one call with accumulate=2 the table is the SECOND draw of a
    same-seed transform under a plain step (which differs from its first), and the generator's offset has advanced as far."""
    from mcquic_amd import parallel
    from mcquic_amd.data.transforms import TrainingInput
    base = _model(dev, 3)
    us = _uniforms(N, HW, KS, dev, 5)
    raws = [torch.randint(0, 256, (N, 3, 96, 80), generator=torch.Generator().manual_seed(70 + i), dtype=torch.uint8).to(dev) for i in range(2)]
    tables, offsets = {}, {}
    for acc in (1, 2):
        model = copy.deepcopy(base)
        transform = TrainingInput((HW, HW), seed=5)
        step = parallel.GraphedTrainStep(model, torch.optim.SGD(model.parameters(), lr=1e-3), raws[0], forward_kwargs={"uniforms": us},
                                         transform=transform, accumulate=acc)
        if acc == 1:
            tables[1] = []
            for raw in raws:
                step(raw)
                tables[1].append(transform.last_params.clone())
        else:
            assert step.raw.dtype == torch.uint8 and tuple(step.raw.shape) == (N, 3, 96, 80)
            assert bool(torch.isfinite(step(torch.cat(raws))))
            tables[2] = transform.last_params.clone()
            with pytest.raises(RuntimeError, match="captured for"):
                step(torch.cat(raws).float())
        offsets[acc] = int(transform.state_dict()["rng"][1])
        step.close()
    assert not torch.equal(tables[1][0], tables[1][1])
    assert torch.equal(tables[2], tables[1][1])
    assert offsets[1] == offsets[2]


def test_neon_through_the_same_path(dev):
    from mcquic_amd import Neon, parallel
    torch.manual_seed(11)
    model = Neon(32, 256, [8, 4, 2, 2], False).to(dev).train()             # (tests/test_neon.py's fixture configuration)
    x = (torch.rand((4, 3, 128, 128), generator=torch.Generator().manual_seed(6)) * 2 - 1).to(dev)
    step = parallel.GraphedTrainStep(model, torch.optim.SGD(model.parameters(), lr=1e-2), x[:2], accumulate=2)
    losses = [float(step(x)) for _ in range(3)]
    assert all(l == l and l < 10 for l in losses), losses
    assert int(step.counts.sum()) == 2 * int(step.coders[0].countSink().sum()) > 0      # both micro-batches' codes (same count of codes each)
    step.close()
