"""mcquic_amd.optim.EMA through parallel.GraphedTrainStep(..., ema=...), on the model and shards of tests/test_gpu_sgd_step.py:
Compressor(32, 2, [64, 32, 16]), two 64 x 64 images, fixed uniforms, mcquic_amd.optim.SGD.  Everything here is compared bit for bit: the
step's kernels and the EMA's are deterministic, and the EMA inside the post graph runs the launches an eager `ema.update()` runs."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
CH, KS, HW, N, LR = 32, [64, 32, 16], 64, 2, 1e-2
# the run whose average must ENCODE differently from its iterate (test_model_under_the_average_...): the average has to lag far enough.
# Measured on an MI355X, codes that differ of 336 after 8 steps: lr 1e-2 (any decay) 0; lr 5e-2, decay 0.5 or 0.9: 1; lr 0.2, decay 0.9: 4
# (all parameters finite, loss 0.3370 -> 0.3331).
AVG_LR, AVG_DECAY, AVG_STEPS = 0.2, 0.9, 8


def _setup(dev, seed=17):
    from mcquic_amd import Compressor
    from test_gpu_graphed_step import _uniforms
    torch.manual_seed(seed)
    model = Compressor(CH, 2, KS).to(dev).train()
    xs = [(torch.rand((N, 3, HW, HW), generator=torch.Generator().manual_seed(90 + i)) * 2 - 1).to(dev) for i in range(2)]
    return model, xs, _uniforms(N, HW, KS, dev, 14)


def _same(a, b):
    return all(torch.equal(x.detach(), y.detach()) for x, y in zip(a, b))


@pytest.mark.parametrize("capture_post", [True, False], ids=["post-graph", "post-eager"])
def test_step_with_ema_equals_step_then_eager_update(dev, capture_post):
    """(a) constructing the step leaves averages and count as they were; (b) four replays with `ema=` are the bits of the same step without it
    followed by an eager `ema.update()`, parameters and averages."""
    from mcquic_amd import optim, parallel
    ours, xs, us = _setup(dev)
    ema_o = optim.EMA(ours, decay=0.9, warmup=True)
    with torch.no_grad():
        for p in ours.parameters():
            p.mul_(1.01)
    ema_o.update()                                            # averages != parameters, one update counted, before the step exists
    twin = copy.deepcopy(ours)
    ema_t = optim.EMA(twin, decay=0.9, warmup=True)
    ema_t.load_state_dict(ema_o.state_dict())
    before = ema_o._flat.clone()
    assert not _same(ema_o.averages, ema_o.params)

    step_o = parallel.GraphedTrainStep(ours, optim.SGD(ours.parameters(), lr=LR, momentum=0.9), xs[0], forward_kwargs={"uniforms": us},
                                       capture_post=capture_post, ema=ema_o)
    assert (step_o.post is not None) == capture_post
    assert torch.equal(ema_o._flat, before) and ema_o.num_updates == 1, "the constructor moved the average"
    assert _same(ours.parameters(), twin.parameters())
    step_t = parallel.GraphedTrainStep(twin, optim.SGD(twin.parameters(), lr=LR, momentum=0.9), xs[0], forward_kwargs={"uniforms": us},
                                       capture_post=capture_post)
    for it in range(4):
        lo, lt = step_o(xs[it % 2]), step_t(xs[it % 2])
        ema_t.update()
        assert torch.equal(lo, lt), it
        assert _same(ours.parameters(), twin.parameters()), it
        assert _same(ema_o.averages, ema_t.averages), it
    assert ema_o.num_updates == ema_t.num_updates == 5
    assert not torch.equal(ema_o._flat, before) and not _same(ema_o.averages, ema_o.params)
    step_o.close()
    step_t.close()


def test_model_under_the_average_equals_a_model_loaded_with_it(dev):
    """(c) under `applied()` the model encodes and decodes as a fresh Compressor loaded with `averaged_state_dict()` does, eagerly and through
    `enableGraphs()`; on exit the live weights are back, bits and codes.  (d) the step refuses to run in between."""
    from mcquic_amd import Compressor, optim, parallel
    model, xs, us = _setup(dev)
    lr, decay, steps = AVG_LR, AVG_DECAY, AVG_STEPS
    ema = optim.EMA(model, decay=decay, warmup=False)
    step = parallel.GraphedTrainStep(model, optim.SGD(model.parameters(), lr=lr, momentum=0.9), xs[0], forward_kwargs={"uniforms": us}, ema=ema)
    for it in range(steps):
        step(xs[it % 2])
    step.invalidate()
    model.eval()
    x = xs[1]
    live_codes = model.encode(x)
    live_bits = [p.detach().clone() for p in model.parameters()]
    model.enableGraphs()
    assert _same(model.encode(x), live_codes)                 # (captures taken under the LIVE weights: the swap must drop them)

    with ema.applied():
        codes = model.encode(x)
        rec = model.decode(codes)
        model.enableGraphs(False)
        eager_codes = model.encode(x)
        eager_rec = model.decode(eager_codes)
        fresh = Compressor(CH, 2, KS).to(dev).eval()
        fresh.load_state_dict(ema.averaged_state_dict())
        want_codes = fresh.encode(x)
        want_rec = fresh.decode(want_codes)
        with pytest.raises(RuntimeError):                     # (d)
            step(xs[0])
        model.enableGraphs()
        model.encode(x)                                       # (captures under the AVERAGE: the swap back must drop these)
    assert _same(codes, want_codes) and torch.equal(rec, want_rec), "graphed calls under the average"
    assert _same(eager_codes, want_codes) and torch.equal(eager_rec, want_rec), "eager calls under the average"

    assert _same(model.parameters(), live_bits), "the live weights came back with other bits"
    assert _same(model.encode(x), live_codes), "graphed encode after the swap back"
    model.enableGraphs(False)
    assert _same(model.encode(x), live_codes), "eager encode after the swap back"
    differ = sum(int((a != b).sum()) for a, b in zip(want_codes, live_codes))
    total = sum(a.numel() for a in live_codes)
    print(f"codes under the average that differ from the live model's: {differ} of {total}")
    assert differ > 0, "the average encodes like the iterate: this test would pass with a swap that does nothing"
    model.train()
    step(xs[0])                                               # the step goes on
    assert ema.num_updates == steps + 1
    step.close()


def test_ema_checkpoint_round_trip_continues_bit_for_bit(dev):
    """(e) `state_dict()` into a new EMA (built with other settings) on a copy of the model, then two more steps on both."""
    from mcquic_amd import Compressor, optim, parallel
    a, xs, us = _setup(dev)
    ema_a = optim.EMA(a, decay=0.9, warmup=True)
    step_a = parallel.GraphedTrainStep(a, optim.SGD(a.parameters(), lr=LR), xs[0], forward_kwargs={"uniforms": us}, ema=ema_a)     # (no momentum: no optimizer state to carry)
    for it in range(2):
        step_a(xs[it])
    step_a.invalidate()
    b = Compressor(CH, 2, KS).to(dev).train()
    b.load_state_dict(a.state_dict())
    ema_b = optim.EMA(b, decay=0.1, warmup=False)
    sd = copy.deepcopy(ema_a.state_dict())
    assert sd["num_updates"] == 2 and sd["decay"] == 0.9 and sd["warmup"] is True and list(sd["averages"]) == ema_a.names
    ema_b.load_state_dict(sd)
    assert (ema_b.decay, ema_b.warmup, ema_b.num_updates) == (0.9, True, 2) and _same(ema_a.averages, ema_b.averages)
    step_b = parallel.GraphedTrainStep(b, optim.SGD(b.parameters(), lr=LR), xs[0], forward_kwargs={"uniforms": us}, ema=ema_b)
    assert ema_b.num_updates == 2 and _same(ema_a.averages, ema_b.averages)
    for it in range(2):
        step_a(xs[it])
        step_b(xs[it])
    assert ema_a.num_updates == ema_b.num_updates == 4
    assert _same(a.parameters(), b.parameters()) and _same(ema_a.averages, ema_b.averages)
    assert not _same(ema_a.averages, [sd["averages"][n] for n in ema_a.names])
    step_a.close()
    step_b.close()
