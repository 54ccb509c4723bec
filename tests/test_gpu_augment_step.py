"""parallel.GraphedTrainStep(..., transform=TrainingInput(...)): the input transform's two launches captured at the head of the
step.  The graphed step on raw uint8 batches against an eager model that is given `ops.augment(raw, size, params)` under the
table the replay drew (`transform.last_params`) -- same losses, same parameters, at the bar of tests/test_gpu_graphed_step.py's
eager-versus-graphed comparison (losses 1e-6 relative, parameters 2e-6 of their largest entry); the tables differ from replay to
replay; one graph or three segment graphs (the constructor allows segments=3 without a process group); and with
transform=None the step is what it was."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

KS = [64, 32, 16]


def _uniforms(n, hw, dev, seed):
    g = torch.Generator().manual_seed(seed)
    us = []
    for lv, k in enumerate(KS):
        s = hw // 16 // (2 ** lv)
        us.append((torch.rand((n, 2, s, s, k), generator=g).to(dev), torch.rand((n, 2, s, s, k), generator=g).to(dev)))
    return us


def _planckian():
    return torch.rand((9, 2), generator=torch.Generator().manual_seed(31)) * 0.8 + 0.6


@pytest.mark.parametrize("segments", [1, 3])
def test_graphed_step_with_transform_equals_eager(dev, segments):
    from mcquic_amd import Compressor, ops, parallel
    from mcquic_amd.data.transforms import TrainingInput
    n, steps, lr, size = 2, 3, 1e-3, (64, 64)
    torch.manual_seed(7)
    eager = Compressor(32, 2, KS).to(dev).train()
    graphed = copy.deepcopy(eager)
    raws = [torch.randint(0, 256, (n, 3, 96, 80), generator=torch.Generator().manual_seed(40 + i), dtype=torch.uint8).to(dev)
            for i in range(steps)]
    us = _uniforms(n, 64, dev, 5)
    transform = TrainingInput(size, (0.75, 1.0), (0.95, 1.05), planckian=_planckian(), seed=99)
    opt_g = torch.optim.SGD(graphed.parameters(), lr=lr)
    step = parallel.GraphedTrainStep(graphed, opt_g, raws[0], forward_kwargs={"uniforms": us}, segments=segments, transform=transform)
    assert len(step.graphs) == segments and step.post is not None
    assert tuple(step.x.shape) == (n, 3) + size and step.x.dtype == torch.float32 and step.raw.dtype == torch.uint8

    opt_e = torch.optim.SGD(eager.parameters(), lr=lr)
    tables, offsets = [], []
    for raw in raws:
        loss_g = float(step(raw))
        table = transform.last_params.clone()
        tables.append(table.cpu())
        offsets.append(int(transform.state_dict()["rng"][1]))
        x = ops.augment(raw, size, table)
        assert torch.equal(x, step.x)                         # the model's input of that replay
        opt_e.zero_grad(set_to_none=True)
        loss = torch.nn.functional.mse_loss(eager(x, uniforms=us)[0], x)
        loss.backward()
        opt_e.step()
        loss_e = float(loss.detach())
        assert abs(loss_e - loss_g) <= 1e-6 * max(1.0, abs(loss_e)), (loss_e, loss_g)
    with pytest.raises(RuntimeError, match="captured for"):
        step(raws[0].float())
    step.close()
    torch.cuda.synchronize()

    assert offsets[0] < offsets[1] < offsets[2]               # the captured draw advanced the offset on every replay
    assert not torch.equal(tables[0], tables[1]) and not torch.equal(tables[1], tables[2]) and not torch.equal(tables[0], tables[2])
    for t in tables:
        assert bool((t[:, ops.AUG_GAIN_ROW] >= 0).all()) and bool((t[:, ops.AUG_H] >= 1).all())
    for (name, pe), (_, pg) in zip(eager.named_parameters(), graphed.named_parameters()):
        scale = max(float(pe.detach().abs().max()), 1e-12)
        assert float((pe.detach() - pg.detach()).abs().max()) <= 2e-6 * scale, name


def test_resuming_the_generator_state_repeats_the_tables(dev):
    """Checkpointing {seed, offset} resumes the stream: a second step built from the saved state draws the same tables."""
    from mcquic_amd import Compressor, parallel
    from mcquic_amd.data.transforms import TrainingInput
    torch.manual_seed(3)
    model = Compressor(32, 2, KS).to(dev).train()
    raw = torch.randint(0, 256, (2, 3, 96, 80), generator=torch.Generator().manual_seed(1), dtype=torch.uint8).to(dev)
    us = _uniforms(2, 64, dev, 5)
    transform = TrainingInput((64, 64), seed=5)
    step = parallel.GraphedTrainStep(model, torch.optim.SGD(model.parameters(), lr=1e-3), raw, forward_kwargs={"uniforms": us},
                                     transform=transform)
    saved = {k: v.clone() for k, v in transform.state_dict().items()}
    first = []
    for _ in range(2):
        step(raw)
        first.append(transform.last_params.clone())
    transform.load_state_dict(saved)                          # in place: the graph keeps reading the same device tensor
    for want in first:
        step(raw)
        assert torch.equal(transform.last_params, want)
    step.close()


def test_without_a_transform_nothing_changes(dev):
    """transform=None: the same seed gives the same losses bit for bit, with or without the keyword."""
    from mcquic_amd import Compressor, parallel
    torch.manual_seed(11)
    base = Compressor(32, 2, KS).to(dev).train()
    xs = [(torch.rand((2, 3, 64, 64), generator=torch.Generator().manual_seed(60 + i)) * 2 - 1).to(dev) for i in range(3)]
    us = _uniforms(2, 64, dev, 5)
    losses = []
    for kw in ({}, {"transform": None}):
        model = copy.deepcopy(base)
        step = parallel.GraphedTrainStep(model, torch.optim.SGD(model.parameters(), lr=1e-3), xs[0], forward_kwargs={"uniforms": us}, **kw)
        assert step.transform is None and step.raw is None
        losses.append([float(step(x)) for x in xs])
        step.close()
    assert losses[0] == losses[1]
