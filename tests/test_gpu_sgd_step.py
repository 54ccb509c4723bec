"""parallel.GraphedTrainStep with mcquic_amd.optim.SGD(momentum=0.9, max_grad_norm=4.0, skip_nonfinite=True) -- the optimizer clips and
guards, the step does not -- against the same step with torch.optim.SGD(momentum=0.9) under the step's own max_grad_norm=4.0, on the
smallest Compressor and input of tests/test_gpu_graphed_step.py, two replays each: the same losses and parameters within the bars
that file holds a captured step with momentum or clipping to (losses 1e-6, parameters 4e-6 of max|p|)."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_graphed_step_with_own_sgd_equals_torch_sgd_under_the_steps_clipping(dev):
    from mcquic_amd import Compressor, optim, parallel
    from test_gpu_graphed_step import _uniforms
    ch, ks, hw, n, lr = 32, [64, 32, 16], 64, 2, 1e-2
    torch.manual_seed(17)
    theirs = Compressor(ch, 2, ks).to(dev).train()
    ours = copy.deepcopy(theirs)
    start = [p.detach().clone() for p in theirs.parameters()]
    xs = [(torch.rand((n, 3, hw, hw), generator=torch.Generator().manual_seed(90 + i)) * 2 - 1).to(dev) for i in range(2)]
    us = _uniforms(n, hw, ks, dev, 14)

    step_t = parallel.GraphedTrainStep(theirs, torch.optim.SGD(theirs.parameters(), lr=lr, momentum=0.9), xs[0], forward_kwargs={"uniforms": us},
                                       max_grad_norm=4.0)
    assert step_t.post is not None
    losses_t, norms_t = [], []
    for x in xs:
        losses_t.append(float(step_t(x)))
        norms_t.append(float(step_t.grad_norm))
    step_t.close()

    opt = optim.SGD(ours.parameters(), lr=lr, momentum=0.9, max_grad_norm=4.0, skip_nonfinite=True)
    with pytest.raises(ValueError, match="clip"):
        parallel.GraphedTrainStep(ours, opt, xs[0], forward_kwargs={"uniforms": us}, max_grad_norm=4.0)
    step_o = parallel.GraphedTrainStep(ours, opt, xs[0], forward_kwargs={"uniforms": us})
    assert step_o.post is not None, "the update should have been captured"
    assert step_o.grad_norm is None and int(opt.skipped) == 0
    losses_o, norms_o = [], []
    for x in xs:
        losses_o.append(float(step_o(x)))
        norms_o.append(float(opt.grad_norm()))
    step_o.close()
    torch.cuda.synchronize()

    print(f"losses torch {losses_t} ours {losses_o}; gradient norms torch {norms_t} ours {norms_o}")
    assert int(opt.skipped) == 0
    for a, b in zip(losses_t, losses_o):
        assert abs(a - b) <= 1e-6 * max(1.0, abs(a)), (losses_t, losses_o)
    for a, b in zip(norms_t, norms_o):
        assert abs(a - b) <= 2e-5 * a, (norms_t, norms_o)
    moved = False
    for (name, pt), (_, po), p0 in zip(theirs.named_parameters(), ours.named_parameters(), start):
        scale = max(float(pt.detach().abs().max()), 1e-12)
        assert float((pt.detach() - po.detach()).abs().max()) <= 4e-6 * scale, name
        moved = moved or not torch.equal(po.detach(), p0)
    assert moved
    assert all(float(st["step"]) == 2.0 for st in opt.state.values() if "step" in st)
