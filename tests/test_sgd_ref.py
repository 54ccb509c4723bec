"""Without a GPU: the float64 restatement of SGD (tests/_sgd_ref.py) against torch.optim.SGD and torch.nn.utils.clip_grad_norm_ on float64
CPU tensors, its skip rule, and the host side of mcquic_amd.optim.SGD: constructor validation, exports, the entry point's declaration and
argument checks (csrc/sgd.hip returns before any launch), checkpoints in torch.optim.SGD's layout."""
import copy
import os
import re

import pytest
import torch

from _sgd_ref import RefSGD, setting_id, settings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1,), (5,), (7, 3, 3, 3), (257,)]


def _values(seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g, dtype=torch.float64) * scale for s in SHAPES]


@pytest.mark.parametrize("max_grad_norm", [None, 0.5])
@pytest.mark.parametrize("kw", settings(), ids=setting_id)
def test_restatement_is_torch_sgd(kw, max_grad_norm):
    """3 steps, within 1e-12 relative of torch.optim.SGD on float64; the clipped runs against clip_grad_norm_ followed by the step
    (gradients of norm ~ 9, so a bound of 0.5 bites at every step)."""
    ours = _values(1)
    theirs = [torch.nn.Parameter(v.clone()) for v in ours]
    ref = RefSGD(ours, lr=0.05, max_grad_norm=max_grad_norm, **kw)
    opt = torch.optim.SGD(theirs, lr=0.05, **kw)
    for it in range(3):
        grads = _values(10 + it, 0.5)
        for p, g in zip(theirs, grads):
            p.grad = g.clone()
        if max_grad_norm is not None:
            norm = float(torch.nn.utils.clip_grad_norm_(theirs, max_grad_norm))
            assert norm > max_grad_norm
        opt.step()
        ref.update(grads)
        if max_grad_norm is not None:
            assert abs(ref.grad_norm - norm) <= 1e-12 * norm
    for i, (a, b) in enumerate(zip(ours, theirs)):
        assert float((a - b.detach()).abs().max()) <= 1e-12 * float(b.detach().abs().max()), SHAPES[i]
        if kw["momentum"] != 0.0:
            m = opt.state[b]["momentum_buffer"]
            assert float((ref.bufs[i] - m).abs().max()) <= 1e-12 * float(m.abs().max()), SHAPES[i]
        else:
            assert ref.bufs[i] is None and "momentum_buffer" not in opt.state[b]


def test_restatement_clip_factor_and_skip_rule():
    # a bound above the norm: the factor is exactly 1, the run is the unclipped one
    a, b = _values(2), _values(2)
    ra, rb = RefSGD(a, lr=0.1, momentum=0.9, max_grad_norm=1e6), RefSGD(b, lr=0.1, momentum=0.9)
    for it in range(2):
        ra.update(_values(20 + it))
        rb.update(_values(20 + it))
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and rb.grad_norm is None
    want = float(torch.cat([g.reshape(-1) for g in _values(21)]).norm())
    assert abs(ra.grad_norm - want) <= 1e-12 * want
    # a non-finite gradient: nothing moves, the next finite update is still the first one
    c, d = _values(3), _values(3)
    rc, rd = RefSGD(c, lr=0.1, momentum=0.9, dampening=0.1, skip_nonfinite=True), RefSGD(d, lr=0.1, momentum=0.9, dampening=0.1)
    for bad in (float("inf"), float("nan")):
        g = _values(30)
        g[2].view(-1)[-1] = bad
        rc.update(g)
    assert rc.skipped == 2 and rc.steps == 0 and all(x is None for x in rc.bufs) and all(torch.equal(x, y) for x, y in zip(c, _values(3)))
    rc.update(_values(31))
    rd.update(_values(31))
    assert rc.steps == 1 and all(torch.equal(x, y) for x, y in zip(c, d)) and all(torch.equal(x, y) for x, y in zip(rc.bufs, rd.bufs))


def _p():
    return [torch.nn.Parameter(torch.ones(4))]


def test_sgd_constructor_validates_like_torch():
    from mcquic_amd import optim
    for kw, msg in ((dict(lr=-1.0), "Invalid learning rate"), (dict(momentum=-0.1), "Invalid momentum value"),
                    (dict(weight_decay=-1e-3), "Invalid weight_decay value"), (dict(lr=torch.zeros(2)), "Tensor lr must be 1-element"),
                    (dict(nesterov=True), "Nesterov momentum requires a momentum and zero dampening"),
                    (dict(nesterov=True, momentum=0.9, dampening=0.1), "Nesterov momentum requires a momentum and zero dampening"),
                    (dict(max_grad_norm=0.0), "Invalid max_grad_norm"), (dict(max_grad_norm=-4.0), "Invalid max_grad_norm")):
        with pytest.raises(ValueError, match=msg):
            optim.SGD(_p(), **kw)
        if "max_grad_norm" not in kw:
            with pytest.raises(ValueError, match=msg):
                torch.optim.SGD(_p(), **kw)
    opt = optim.SGD(_p())
    g = opt.param_groups[0]
    assert (g["lr"], g["momentum"], g["dampening"], g["weight_decay"], g["nesterov"], g["maximize"]) == (1e-3, 0.0, 0.0, 0.0, False, False)
    assert opt.max_grad_norm is None and opt.skip_nonfinite is False
    with pytest.raises(NotImplementedError):
        opt.step(lambda: 0.0)
    with pytest.raises(RuntimeError, match="max_grad_norm"):
        opt.grad_norm()                                       # neither option is on: no norm is computed
    assert opt.skipped.dtype == torch.int64 and opt.skipped.dim() == 0 and int(opt.skipped) == 0


def test_sgd_is_exported_and_the_registry_is_unchanged():
    from mcquic_amd import optim
    assert "SGD" in optim.__all__ and issubclass(optim.SGD, torch.optim.Optimizer)
    assert optim.REGISTRY["SGD"] is torch.optim.SGD           # which class the reference's name resolves to is existing behaviour


def test_sgd_entry_point_is_declared_and_bound():
    from mcquic_amd import _lib
    header = open(os.path.join(ROOT, "include", "mcquic_hip.h")).read()
    assert re.search(r"\bint\s+mcq_sgd_step_f32\s*\(", header)
    assert "mcq_sgd_step_f32" in _lib.SYMBOLS
    assert "sgd.hip" in __import__("mcquic_amd.build", fromlist=["SOURCES"]).SOURCES


def test_sgd_entry_point_checks_its_arguments():
    """Every refusal below happens on the host, before any launch: fake non-NULL addresses are never dereferenced."""
    from mcquic_amd import _lib
    lib = _lib.load()
    ok = 64

    def call(tables=ok, ntensors=1, nblocks=1, step=ok, lr=1e-3, momentum=0.0, dampening=0.0, wd=0.0, nesterov=0, partials=None, nparts=0,
             bound=None, gnorm=None, skip=0, skipped=None, scalars=ok):
        return lib.mcq_sgd_step_f32(tables, ntensors, ok, ok, ok, nblocks, step, None, lr, momentum, dampening, wd, nesterov, 0, partials, nparts,
                                    bound, gnorm, skip, skipped, scalars, None)
    for kw in (dict(tables=None), dict(ntensors=0), dict(nblocks=0), dict(step=None), dict(scalars=None), dict(lr=-1.0), dict(lr=float("nan")),
               dict(momentum=-0.5), dict(wd=-1.0), dict(dampening=float("nan")), dict(nesterov=1), dict(nesterov=1, momentum=0.9, dampening=0.1),
               dict(bound=ok), dict(skip=1), dict(skipped=ok),                           # clipping and the guard need the partials
               dict(partials=ok, nparts=0, gnorm=ok), dict(partials=ok, nparts=1)):      # ... and the partials a count and the norm's slot
        assert call(**kw) == _lib.MCQ_EINVAL, kw


def test_sgd_checkpoints_have_torch_sgd_layout():
    """No device is needed for the layout: a torch.optim.SGD checkpoint loads (its buffer means "not the first update"), comes back
    as `momentum_buffer` alone, and torch.optim.SGD loads and steps from what we save; unsupported modes are refused."""
    from mcquic_amd import optim
    theirs = [torch.nn.Parameter(torch.ones(4)), torch.nn.Parameter(torch.ones(3))]
    ot = torch.optim.SGD(theirs, lr=0.1, momentum=0.9, dampening=0.1, weight_decay=1e-2)
    for p in theirs:
        p.grad = torch.full_like(p, 0.5)
    ot.step()
    ours = [torch.nn.Parameter(p.detach().clone()) for p in theirs]
    oo = optim.SGD(ours, lr=0.3)
    assert oo.state_dict()["state"] == {}
    oo.load_state_dict(copy.deepcopy(ot.state_dict()))
    g = oo.param_groups[0]
    assert (g["lr"], g["momentum"], g["dampening"], g["weight_decay"]) == (0.1, 0.9, 0.1, 1e-2)
    assert all(float(oo.state[p]["step"]) == 1.0 for p in ours)
    sd = oo.state_dict()
    assert sorted(sd["state"]) == [0, 1] and all(list(st) == ["momentum_buffer"] for st in sd["state"].values())
    assert all(torch.equal(sd["state"][i]["momentum_buffer"], ot.state[p]["momentum_buffer"]) for i, p in enumerate(theirs))
    back = torch.optim.SGD([torch.nn.Parameter(p.detach().clone()) for p in theirs], lr=0.3)
    back.load_state_dict(copy.deepcopy(sd))
    for p, q in zip(back.param_groups[0]["params"], theirs):
        p.grad, q.grad = torch.full_like(p, 0.25), torch.full_like(q, 0.25)
    back.step()
    ot.step()
    assert all(torch.equal(p.detach(), q.detach()) for p, q in zip(back.param_groups[0]["params"], theirs))
    # a checkpoint without buffers (momentum 0, or saved before the first step) starts over
    fresh = optim.SGD(ours, lr=0.1, momentum=0.9)
    fresh.load_state_dict(torch.optim.SGD(theirs, lr=0.1, momentum=0.9).state_dict())
    assert all(float(fresh.state[p]["step"]) == 0.0 for p in ours) and fresh.state_dict()["state"] == {}
    for k in ("foreach", "fused", "differentiable"):
        bad = copy.deepcopy(ot.state_dict())
        bad["param_groups"][0][k] = True
        with pytest.raises(NotImplementedError, match=k):
            optim.SGD(ours, lr=0.1).load_state_dict(bad)
