"""mcquic_amd.optim.Lamb (csrc/lamb.hip: the whole model in five launches, trust ratios on the device) against its specification
restated with torch operations (tests/_lamb_ref.py) in float32 on the device and in float64 on the CPU: every mode, clipping on and
off, determinism, a captured update with a device learning rate, two param groups under one gradient norm, checkpoints (our own
layout and apex's), and the update captured inside parallel.GraphedTrainStep."""
import copy
import itertools

import pytest
import torch

from _lamb_ref import RefLamb
from _record import record

pytestmark = pytest.mark.gpu
# one element; no multiple of 4; around the 4096-element chunk; several chunks and a ragged tail; 36 full chunks; two full chunks; odd
# sizes; [9] starts as all zeros (||p|| = 0); [10] has a zero gradient at every step (||u|| = 0 without decay); [11] is, on the device, a
# view starting 4 bytes past a 16-byte boundary
SHAPES = [(1,), (3,), (4095,), (4096,), (4097,), (3 * 4096 + 5,), (128, 128, 3, 3), (2, 64, 64), (5, 7, 11), (300,), (257,), (1029,)]
ZERO_PARAM, ZERO_GRAD, VIEW = 9, 10, 11


def _params(dev, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    vals = [torch.randn(s, generator=g) for s in SHAPES]
    vals[ZERO_PARAM].zero_()
    out = [torch.nn.Parameter(v.to(dev, dtype)) for v in vals]
    if dtype == torch.float32 and out[VIEW].is_cuda:
        base = torch.zeros(vals[VIEW].numel() + 8, device=dev)
        t = base[1: 1 + vals[VIEW].numel()]
        t.copy_(vals[VIEW])
        assert t.data_ptr() % 16 == 4 and t.is_contiguous()
        out[VIEW] = torch.nn.Parameter(t)
    return out


def _fresh_grads(seed):
    g = torch.Generator().manual_seed(seed)
    vals = [torch.randn(s, generator=g) * 0.1 for s in SHAPES]
    vals[ZERO_GRAD].zero_()
    return vals


def _grads(params, seed):
    for p, v in zip(params, _fresh_grads(seed)):
        p.grad = v.to(p.device, p.dtype)


def _within_bar(ours, f32, f64, tag, oo=None, o32=None):
    """The bar of test_adam_matches_torch: per tensor within 2e-6 max|p| of the float32 restatement, or no further from the float64
    truth than 3x the restatement's own distance + 1e-7 max|p|; the moments 2e-6 / 4e-6, loosened 20x where only the second holds."""
    for i, (a, b, t) in enumerate(zip(ours, f32, f64)):
        a, b, t = a.detach(), b.detach(), t.detach()
        scale = max(float(b.abs().max()), 1e-12)
        d32 = float((a - b).abs().max())
        e_ours = float((a.double().cpu() - t.cpu()).abs().max())
        e_ref = float((b.double().cpu() - t.cpu()).abs().max())
        print(f"{tag} {SHAPES[i]}: |ours - f32| {d32 / scale:.3e}  |ours - f64| {e_ours / scale:.3e}  |f32 - f64| {e_ref / scale:.3e}")
        assert d32 <= 2e-6 * scale or e_ours <= 3 * e_ref + 1e-7 * scale, (tag, SHAPES[i], d32 / scale, e_ours / scale, e_ref / scale)
        if oo is not None:
            loose = 1.0 if d32 <= 2e-6 * scale else 20.0
            for name, tol in (("exp_avg", 2e-6), ("exp_avg_sq", 4e-6)):
                x, y = oo.state[ours[i]][name], o32.state[f32[i]][name]
                s = max(float(y.abs().max()), 1e-12)
                err = float((x - y).abs().max())
                assert err <= tol * loose * s, (tag, SHAPES[i], name, err / s)


def _diagnostic(ours, f32, f64, key):
    """1e-6 relative to the float64 value -- or, where float32 arithmetic itself does not get that close, 3x the float32
    restatement's own distance from float64 (recorded); non-finite values (a zero norm) must be the same ones."""
    ours, f32, f64 = ours.double().cpu().reshape(-1), f32.double().cpu().reshape(-1), f64.double().cpu().reshape(-1)
    fin = torch.isfinite(f64)
    assert torch.equal(torch.isfinite(ours), fin) and torch.equal(torch.nan_to_num(ours[~fin], nan=-1.0), torch.nan_to_num(f64[~fin], nan=-1.0)), key
    rel = (ours[fin] - f64[fin]).abs() / f64[fin].abs().clamp_min(1e-300)
    rel32 = (f32[fin] - f64[fin]).abs() / f64[fin].abs().clamp_min(1e-300)
    print(f"{key}: ours {float(rel.max()):.3e}, float32 restatement {float(rel32.max()):.3e}")
    if bool((rel > 1e-6).any()):
        record(key, value=float(rel.max()), restatement=float(rel32.max()), bar="max(1e-6, 3 x restatement), per entry")
    assert bool((rel <= torch.maximum(torch.full_like(rel, 1e-6), 3 * rel32)).all()), (key, float(rel.max()), float(rel32.max()))


MODES = [dict(adam_w_mode=a, weight_decay=w, use_nvlamb=n) for a, w, n in itertools.product([True, False], [0.0, 0.01], [False, True])]
MODES += [dict(bias_correction=False), dict(grad_averaging=False), dict(betas=(0.8, 0.95), eps=1e-8)]


@pytest.mark.parametrize("max_grad_norm", [1.0, 1e6])
@pytest.mark.parametrize("kw", MODES, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_lamb_matches_the_specification(dev, kw, max_grad_norm):
    from mcquic_amd import optim
    ours, f32, f64 = _params(dev, 1), _params(dev, 1), _params("cpu", 1, torch.float64)
    oo = optim.Lamb(ours, lr=3e-3, max_grad_norm=max_grad_norm, **kw)
    o32, o64 = RefLamb(f32, lr=3e-3, max_grad_norm=max_grad_norm, **kw), RefLamb(f64, lr=3e-3, max_grad_norm=max_grad_norm, **kw)
    tag = f"lamb[{kw}, max_grad_norm={max_grad_norm}]"
    for it in range(6):
        for ps in (ours, f32, f64):
            _grads(ps, 10 + it)
        oo.step()
        o32.step()
        o64.step()
        if it in (0, 5):
            _diagnostic(oo.grad_norm, o32.grad_norm, o64.grad_norm, f"{tag} step {it} grad_norm")
            _diagnostic(oo.trust_ratios(), torch.stack(o32.ratios[0]), torch.stack(o64.ratios[0]), f"{tag} step {it} trust_ratios")
    G = float(oo.grad_norm)
    assert G > 1.0                                            # (0.1 randn over 1.9e5 elements: about 43)
    assert (G > max_grad_norm) == (max_grad_norm == 1.0)      # clipping engages in one run of the set and not in the other
    _within_bar(ours, f32, f64, tag, oo, o32)
    for p in ours:
        assert float(oo.state[p]["step"]) == 6.0


def test_lamb_is_deterministic(dev):
    from mcquic_amd import optim
    a, b = _params(dev, 2), _params(dev, 2)
    oa, ob = optim.Lamb(a, lr=3e-3), optim.Lamb(b, lr=3e-3)
    for it in range(3):
        _grads(a, 30 + it)
        _grads(b, 30 + it)
        oa.step()
        ob.step()
    assert torch.equal(oa.grad_norm, ob.grad_norm) and torch.equal(oa.trust_ratios(), ob.trust_ratios())
    for p, q in zip(a, b):
        assert torch.equal(p.detach(), q.detach())
        assert torch.equal(oa.state[p]["exp_avg"], ob.state[q]["exp_avg"]) and torch.equal(oa.state[p]["exp_avg_sq"], ob.state[q]["exp_avg_sq"])


def test_lamb_device_learning_rate_and_capture(dev):
    """test_adam_device_learning_rate_and_capture for Lamb: the rate is a device tensor refilled between replays; a replayed step is
    the same bits as that step run eagerly by a twin; the gradients are only read."""
    from mcquic_amd import optim
    ours, twin, f32, f64 = _params(dev, 3), _params(dev, 3), _params(dev, 3), _params("cpu", 3, torch.float64)
    lr_o, lr_w = torch.tensor(0.0, device=dev), torch.tensor(0.0, device=dev)
    oo, ow = optim.Lamb(ours, lr=lr_o), optim.Lamb(twin, lr=lr_w)
    o32, o64 = RefLamb(f32, lr=0.0), RefLamb(f64, lr=0.0)
    for ps in (ours, twin, f32, f64):
        _grads(ps, 5)
    oo.prepare()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lr_o.fill_(1e-3)
        oo.step()                                              # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    lr_w.fill_(1e-3)
    ow.step()
    for o in (o32, o64):
        o.param_groups[0]["lr"] = 1e-3
        o.step()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        oo.step()
    for it in range(4):
        rate = 1e-3 * (it + 2)
        lr_o.fill_(rate)
        lr_w.fill_(rate)
        o32.param_groups[0]["lr"] = o64.param_groups[0]["lr"] = rate
        fresh = _fresh_grads(50 + it)
        for ps in (ours, twin, f32, f64):
            for p, v in zip(ps, fresh):
                p.grad.copy_(v)                                # (same addresses: the graph reads them)
        graph.replay()
        ow.step()
        o32.step()
        o64.step()
        for p, q, v in zip(ours, twin, fresh):
            assert torch.equal(p.detach(), q.detach()), "a replayed step differs from the same step run eagerly"
            assert torch.equal(p.grad, v.to(dev)), "step() changed a gradient"
    _within_bar(ours, f32, f64, "captured update with a scheduled rate")
    assert float(oo.state[ours[0]]["step"]) == 5.0
    # a changed gradient address inside a capture is refused, not silently captured as a host copy
    ours[0].grad = ours[0].grad.clone()
    g2 = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError):
        with torch.cuda.graph(g2):
            oo.step()


def test_lamb_two_param_groups_share_one_gradient_norm(dev):
    from mcquic_amd import optim
    ours, f32, f64 = _params(dev, 4), _params(dev, 4), _params("cpu", 4, torch.float64)

    def groups(ps):
        return [dict(params=ps[:5], weight_decay=0.0), dict(params=ps[5:], weight_decay=0.01)]
    oo = optim.Lamb(groups(ours), lr=3e-3, max_grad_norm=1.0)
    o32, o64 = RefLamb(groups(f32), lr=3e-3, max_grad_norm=1.0), RefLamb(groups(f64), lr=3e-3, max_grad_norm=1.0)
    for it in range(4):
        for ps in (ours, f32, f64):
            _grads(ps, 40 + it)
        oo.step()
        o32.step()
        o64.step()
    _diagnostic(oo.grad_norm, o32.grad_norm, o64.grad_norm, "two groups grad_norm")
    for gi in (0, 1):
        _diagnostic(oo.trust_ratios(gi), torch.stack(o32.ratios[gi]), torch.stack(o64.ratios[gi]), f"two groups trust_ratios[{gi}]")
    _within_bar(ours, f32, f64, "two groups", oo, o32)


def test_lamb_checkpoints(dev):
    from mcquic_amd import optim
    a, f32, f64 = _params(dev, 6), _params(dev, 6), _params("cpu", 6, torch.float64)
    oa, o32, o64 = optim.Lamb(a, lr=3e-3), RefLamb(f32, lr=3e-3), RefLamb(f64, lr=3e-3)
    for it in range(3):
        for ps in (a, f32, f64):
            _grads(ps, 60 + it)
        oa.step()
        o32.step()
        o64.step()
    sd = copy.deepcopy(oa.state_dict())
    assert all(float(st["step"]) == 3.0 for st in sd["state"].values())
    assert len({st["step"].data_ptr() for st in sd["state"].values()}) == len(SHAPES), "every parameter gets a step of its own"
    # our own layout into a fresh optimizer on copied parameters: the runs continue as one, and the flat buffers stay where they are
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    ob = optim.Lamb(b, lr=3e-3)
    _grads(b, 0)
    ob.prepare()
    addr = [ob._plans[0].flat_m.data_ptr(), ob._plans[0].flat_v.data_ptr(), ob._plans[0].step.data_ptr()]
    ob.load_state_dict(sd)
    # apex's layout, made by hand from the restatement's moments: an integer `step` in the group, none per parameter
    c = [torch.nn.Parameter(p.detach().clone()) for p in f32]
    oc = optim.Lamb(c, lr=3e-3)
    apex = {"state": {i: {"exp_avg": o32.state[p]["exp_avg"].clone(), "exp_avg_sq": o32.state[p]["exp_avg_sq"].clone()} for i, p in enumerate(f32)},
            "param_groups": [dict(lr=3e-3, bias_correction=True, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, grad_averaging=True,
                                  max_grad_norm=1.0, step=3, params=list(range(len(f32))))]}
    oc.load_state_dict(apex)
    assert apex["param_groups"][0]["step"] == 3 and "step" not in apex["state"][0], "the caller's dict is left as it was"
    for it in range(3, 6):
        for ps in (a, b, c, f32, f64):
            _grads(ps, 60 + it)
        for o in (oa, ob, oc, o32, o64):
            o.step()
    assert addr == [ob._plans[0].flat_m.data_ptr(), ob._plans[0].flat_v.data_ptr(), ob._plans[0].step.data_ptr()]
    for p, q in zip(a, b):
        assert torch.equal(p.detach(), q.detach())
        assert torch.equal(oa.state[p]["exp_avg"], ob.state[q]["exp_avg"]) and torch.equal(oa.state[p]["exp_avg_sq"], ob.state[q]["exp_avg_sq"])
    assert float(oc.state[c[0]]["step"]) == 6.0
    _within_bar(c, f32, f64, "continuing from an apex-layout checkpoint", oc, o32)


def test_graphed_step_with_lamb_equals_eager_restatement(dev):
    from mcquic_amd import Compressor, optim, parallel
    from test_gpu_graphed_step import _uniforms
    ch, ks, hw, n, steps = 32, [64, 32, 16], 64, 2, 4
    torch.manual_seed(21)
    eager = Compressor(ch, 2, ks).to(dev).train()
    graphed = copy.deepcopy(eager)
    xs = [(torch.rand((n, 3, hw, hw), generator=torch.Generator().manual_seed(70 + i)) * 2 - 1).to(dev) for i in range(steps)]
    us = _uniforms(n, hw, ks, dev, 13)
    opt_e = RefLamb(eager.parameters(), lr=1e-3)
    losses_e = []
    for x in xs:
        opt_e.zero_grad(set_to_none=True)
        loss = torch.nn.functional.mse_loss(eager(x, uniforms=us)[0], x)
        loss.backward()
        opt_e.step()
        losses_e.append(float(loss.detach()))
    step = parallel.GraphedTrainStep(graphed, optim.Lamb(graphed.parameters(), lr=1e-3), xs[0], forward_kwargs={"uniforms": us})
    assert step.post is not None, "the update should have been captured"
    losses_g = [float(step(x)) for x in xs]
    step.close()
    for a, b in zip(losses_e, losses_g):
        assert abs(a - b) <= 2e-6 * max(1.0, abs(a)), (losses_e, losses_g)
    for (name, pe), (_, pg) in zip(eager.named_parameters(), graphed.named_parameters()):
        scale = max(float(pe.detach().abs().max()), 1e-12)
        assert float((pe.detach() - pg.detach()).abs().max()) <= 2e-5 * scale, name
