"""mcquic_amd.optim.SGD (csrc/sgd.hip: a parameter group in one launch; clipping and the non-finite guard on the device) against the
float64 restatement of tests/_sgd_ref.py, started from the same float32 values.

The bar (`_bar`): torch.optim.SGD(foreach=True) runs on the device on the same inputs; its worst error against the restatement, relative
to max|x| per tensor, over parameters and momentum buffers, is the measured error of a float32 SGD.  Ours may be 4 x that far from the
restatement (the project's margin over a measured reference error), and never needs to be closer than one float32 ulp of max|x|.

Tensor sizes, with c = mcq_adam_chunk(): 1, 3, 4, 5, c - 1, c, c + 1, 2c + 5 (each chunk edge; 16-byte lanes and the dword tail),
[7, 3, 3, 3], a tensor without elements (it owns no chunk) and a parameter that is a view starting 4 bytes past a 16-byte boundary
(the dword path for a whole tensor)."""
import copy
import math

import pytest
import torch

from _sgd_ref import RefSGD, setting_id, settings

pytestmark = pytest.mark.gpu
VIEW = 10                                                     # index of the misaligned view below
LR = 0.05


def _chunk():
    from mcquic_amd import _lib
    return _lib.load().mcq_adam_chunk()


def _shapes():
    c = _chunk()
    return [(1,), (3,), (4,), (5,), (c - 1,), (c,), (c + 1,), (2 * c + 5,), (7, 3, 3, 3), (0,), (1029,)]


def _values(seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g) * scale for s in _shapes()]


def _params(dev, seed):
    out = []
    for i, v in enumerate(_values(seed)):
        if i == VIEW:
            base = torch.zeros(v.numel() + 8, device=dev)
            t = base[1: 1 + v.numel()]
            t.copy_(v)
            assert t.data_ptr() % 16 == 4 and t.is_contiguous()
            out.append(torch.nn.Parameter(t))
        else:
            out.append(torch.nn.Parameter(v.to(dev)))
    assert out[VIEW].data_ptr() % 16 == 4
    return out


def _grads(params, seed, scale=0.5):
    vals = _values(seed, scale)
    for p, v in zip(params, vals):
        p.grad = v.to(p.device)
    return vals


def _refill(params, vals):
    for p, v in zip(params, vals):
        p.grad.copy_(v)                                       # (same addresses: a captured step reads them)


def _ulp(x: float) -> float:
    return 2.0 ** (math.floor(math.log2(x)) - 23) if x > 0 else 0.0


def _rel_err(got, want):
    """Worst |got - want| / max|want| over the tensors that have elements."""
    worst = 0.0
    for a, t in zip(got, want):
        if t.numel():
            worst = max(worst, float((a.detach().double().cpu() - t).abs().max()) / max(float(t.abs().max()), 1e-300))
    return worst


def _bar(tag, ours, theirs, want):
    """`ours` / `theirs` / `want`: lists of tensors (parameters, then momentum buffers) of optim.SGD, of torch's foreach SGD on the device and
    of the restatement.  Prints both measured errors; ours within max(4 x torch's worst, one float32 ulp of max|x|) per tensor."""
    e_torch, e_ours = _rel_err(theirs, want), _rel_err(ours, want)
    print(f"{tag}: worst error relative to max|x| -- torch foreach {e_torch:.3e}, ours {e_ours:.3e}")
    for i, (a, t) in enumerate(zip(ours, want)):
        if t.numel():
            top = float(t.abs().max())
            err = float((a.detach().double().cpu() - t).abs().max())
            assert err <= max(4.0 * e_torch * top, _ulp(top)), (tag, i, tuple(t.shape), err / top, e_torch)
    return e_torch, e_ours


def _bufs(opt, params):
    return [opt.state[p]["momentum_buffer"] for p in params if "momentum_buffer" in opt.state[p]]


def _run(dev, kw, steps=3, seed=1, max_grad_norm=None):
    """(ours, optimizer, torch's, its optimizer, restatement) after `steps` updates from equal values with equal gradients."""
    from mcquic_amd import optim
    ours, theirs = _params(dev, seed), _params(dev, seed)
    f64 = [p.detach().double().cpu() for p in ours]
    oo = optim.SGD(ours, lr=LR, max_grad_norm=max_grad_norm, **kw)
    ot = torch.optim.SGD(theirs, lr=LR, foreach=True, **kw)
    ref = RefSGD(f64, lr=LR, max_grad_norm=max_grad_norm, **kw)
    for it in range(steps):
        vals = _grads(ours, 10 * seed + it)
        _grads(theirs, 10 * seed + it)
        if max_grad_norm is not None:
            torch.nn.utils.clip_grad_norm_(theirs, max_grad_norm)
        oo.step()
        ot.step()
        ref.update(vals)
        assert all(torch.equal(p.grad.cpu(), v) for p, v in zip(ours, vals)), "step() changed a gradient"
    return ours, oo, theirs, ot, ref


@pytest.mark.parametrize("kw", settings(), ids=setting_id)
def test_sgd_matches_the_restatement(dev, kw):
    ours, oo, theirs, ot, ref = _run(dev, kw)
    has_buf = kw["momentum"] != 0.0
    want = ref.params + ([b for b in ref.bufs] if has_buf else [])
    _bar(f"sgd[{setting_id(kw)}]", [p for p in ours] + _bufs(oo, ours), [p for p in theirs] + _bufs(ot, theirs), want)
    plan = oo._plans[0]
    c = _chunk()
    assert plan.nblocks == sum(-(-math.prod(s) // c) for s in _shapes()) and plan.ntensors == len(_shapes())
    assert float(plan.step) == 3.0
    assert (plan.flat_m is not None) == has_buf and plan.flat_v is None, "one flat buffer with momentum, none without"
    assert len(_bufs(oo, ours)) == (len(ours) if has_buf else 0)
    sd = oo.state_dict()["state"]
    assert all(list(st) == ["momentum_buffer"] for st in sd.values()) and len(sd) == (len(ours) if has_buf else 0)


def _same_bits(a, oa, b, ob):
    for p, q in zip(a, b):
        assert torch.equal(p.detach(), q.detach())
    for x, y in zip(_bufs(oa, a), _bufs(ob, b)):
        assert torch.equal(x, y)


def test_sgd_is_deterministic(dev):
    from mcquic_amd import optim
    kw = dict(momentum=0.9, dampening=0.1, weight_decay=1e-2)
    a, oa, _, _, _ = _run(dev, kw, max_grad_norm=0.5)
    b, ob, _, _, _ = _run(dev, kw, max_grad_norm=0.5)
    _same_bits(a, oa, b, ob)
    assert torch.equal(oa.grad_norm(), ob.grad_norm()) and float(oa.grad_norm()) > 0.5
    # a model of 640 small tensors: one launch, the same bits twice
    def model(seed):
        g = torch.Generator().manual_seed(seed)
        return [torch.randn(1 + (7 * i) % 301, generator=g) for i in range(640)]
    runs = []
    for _ in range(2):
        ps = [torch.nn.Parameter(v.to(dev)) for v in model(5)]
        opt = optim.SGD(ps, lr=LR, momentum=0.9, nesterov=True, max_grad_norm=1.0, skip_nonfinite=True)
        for it in range(3):
            for p, v in zip(ps, model(50 + it)):
                p.grad = v.to(dev)
            opt.step()
        assert opt._plans[0].ntensors == 640 and int(opt.skipped) == 0
        runs.append((ps, opt))
    _same_bits(runs[0][0], runs[0][1], runs[1][0], runs[1][1])
    assert torch.equal(runs[0][1].grad_norm(), runs[1][1].grad_norm())
    assert not torch.equal(runs[0][0][0].detach().cpu(), model(5)[0])


def test_sgd_device_learning_rate(dev):
    """A rate given as a device tensor is read on every call: refilled between two calls, the run is the bits of a twin whose host rate
    was changed the same way, and not those of a run that kept the first rate."""
    from mcquic_amd import optim
    a, b, c = _params(dev, 2), _params(dev, 2), _params(dev, 2)
    lr = torch.tensor(0.05, device=dev)
    oa, ob, oc = optim.SGD(a, lr=lr, momentum=0.9), optim.SGD(b, lr=0.05, momentum=0.9), optim.SGD(c, lr=0.05, momentum=0.9)
    for it, rate in enumerate((0.05, 0.02)):
        lr.fill_(rate)
        ob.param_groups[0]["lr"] = rate
        for ps in (a, b, c):
            _grads(ps, 20 + it)
        for o in (oa, ob, oc):
            o.step()
    _same_bits(a, oa, b, ob)
    assert not torch.equal(a[5].detach(), c[5].detach())
    d = _params(dev, 2)
    _grads(d, 20)
    with pytest.raises(TypeError):
        optim.SGD(d, lr=torch.tensor(0.05, device=dev, dtype=torch.float64)).step()


def test_sgd_captured_step(dev):
    """`step()` captured after `prepare()`, with clipping and the guard on (three launches): three replays are the bits of three eager
    calls of a twin; a gradient that moved is refused under capture, not silently captured as a host copy."""
    from mcquic_amd import optim
    kw = dict(lr=LR, momentum=0.9, weight_decay=1e-2, max_grad_norm=0.5, skip_nonfinite=True)
    warm = _params(dev, 3)
    _grads(warm, 30)
    optim.SGD(warm, **kw).step()                              # (the kernels' first launch, outside any capture)
    a, b = _params(dev, 3), _params(dev, 3)
    oa, ob = optim.SGD(a, **kw), optim.SGD(b, **kw)
    _grads(a, 30)
    oa.prepare()
    assert float(oa._plans[0].step) == 0.0 and not _bufs(oa, a)[0].any(), "prepare() updates nothing"
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        oa.step()
    for it in range(3):
        vals = _grads(b, 30 + it)
        _refill(a, vals)
        graph.replay()
        ob.step()
        _same_bits(a, oa, b, ob)
        assert torch.equal(oa.grad_norm(), ob.grad_norm())
    assert float(oa._plans[0].step) == 3.0 and int(oa.skipped) == 0
    assert not torch.equal(a[5].detach().cpu(), _values(3)[5])
    a[0].grad = a[0].grad.clone()
    g2 = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError):
        with torch.cuda.graph(g2):
            oa.step()


def _snapshot(params, opt):
    return [p.detach().clone() for p in params] + [b.clone() for b in _bufs(opt, params)] + [opt._plans[0].step.clone()]


def test_sgd_skips_a_nonfinite_gradient(dev):
    """One inf, then one NaN, in the last element of the 2c + 5 tensor (the dword tail of its last chunk): parameters, buffers and the
    step count keep their bits, `skipped` goes 0 -> 1 -> 2, and the next finite step is the one of a run that never saw them."""
    from mcquic_amd import optim
    kw = dict(lr=LR, momentum=0.9, dampening=0.1, weight_decay=1e-2, skip_nonfinite=True)
    for steps_before in (0, 2):                               # (0: the skipped calls come before the FIRST update, which stays the first)
        a, b = _params(dev, 4), _params(dev, 4)
        oa, ob = optim.SGD(a, **kw), optim.SGD(b, **kw)
        for it in range(steps_before):
            _grads(a, 40 + it)
            _grads(b, 40 + it)
            oa.step()
            ob.step()
        _grads(a, 45)
        oa.prepare()
        before = _snapshot(a, oa)
        assert int(oa.skipped) == 0
        for n, bad in enumerate((float("inf"), float("nan"))):
            _grads(a, 45)
            a[7].grad.view(-1)[-1] = bad
            oa.step()
            assert int(oa.skipped) == n + 1 and not math.isfinite(float(oa.grad_norm()))
            now = _snapshot(a, oa)
            assert len(now) == len(before) and all(torch.equal(x, y) for x, y in zip(now, before))
        _grads(a, 46)
        _grads(b, 46)
        oa.step()
        ob.step()
        _same_bits(a, oa, b, ob)
        assert int(oa.skipped) == 2 and int(ob.skipped) == 0 and float(oa._plans[0].step) == steps_before + 1
        assert math.isfinite(float(oa.grad_norm()))


def test_sgd_without_the_guard_updates_like_torch(dev):
    """skip_nonfinite=False and no clipping: the bad value goes through as it does in torch.optim.SGD -- the same element turns
    non-finite, every other one is the plain update.  One update p - lr g from equal floats: each side is within half an ulp of its
    result (plus the rounding of lr g, far below it), so the two differ by at most 2 ulp of max|p|."""
    from mcquic_amd import optim
    for bad in (float("inf"), float("nan")):
        a, b = _params(dev, 6), _params(dev, 6)
        oa, ob = optim.SGD(a, lr=LR, momentum=0.9), torch.optim.SGD(b, lr=LR, momentum=0.9, foreach=True)
        for ps in (a, b):
            _grads(ps, 60)
            ps[7].grad.view(-1)[-1] = bad
        oa.step()
        ob.step()
        assert int(oa.skipped) == 0
        for i, (p, q) in enumerate(zip(a, b)):
            p, q = p.detach(), q.detach()
            fin = torch.isfinite(q)
            assert torch.equal(torch.isfinite(p), fin) and torch.equal(torch.isnan(p), torch.isnan(q)), i
            assert int((~fin).sum()) == (1 if i == 7 else 0)
            if p.numel():
                assert float((p[fin] - q[fin]).abs().max()) <= 2 * _ulp(float(q[fin].abs().max())), i


def test_sgd_clips_like_clip_grad_norm(dev):
    kw = dict(momentum=0.9, dampening=0.1, weight_decay=1e-2)
    ours, oo, theirs, ot, ref = _run(dev, kw, max_grad_norm=0.5)
    G, want = float(oo.grad_norm()), ref.grad_norm
    print(f"grad_norm: ours {G!r}, restatement {want!r}")
    assert want > 0.5 and abs(G - want) <= 1e-6 * want         # (0.5 randn over 2.2e4 elements: about 74; the bound bites)
    _bar("sgd clipped", [p for p in ours] + _bufs(oo, ours), [p for p in theirs] + _bufs(ot, theirs), ref.params + ref.bufs)
    # a bound above the norm: the bits of the optimizer that does not clip
    a, oa, _, _, ra = _run(dev, kw, max_grad_norm=1e4)
    b, ob, _, _, _ = _run(dev, kw)
    assert ra.grad_norm < 1e4 and abs(float(oa.grad_norm()) - ra.grad_norm) <= 1e-6 * ra.grad_norm
    _same_bits(a, oa, b, ob)
    with pytest.raises(RuntimeError):
        ob.grad_norm()


def test_sgd_two_param_groups_share_one_gradient_norm(dev):
    """The norm, the clip factor and the guard span all groups; a skipped call is counted once."""
    from mcquic_amd import optim
    ours = _params(dev, 7)
    f64 = [p.detach().double().cpu() for p in ours]
    oo = optim.SGD([dict(params=ours[:6], momentum=0.0), dict(params=ours[6:], momentum=0.9)], lr=LR, max_grad_norm=0.5, skip_nonfinite=True)
    r0, r1 = RefSGD(f64[:6], lr=LR, momentum=0.0), RefSGD(f64[6:], lr=LR, momentum=0.9)
    for it in range(2):
        vals = _grads(ours, 70 + it)
        oo.step()
        G = math.sqrt(sum(float(v.double().pow(2).sum()) for v in vals))
        assert abs(float(oo.grad_norm()) - G) <= 1e-6 * G
        c = min(1.0, 0.5 / (G + 1e-6))
        r0.update([v.double() * c for v in vals[:6]])
        r1.update([v.double() * c for v in vals[6:]])
    for i, (p, t) in enumerate(zip(ours, f64)):
        if t.numel():                                         # (two updates of float32 SGD: a few ulp of max|p|, 8 with the margin)
            assert float((p.detach().double().cpu() - t).abs().max()) <= 8 * _ulp(float(t.abs().max())), i
    before = [p.detach().clone() for p in ours]
    _grads(ours, 75)
    ours[2].grad[0] = float("nan")                            # in the FIRST group: the second one must not move either
    oo.step()
    assert int(oo.skipped) == 1 and all(torch.equal(p.detach(), q) for p, q in zip(ours, before))
    assert [float(oo._plans[g].step) for g in (0, 1)] == [2.0, 2.0]


def _continue(dev, first_cls, then_cls):
    """2 steps with one optimizer, its state_dict() into the other on the same parameters, 1 more step there."""
    from mcquic_amd import optim
    kw = dict(lr=LR, momentum=0.9, dampening=0.1, weight_decay=1e-2)
    make = {"ours": lambda ps: optim.SGD(ps, **kw), "torch": lambda ps: torch.optim.SGD(ps, **kw)}    # (foreach is torch's default on a device)
    ps = _params(dev, 8)
    f64 = [p.detach().double().cpu() for p in ps]
    ref = RefSGD(f64, **kw)
    opt = make[first_cls](ps)
    for it in range(2):
        ref.update(_grads(ps, 80 + it))
        opt.step()
    sd = copy.deepcopy(opt.state_dict())
    assert all(list(st) == ["momentum_buffer"] for st in sd["state"].values()) and len(sd["state"]) == len(ps)
    nxt = make[then_cls](ps)
    nxt.load_state_dict(sd)
    ref.update(_grads(ps, 82))
    nxt.step()
    return ps, nxt, ref


def test_sgd_checkpoints_exchange_with_torch_sgd(dev):
    """Both directions end within the bar of 3 steps of the restatement -- the third step is NOT a first update (a first update would set
    buf = g: off by the whole 0.9 buf of two steps) -- where the bar's reference error is torch's own 3 straight steps."""
    kw = dict(momentum=0.9, dampening=0.1, weight_decay=1e-2)
    _, _, theirs, ot, ref3 = _run(dev, kw, seed=8)
    straight = [p for p in theirs] + _bufs(ot, theirs)
    for first, then in (("ours", "torch"), ("torch", "ours")):
        ps, opt, ref = _continue(dev, first, then)
        assert all(torch.equal(x, y) for x, y in zip(ref.params + ref.bufs, ref3.params + ref3.bufs))
        _bar(f"sgd checkpoint {first} -> {then}", [p for p in ps] + _bufs(opt, ps), straight, ref.params + ref.bufs)
        if then == "ours":
            assert float(opt._plans[0].step) == 2.0           # (a loaded buffer: "not the first update", then one more)


def test_adam_and_lamb_are_untouched(dev):
    """Adam and Lamb share `_Planned` with SGD: one step of each on tensors an SGD has already updated is the bits of a fresh instance's
    step from the same values, and their state is still two moments and a step count."""
    from mcquic_amd import optim
    ps = _params(dev, 9)
    sgd = optim.SGD(ps, lr=LR, momentum=0.9, max_grad_norm=0.5)
    _grads(ps, 90)
    sgd.step()
    for make in (lambda q: optim.Adam(q, lr=1e-2), lambda q: optim.AdamW(q, lr=1e-2), lambda q: optim.Lamb(q, lr=1e-2)):
        a = [torch.nn.Parameter(p.detach().clone()) for p in ps]
        b = [torch.nn.Parameter(p.detach().clone()) for p in ps]
        oa, ob = make(a), make(b)
        for q in (a, b):
            _grads(q, 91)
        oa.step()
        ob.step()
        for p, q, orig in zip(a, b, ps):
            assert torch.equal(p.detach(), q.detach())
            assert sorted(oa.state[p]) == ["exp_avg", "exp_avg_sq", "step"] and float(oa.state[p]["step"]) == 1.0
            assert torch.equal(oa.state[p]["exp_avg"], ob.state[q]["exp_avg"]) and torch.equal(oa.state[p]["exp_avg_sq"], ob.state[q]["exp_avg_sq"])
            if p.numel():
                assert not torch.equal(p.detach(), orig.detach())
        assert oa._plans[0].flat_m is not None and oa._plans[0].flat_v is not None
