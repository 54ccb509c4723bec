"""GPU: the step guard (csrc/step_guard.hip, mcquic_amd.guard) and the `skip` argument of every update kernel, leaf by leaf.

Tensor tables whose sizes sit on the table's seams -- the chunk size is read from the library (`mcq_adam_chunk()`, which returns
tensor_list.h's MCQ_LIST_CHUNK; tests/test_step_guard_host.py holds the two together): numel 1, chunk - 1, chunk, chunk + 1, two chunks + 1,
and a second parameter group.  One bad element at a time (NaN, +inf, -inf) at the first element of the first tensor, the last element of
the last tensor, either side of a chunk seam, inside the numel-1 tensor and inside the second group only.  A skipped call must leave
EVERYTHING bit for bit (compared as raw words: NaN-safe) and count once; a clean call with the guard on must be the guard-off twin bit for
bit; `grad_norm` against the float64 restatement (tests/_guard_ref.py) under the bar the SGD and LAMB norm tests use (1e-6 relative: the
same arithmetic -- double partials per chunk, a fixed tree, one rounding to float32)."""
import copy
import math

import numpy as np
import pytest
import torch

import _guard_ref as R

pytestmark = pytest.mark.gpu
NORM_BAR = 1e-6                                               # tests/test_gpu_sgd.py::test_sgd_clips_like_clip_grad_norm
BAD = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}
PLACES = ["first-of-first", "last-of-last", "seam-before", "seam-after", "second-seam", "numel-1", "second-group-only"]
KS = [(2, 8), (1, 5)]                                         # (m, k) of two frequency-EMA levels


def _chunk():
    from mcquic_amd import _lib
    return int(_lib.load().mcq_adam_chunk())


def _sizes():
    c = _chunk()
    return [1, c - 1, c, c + 1, 2 * c + 1], [3, c + 5]        # group A (index 0 is the numel-1 tensor), group B


def _places():
    """name -> (group, tensor, element) of the one bad element."""
    c = _chunk()
    return {"first-of-first": (0, 0, 0), "last-of-last": (1, 1, c + 4), "seam-before": (0, 4, c - 1), "seam-after": (0, 4, c),
            "second-seam": (0, 4, 2 * c), "numel-1": (0, 0, 0), "second-group-only": (1, 0, 1)}


def _bits(t):
    return t.detach().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach()


def _same(a, b):
    a, b = list(a), list(b)
    return len(a) == len(b) and all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _params(dev, seed=0):
    """Two parameter groups with gradients; values of order 1."""
    g = torch.Generator().manual_seed(seed)
    groups = [[torch.nn.Parameter(torch.randn(n, generator=g).to(dev)) for n in sizes] for sizes in _sizes()]
    for ps in groups:
        for p in ps:
            p.grad = (0.1 * torch.randn(p.numel(), generator=g)).to(dev)
    return groups


def _optimizer(kind, groups, **kw):
    from mcquic_amd import optim
    spec = [dict(params=groups[0]), dict(params=groups[1])]
    if kind == "adam":
        return optim.Adam(spec, lr=1e-2, weight_decay=1e-2, **kw)
    if kind == "adamw":
        return optim.AdamW(spec, lr=1e-2, **kw)
    if kind == "lamb":
        return optim.Lamb(spec, lr=1e-2, **kw)
    return optim.SGD(spec, lr=1e-2, momentum=0.9, **kw)


def _opt_state(opt):
    out = [p for g in opt.param_groups for p in g["params"]]
    for g in opt.param_groups:
        for p in g["params"]:
            out += [v for _, v in sorted(opt.state[p].items()) if torch.is_tensor(v)]
    if hasattr(opt, "_plans"):
        out += [plan.step for plan in opt._plans.values()]
    return out


class World:
    """Everything the update owns, around one optimizer: parameters + state, an EMA, a scheduler, two frequency-EMA levels."""

    def __init__(self, dev, kind, own: bool, attached: bool):
        from mcquic_amd import guard, optim, schedule
        self.groups = _params(dev)
        self.all = [p for ps in self.groups for p in ps]
        self.opt = _optimizer(kind, self.groups, **({"skip_nonfinite": True} if own else {}))
        self.guard = guard.StepGuard(dev) if attached else None
        if attached:
            self.opt.attach_guard(self.guard)
        self.ema = optim.EMA(self.all, decay=0.9)
        self.sched = schedule.CosineAnnealingWarmupRestarts(self.opt, 6, warmup_steps=2)
        g = torch.Generator().manual_seed(5)
        self.freqs = [torch.rand(m, k, generator=g).to(dev) for m, k in KS]
        self.counts = torch.cat([torch.randint(1, 9, (m * k,), generator=g) for m, k in KS]).to(dev)

    def step(self):
        from mcquic_amd import ops
        self.opt.step()
        flag = None if self.guard is None else self.guard.skip
        self.ema.update(skip=flag)
        ops.freq_ema_update_(self.freqs, self.counts, 0.9, skip=flag)
        self.sched.step(skip=flag)

    def state(self):
        return _opt_state(self.opt) + list(self.ema.averages) + [self.ema._count] + self.freqs + [self.sched._buf] + list(self.sched._lrs)

    def snapshot(self):
        return [t.detach().clone() for t in self.state()]

    def poison(self, place, value):
        gi, ti, ei = place
        self.groups[gi][ti].grad[ei] = value

    def norm(self):
        if self.guard is not None:
            return float(self.guard.grad_norm)
        return float(self.opt._guard.grad_norm if self.opt._guard is not None else self.opt.grad_norm())

    def skipped(self):
        return int(self.guard.skipped) if self.guard is not None else int(self.opt.skipped)


@pytest.mark.parametrize("value", sorted(BAD))
@pytest.mark.parametrize("place", PLACES)
def test_one_bad_element_skips_everything(dev, place, value):
    """All of Adam, AdamW, Lamb, SGD (each under an attached guard -- the tensor-table reduction, or for Lamb its own partials -- and
    under its own `skip_nonfinite`), with the EMA, the scheduler and the frequency EMA behind the attached guard's flag."""
    where = _places()[place]
    for kind in ("adam", "adamw", "lamb", "sgd"):
        for own in (False, True):
            w = World(dev, kind, own=own, attached=not own)
            w.step()                                          # a clean step first: moments, counts and the schedule are under way
            assert w.skipped() == 0
            moved = w.snapshot()
            w.poison(where, BAD[value])
            grads = [p.grad.clone() for p in w.all]
            before = w.snapshot()
            if own:
                w.opt.step()                                  # (the rest of the world has no flag to obey here)
                assert _same(_opt_state(w.opt), before[: len(_opt_state(w.opt))]), (kind, "own", place, value)
            else:
                w.step()
                assert _same(w.state(), before), (kind, "attached", place, value)
                assert int(w.guard.skip) == 1 and int(w.guard.consecutive) == 1
                assert not math.isfinite(float(w.guard.grad_norm))
            assert w.skipped() == 1, (kind, own, place, value)
            assert _same([p.grad for p in w.all], grads), "the gradients are only read"
            assert len(moved) == len(before)
    # the counters over a run: bad, bad, clean, bad (the reference: tests/_guard_ref.py)
    from mcquic_amd import guard
    w = World(dev, "adam", own=False, attached=True)
    clean = [p.grad.clone() for p in w.all]
    seq = []
    for bad in (True, True, False, True):
        for p, g in zip(w.all, clean):
            p.grad.copy_(g)
        if bad:
            w.poison(where, BAD[value])
        seq.append([p.grad.cpu().numpy() for p in w.all])
        w.opt.step()
        rec = R.run(seq)[-1]
        assert (int(w.guard.skip), int(w.guard.skipped), int(w.guard.consecutive)) == (rec["skip"], rec["skipped"], rec["consecutive"])
    with pytest.raises(RuntimeError, match="Loss becomes NAN. Train crashed."):
        w.guard.check(max_consecutive=1)
    w.guard.check(max_consecutive=2)                          # one in a row: below the limit
    assert isinstance(w.guard, guard.StepGuard)


@pytest.mark.parametrize("kind", ["adam", "adamw", "lamb", "sgd"])
def test_finite_gradients_equal_the_guard_off_twin(dev, kind):
    """Three clean steps: attached guard, own guard and no guard produce the same bits everywhere, nothing is skipped, and the norm is the
    float64 reference's under the bar."""
    plain, attached, own = World(dev, kind, False, False), World(dev, kind, False, True), World(dev, kind, True, False)
    for it in range(3):
        for w in (plain, attached, own):
            for p in w.all:
                p.grad.mul_(1.5)
            w.step()
        assert _same(attached.state(), plain.state()), (kind, it)
        assert _same(_opt_state(own.opt), _opt_state(plain.opt)), (kind, it)
        want = R.norm([p.grad.cpu().numpy() for p in plain.all])
        for w in (attached, own):
            got = w.norm()
            print(f"{kind} step {it}: grad_norm {got!r}, float64 reference {want!r}, relative error {abs(got - want) / want:.3e}")
            assert abs(got - want) <= NORM_BAR * want
    assert attached.skipped() == 0 and own.skipped() == 0 and int(attached.guard.consecutive) == 0


def test_huge_finite_gradient_is_not_an_overflow(dev):
    """Elements of 1e19: their float32 squares are inf, their float64 sum of squares is not.  The guard must NOT skip (table form, flat
    form, and through Adam and SGD, whose updates are the guard-off twins' bit for bit)."""
    from mcquic_amd import guard
    c = _chunk()
    for kind in ("adam", "sgd"):
        plain, attached = World(dev, kind, False, False), World(dev, kind, False, True)
        for w in (plain, attached):
            w.groups[0][3].grad.fill_(1e19)
            w.groups[1][0].grad.fill_(-1e19)
            w.step()
        assert int(attached.guard.skip) == 0 and attached.skipped() == 0
        assert _same(attached.state(), plain.state())
        want = R.norm([p.grad.cpu().numpy() for p in plain.all])
        got = float(attached.guard.grad_norm)
        print(f"1e19 ({kind}): grad_norm {got!r}, float64 reference {want!r}")
        assert math.isfinite(want) and abs(got - want) <= NORM_BAR * want
    flat = torch.full((2 * c + 1,), 1e19, device=dev)
    g = guard.StepGuard(dev).run_flat(flat)
    assert int(g.skip) == 0 and abs(float(g.grad_norm) - 1e19 * math.sqrt(2 * c + 1)) <= NORM_BAR * 1e19 * math.sqrt(2 * c + 1)
    assert float((flat * flat).sum()) == float("inf"), "a float32 sum of squares does overflow here"


@pytest.mark.parametrize("n", [1, 4095, 4096, 4097, 8193])
def test_flat_form_and_borrowed_norm_agree(dev, n):
    """Own reduction over a flat buffer, the partials form, and the borrowed forms (a float32 norm; the clip's float32 sum of squares) give
    the same flag for a clean buffer and for each bad value at the first, the last and (where there is one) a seam element; equal inputs
    give equal bits; and a guarded clip applies the factor exactly when the flag is clear."""
    from mcquic_amd import guard, ops
    c = _chunk()
    base = torch.randn(n, generator=torch.Generator().manual_seed(n)).to(dev)
    cases = [(None, None)] + [(i, v) for i in sorted({0, n - 1, min(c, n - 1), min(c - 1, n - 1)}) for v in BAD.values()]
    for idx, v in cases:
        x = base.clone()
        if idx is not None:
            x[idx] = v
        want = R.step(R.fresh(), [x.cpu().numpy()])
        own, again, lent, lent_sq, parts = (guard.StepGuard(dev) for _ in range(5))
        own.run_flat(x)
        again.run_flat(x.clone())
        assert torch.equal(own.record, again.record), "equal inputs, equal bits"
        parts.from_partials(own._partials, int(-(-n // c)))
        assert torch.equal(parts.record, own.record)
        lent.from_norm(own.grad_norm.clone())
        sq = ops.sumsq(x)
        lent_sq.from_norm(sq, squared=True)
        for g in (own, lent, lent_sq):
            assert (int(g.skip), int(g.skipped), int(g.consecutive)) == (want["skip"], want["skipped"], want["consecutive"]), (idx, v)
        if want["skip"] == 0:
            G = float(want["grad_norm"])
            assert abs(float(own.grad_norm) - G) <= NORM_BAR * G and abs(float(lent_sq.grad_norm) - G) <= NORM_BAR * G
        y, z = x.clone(), x.clone()
        ops.clip_by_norm_(y, 0.5)                             # the unguarded clip
        norm = ops.clip_by_norm_(z, 0.5, sq=sq, skip=lent_sq.skip)
        assert _same([z], [x if want["skip"] else y]), "the factor of a skipped step is never applied; a clean one is the plain clip"
        assert torch.equal(_bits(norm), _bits(lent_sq.grad_norm))


def test_guard_state_round_trip_and_argument_checks(dev):
    from mcquic_amd import guard, ops
    g = guard.StepGuard(dev).run_flat(torch.full((3,), float("nan"), device=dev))
    h = guard.StepGuard(dev)
    h.load_state_dict(copy.deepcopy(g.state_dict()))
    assert torch.equal(h.record, g.record) and int(h.skipped) == 1
    with pytest.raises(TypeError):
        g.run_flat(torch.zeros(3, dtype=torch.float64, device=dev))
    with pytest.raises(TypeError):
        g.from_norm(torch.zeros(2, device=dev))
    with pytest.raises(TypeError):
        g.from_partials(torch.zeros(2, device=dev), 1)
    with pytest.raises(ValueError):
        g.check(max_consecutive=0)
    with pytest.raises(TypeError, match="one int32"):
        ops.freq_ema_update_([torch.rand(1, 4, device=dev)], torch.ones(4, dtype=torch.int64, device=dev), 0.9, skip=torch.zeros((), device=dev))
    assert np.isnan(float(g.grad_norm))
