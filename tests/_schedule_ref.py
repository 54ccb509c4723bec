"""The reference's learning-rate schedulers (mcquic/train/lrSchedulers.py) restated as plain float64 Python, one function per
scheduler, each operation in the reference's order: what tests/golden/f19_lr_schedules.npz records, recomputed without torch.  Both are
CPython float64 running the same operations on the same libm, so tests/test_schedule_ref.py compares them exactly.

A case is a dict of the fixture's `cases` list: {"name", "scheduler", "kwargs", "base_lrs", "steps", "last_epoch"}.  `sequence(case)`
returns (rates, epochs): the groups' rates after the constructor and after each of `steps` calls of step(), and last_epoch there."""
import json
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f19_lr_schedules.npz")


def load():
    """(cases, {name: rates [steps + 1, groups]}, {name: epochs [steps + 1]}) of the fixture."""
    z = np.load(GOLDEN)
    cases = json.loads(str(z["cases"]))
    return cases, {c["name"]: z[f"rates_{c['name']}"] for c in cases}, {c["name"]: z[f"epochs_{c['name']}"] for c in cases}


def exact_points(case):
    """Per recorded point: is the rate there an arithmetic-only branch?  Placeholder, MultiStep and Cyclic triangular: all of them;
    Cosine: every warm-up ramp (a later cycle's bounds carry gamma ** cycle: a pow whose exact result is representable)."""
    rates, _ = sequence(case, want_branch=True)
    return rates


def _placeholder(case, want_branch):
    base = list(case["base_lrs"])
    n = case["steps"] + 1
    return [([True] * len(base) if want_branch else list(base)) for _ in range(n)], list(range(n))


def _multistep(case, want_branch):
    kw = case["kwargs"]
    milestones, gamma = set(kw["milestones"]), kw.get("gamma", 0.1)
    first = min(milestones)
    base = list(case["base_lrs"])
    lrs, e = list(base), case["last_epoch"]
    rates, epochs = [], []
    for _ in range(case["steps"] + 1):
        e += 1
        if e <= first:
            lrs = [b * float(e + 1) / first for b in base]
        elif e in milestones:
            lrs = [lr * gamma for lr in lrs]
        rates.append([True] * len(base) if want_branch else list(lrs))
        epochs.append(e)
    return rates, epochs


def _cyclic(case, want_branch):
    kw = case["kwargs"]
    groups = len(case["base_lrs"])
    as_list = lambda v: list(v) if isinstance(v, (list, tuple)) else [v] * groups     # noqa: E731
    base, peak = as_list(kw["base_lr"]), as_list(kw["max_lr"])
    up = float(kw.get("step_size_up", 2000))
    down = float(kw["step_size_down"]) if kw.get("step_size_down") is not None else up
    total = up + down
    ratio = up / total
    mode, gamma = kw.get("mode", "triangular"), kw.get("gamma", 1.)
    e = case["last_epoch"]
    rates, epochs = [], []
    for i in range(case["steps"] + 1):
        e += 1
        cycle = math.floor(1 + e / total)
        x = 1. + e / total - cycle
        scale = x / ratio if x <= ratio else (x - 1) / (ratio - 1)
        row = []
        # (the constructor's step runs on the groups' initial_lr; with last_epoch == -1 that IS base_lr)
        for b, p in zip(case["base_lrs"] if i == 0 else base, peak):
            height = (p - b) * scale
            f = 1. if mode == "triangular" else 1 / (2. ** (cycle - 1)) if mode == "triangular2" else gamma ** e
            row.append(b + height * f)
        rates.append([mode == "triangular"] * groups if want_branch else row)
        epochs.append(e)
    return rates, epochs


def _cosine(case, want_branch):
    kw = case["kwargs"]
    first, mult, ratio = kw["first_cycle_steps"], kw.get("cycle_mult", 1.), kw.get("lrScaleRatio", 0.001)
    warm, gamma = kw.get("warmup_steps", 0), kw.get("gamma", 1.)
    base = list(case["base_lrs"])
    peak = list(base)
    low = [lr * ratio for lr in peak]
    low_base = list(low)
    cur, cycle = first, 0
    k = case["last_epoch"]
    sic = k
    rates, epochs = [], []
    for i in range(case["steps"] + 1):
        if i == 0 and k != -1:                                # step(k): the closed form
            if k >= first:
                if mult == 1.:
                    sic, cycle = k % first, k // first
                else:
                    n = int(math.log((k / first * (mult - 1) + 1), mult))
                    cycle = n
                    sic = k - int(first * (mult ** n - 1) / (mult - 1))
                    cur = first * mult ** (n)
                peak = [lr * (gamma ** cycle) for lr in base]
                low = [lr * (gamma ** cycle) for lr in low_base]
            else:
                cur, sic = first, k
            e = k + 1
        else:                                                 # step(None): the recurrence
            e = (k if i == 0 else e) + 1
            sic = sic + 1
            if sic >= cur:
                cycle += 1
                sic = sic - cur
                cur = int((cur - warm) * mult) + warm
                peak = [lr * (gamma ** cycle) for lr in base]
                low = [lr * (gamma ** cycle) for lr in low_base]
        if sic == -1:
            row, exact = list(low), True
        elif sic < warm:
            row, exact = [(hi - lo) * sic / warm + lo for lo, hi in zip(low, peak)], True
        else:
            row, exact = [lo + (hi - lo) * (1 + math.cos(math.pi * (sic - warm) / (cur - warm))) / 2 for lo, hi in zip(low, peak)], False
        rates.append([exact] * len(base) if want_branch else row)
        epochs.append(e)
    return rates, epochs


_BY_NAME = {"Placeholder": _placeholder, "MultiStepLRWithWarmUp": _multistep, "CyclicLR": _cyclic, "CosineAnnealingWarmupRestarts": _cosine}


def sequence(case, want_branch=False):
    rates, epochs = _BY_NAME[case["scheduler"]](case, want_branch)
    return np.array(rates, dtype=bool if want_branch else np.float64), np.array(epochs, dtype=np.int64)


def make_scheduler(case, dev, lr_tensors=False):
    """(optimizer, scheduler) of mcquic_amd for a fixture case: mcquic_amd.optim.SGD over one small parameter per group on `dev`, the
    groups' rates as the generator sets them (host floats; `lr_tensors`: 0-dim float32 tensors on `dev`, which the scheduler adopts)."""
    import torch
    from mcquic_amd import optim, schedule
    groups = []
    for lr in case["base_lrs"]:
        g = {"params": [torch.nn.Parameter(torch.zeros(4, device=dev))], "lr": torch.tensor(lr, dtype=torch.float32, device=dev) if lr_tensors else lr}
        if case["last_epoch"] != -1:
            g["initial_lr"] = lr
        groups.append(g)
    opt = optim.SGD(groups, lr=1.0)
    kwargs = dict(case["kwargs"])
    if case["last_epoch"] != -1:
        kwargs["last_epoch"] = case["last_epoch"]
    return opt, schedule.REGISTRY[case["scheduler"]](opt, **kwargs)
