#!/usr/bin/env python3
"""Capture F19 (tests/golden/f19_lr_schedules.npz): the learning-rate sequences of the REAL reference's schedulers
(mcquic/train/lrSchedulers.py: Placeholder, MultiStepLRWithWarmUp, CyclicLR, CosineAnnealingWarmupRestarts), imported unmodified from
the reference tree and stepped on a CPU torch.optim.SGD whose rates are Python floats.  Runs only where the reference tree is; the
output is data: case parameters and float64 rate sequences of at most 64 steps each.

    python tests/golden/make_golden_schedules.py

The loader supplies the two things the file needs from its surroundings: a pass-through `mcquic.utils.LrSchedulerRegistry` (the real
one pulls vlutils), and a wrapper around `torch.optim.lr_scheduler._LRScheduler.__init__` that drops the `verbose` argument the
reference still passes and current torch no longer takes.

Stored:
    cases          JSON: a list of {"name", "scheduler", "kwargs", "base_lrs", "steps", "last_epoch"}; `last_epoch` != -1 is a resume
                   constructor (the groups carry `initial_lr` = `lr` = base_lrs)
    rates_<name>   float64 [steps + 1, groups]: the groups' `lr` after the constructor, then after each `step()`
    epochs_<name>  int64 [steps + 1]: `last_epoch` at the same points
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_harness              # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
COSINE_A = dict(first_cycle_steps=6, cycle_mult=1.5, lrScaleRatio=0.1, warmup_steps=2, gamma=0.5)
CYCLIC = dict(base_lr=0.01, max_lr=0.1, step_size_up=3, step_size_down=2)
CASES = [
    dict(name="cosine_restarts", scheduler="CosineAnnealingWarmupRestarts", kwargs=COSINE_A, base_lrs=[0.1], steps=40),
    # configs/a800_8.yaml (2000 warm-up steps, one 100 000-step cycle, lrScaleRatio 0.0) scaled down, run past the restart
    dict(name="cosine_a800", scheduler="CosineAnnealingWarmupRestarts",
         kwargs=dict(first_cycle_steps=20, cycle_mult=1.0, lrScaleRatio=0.0, warmup_steps=4, gamma=1.0), base_lrs=[1e-4], steps=48),
    dict(name="multistep", scheduler="MultiStepLRWithWarmUp", kwargs=dict(milestones=[3, 5, 8], gamma=0.1), base_lrs=[0.05], steps=16),
    dict(name="multistep_duplicate", scheduler="MultiStepLRWithWarmUp", kwargs=dict(milestones=[2, 4, 4, 7], gamma=0.5), base_lrs=[0.05], steps=12),
    dict(name="cyclic_triangular", scheduler="CyclicLR", kwargs=dict(CYCLIC, mode="triangular", cycle_momentum=False), base_lrs=[0.01], steps=24),
    dict(name="cyclic_triangular2", scheduler="CyclicLR", kwargs=dict(CYCLIC, mode="triangular2", cycle_momentum=False), base_lrs=[0.01], steps=24),
    dict(name="cyclic_exp_range", scheduler="CyclicLR", kwargs=dict(CYCLIC, mode="exp_range", gamma=0.9, cycle_momentum=False), base_lrs=[0.01], steps=24),
    dict(name="placeholder", scheduler="Placeholder", kwargs={}, base_lrs=[0.02], steps=5),
    dict(name="cosine_two_groups", scheduler="CosineAnnealingWarmupRestarts", kwargs=COSINE_A, base_lrs=[0.1, 0.003], steps=40),
    dict(name="cyclic_two_groups", scheduler="CyclicLR",
         kwargs=dict(base_lr=[0.01, 0.002], max_lr=[0.1, 0.05], step_size_up=3, step_size_down=2, mode="triangular2", cycle_momentum=False),
         base_lrs=[0.01, 0.002], steps=24),
] + [dict(name=f"cosine_resume_{k}", scheduler="CosineAnnealingWarmupRestarts", kwargs=COSINE_A, base_lrs=[0.1], steps=24, last_epoch=k)
     for k in (0, 5, 9, 30)]


def reference_schedulers():
    """The reference's lrSchedulers module, unmodified."""
    registry = types.SimpleNamespace(register=lambda cls: cls)
    pkg = types.ModuleType("mcquic")
    pkg.__path__ = []
    utils = types.ModuleType("mcquic.utils")
    utils.LrSchedulerRegistry = registry
    sys.modules.setdefault("mcquic", pkg)
    sys.modules["mcquic.utils"] = utils
    base = torch.optim.lr_scheduler._LRScheduler
    init = base.__init__

    def without_verbose(self, optimizer, last_epoch=-1, verbose=False):
        init(self, optimizer, last_epoch)
    base.__init__ = without_verbose
    spec = importlib.util.spec_from_file_location("mcquic_reference_lrSchedulers", os.path.join(ref_harness.REF, "mcquic", "train", "lrSchedulers.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    import warnings
    warnings.simplefilter("ignore")                          # ("lr_scheduler.step() before optimizer.step()": no optimizer steps here)
    ref = reference_schedulers()
    out = {}
    cases = []
    for case in CASES:
        case = dict(case)
        case.setdefault("last_epoch", -1)
        groups = []
        for lr in case["base_lrs"]:
            g = {"params": [torch.nn.Parameter(torch.zeros(1))], "lr": lr}
            if case["last_epoch"] != -1:
                g["initial_lr"] = lr
            groups.append(g)
        opt = torch.optim.SGD(groups, lr=1.0)
        kwargs = dict(case["kwargs"])
        if case["last_epoch"] != -1:
            kwargs["last_epoch"] = case["last_epoch"]
        sched = getattr(ref, case["scheduler"])(opt, **kwargs)
        rates, epochs = [], []
        for i in range(case["steps"] + 1):
            if i:
                sched.step()
            rates.append([float(g["lr"]) for g in opt.param_groups])
            epochs.append(int(sched.last_epoch))
        assert case["steps"] <= 64
        out[f"rates_{case['name']}"] = np.array(rates, dtype=np.float64)
        out[f"epochs_{case['name']}"] = np.array(epochs, dtype=np.int64)
        cases.append(case)
        print(case["name"], epochs[0], epochs[-1], " ".join(f"{r[0]:.6g}" for r in rates[:14]))
    out["cases"] = np.array(json.dumps(cases))
    path = os.path.join(OUT, "f19_lr_schedules.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
