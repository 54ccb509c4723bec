"""GPU: `parallel.GraphedTrainStep(..., skip_nonfinite=True)` on the model and shards of tests/test_gpu_ema_step.py (Compressor(32, 2,
[64, 32, 16]), two 64 x 64 images, segments=1), with the whole update in use: EMA, scheduler, meter.  Three batches -- clean, one NaN pixel,
clean.  A NaN input is ordinary arithmetic: nothing faults, the loss and every gradient come out NaN.  The skipped step must leave every
state dict bit for bit; the third step must land where a guard-OFF twin lands that only ever saw the two clean batches (its device
generator set to the states the guarded run had in front of them): the guard changes nothing about a clean step.  Both with the update
captured as the post graph and with `capture_post=False`, where the same update runs eagerly after the exchange."""
import collections
import copy
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CONFIGS = {"adam": ("adam", None), "adam-clip": ("adam", 4.0), "lamb": ("lamb", None), "sgd": ("sgd", None)}


def _build(dev, kind, clip, model, x, **extra):
    from mcquic_amd import monitor, optim, parallel, schedule
    from test_gpu_ema_step import HW, N
    if kind == "adam":
        opt = optim.Adam(model.parameters(), lr=1e-3)
    elif kind == "lamb":
        opt = optim.Lamb(model.parameters(), lr=1e-3)
    else:
        opt = optim.SGD(model.parameters(), lr=1e-2, momentum=0.9)
    ema = optim.EMA(model, decay=0.9)
    sched = schedule.CosineAnnealingWarmupRestarts(opt, 6, warmup_steps=2)
    meter = monitor.StepMeter(model, capacity=8, pixels=N * HW * HW)
    step = parallel.GraphedTrainStep(model, opt, x, segments=1, max_grad_norm=clip, ema=ema, scheduler=sched, meter=meter, **extra)
    return dict(model=model, opt=opt, ema=ema, sched=sched, meter=meter, step=step)


def _state(w):
    """Every tensor the post graph owns: model (parameters and every `_freqEMA`), optimizer state and step counts, the EMA shadow and its
    count, scheduler state and rates."""
    out = [v for _, v in sorted(w["model"].state_dict().items())]
    assert any("_freqEMA" in k for k in w["model"].state_dict())
    for p, st in w["opt"].state.items():
        out += [v for _, v in sorted(st.items()) if torch.is_tensor(v)]
    out += [plan.step for plan in w["opt"]._plans.values()]
    out += list(w["ema"].averages) + [w["ema"]._count, w["sched"]._buf] + list(w["sched"]._lrs)
    return out


def _same(a, b):
    a, b = list(a), list(b)
    return len(a) == len(b) and all(torch.equal(x.detach(), y.detach()) for x, y in zip(a, b))


@pytest.mark.parametrize("capture_post", [True, False], ids=["post-graph", "post-eager"])
@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_nan_batch_is_skipped_and_the_run_continues_as_if_it_never_came(dev, config, capture_post):
    from mcquic_amd import ops
    from test_gpu_ema_step import _setup
    kind, clip = CONFIGS[config]
    model, xs, _ = _setup(dev)
    bad = xs[1].clone()
    bad[1, 2, 7, 5] = float("nan")
    ours = _build(dev, kind, clip, model, xs[0], skip_nonfinite=True, capture_post=capture_post)
    twin = _build(dev, kind, clip, copy.deepcopy(model), xs[0], capture_post=capture_post)
    assert (ours["step"].post is not None) == capture_post and (twin["step"].post is not None) == capture_post and twin["step"].guard is None
    assert _same(_state(ours), _state(twin)), "the constructors left both where they started"
    guard, step = ours["step"].guard, ours["step"]

    rng0 = ops.get_rng_state(dev)
    l0 = step(xs[0]).clone()
    assert int(guard.skip) == 0 and int(guard.skipped) == 0 and torch.equal(step.grad_norm, guard.grad_norm)
    before = [t.detach().clone() for t in _state(ours)]
    l1 = step(bad).clone()
    assert not torch.isfinite(l1), "the NaN pixel reaches the loss"
    assert _same(_state(ours), before), "a skipped step leaves every tensor the post graph owns bit for bit"
    assert (int(guard.skip), int(guard.skipped), int(guard.consecutive)) == (1, 1, 1) and not np.isfinite(float(guard.grad_norm))
    guard.check(max_consecutive=2)
    with pytest.raises(RuntimeError, match="Loss becomes NAN. Train crashed."):
        guard.check(max_consecutive=1)
    rng2 = ops.get_rng_state(dev)
    l2 = step(xs[1]).clone()
    assert (int(guard.skip), int(guard.skipped), int(guard.consecutive)) == (0, 1, 0)
    rows = ours["meter"].read()
    assert rows["skipped"].tolist() == [0, 1, 1] and np.isnan(rows["grad_norm"][1]) and np.isfinite(rows["grad_norm"][[0, 2]]).all()
    assert rows["lr"][1] == rows["lr"][0] != rows["lr"][2], "the schedule stood still through the skipped step"

    ops.set_rng_state(rng0, dev)
    t0 = twin["step"](xs[0]).clone()
    ops.set_rng_state(rng2, dev)
    t2 = twin["step"](xs[1]).clone()
    assert torch.equal(l0, t0) and torch.equal(l2, t2)
    assert _same(_state(ours), _state(twin)), "after the skipped batch the run is the run that never saw it, bit for bit"
    assert not _same(_state(ours), before), "the clean steps do move the state"
    assert ours["ema"].num_updates == 2 and ours["sched"].last_epoch == twin["sched"].last_epoch
    if clip is not None:
        assert torch.equal(step.grad_norm, twin["step"].grad_norm)
    for w in (ours, twin):
        w["step"].close()


def test_contradictory_settings_are_refused(dev):
    from mcquic_amd import optim, parallel
    lin, x = torch.nn.Linear(2, 2).to(dev), torch.zeros(1, 2, device=dev)
    for own in (optim.Adam(lin.parameters(), skip_nonfinite=True), optim.Lamb(lin.parameters(), skip_nonfinite=True),
                optim.SGD(lin.parameters(), lr=0.1, skip_nonfinite=True)):
        with pytest.raises(ValueError, match="counted twice"):
            parallel.GraphedTrainStep(lin, own, x, skip_nonfinite=True)
    with pytest.raises(ValueError, match="whose kernels take the guard's flag"):
        parallel.GraphedTrainStep(lin, torch.optim.SGD(lin.parameters(), lr=0.1), x, skip_nonfinite=True)


def test_post_graph_kernel_names_guard_off_and_on(dev, tmp_path):
    """A kernel trace of the post graphs (tests/_guard_names_worker.py under rocprofv3), Adam with the step's clipping, Lamb and SGD, each
    with EMA + scheduler + meter.  With `skip_nonfinite=False` the replayed kernel-name list EQUALS the parent commit's, recorded from it
    with the same worker (tests/golden/f20_post_graph_kernel_names.json): not one launch changes.  With the guard on, every update launch
    is its `_skip` twin and the guard's own launches are in front."""
    import csv
    import glob
    import shutil
    import subprocess
    import sys
    from _guard_names_worker import KINDS
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    run = subprocess.run([prof, "--kernel-trace", "--hip-runtime-trace", "-f", "csv", "-d", str(tmp_path), "-o", "guard", "--",
                          sys.executable, os.path.join(HERE, "_guard_names_worker.py")], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]

    def rows(what):
        files = glob.glob(os.path.join(str(tmp_path), "**", f"*{what}.csv"), recursive=True)
        assert len(files) == 1, (what, files)
        with open(files[0]) as f:
            return list(csv.DictReader(f))
    launches = sorted(int(r["Start_Timestamp"]) for r in rows("hip_api_trace") if "GraphLaunch" in r["Function"])
    calls = 2 * len(KINDS)
    assert len(launches) >= 4 * calls, launches
    cuts = launches[-2 * calls:][::2] + [float("inf")]        # the segment graph's launch of each of the last `calls` calls
    kernels = sorted((int(r["Start_Timestamp"]), r["Kernel_Name"]) for r in rows("kernel_trace") if "copyBuffer" not in r["Kernel_Name"])

    def post_graph(i):
        names = [n for t, n in kernels if cuts[i] <= t < cuts[i + 1]]
        last = max(j for j, n in enumerate(names) if "gather_flat_kernel" in n)     # the segment graph ends with the gather
        return names[last + 1:]
    golden = json.load(open(os.path.join(HERE, "golden", "f20_post_graph_kernel_names.json")))["post_graph"]
    for k, kind in enumerate(KINDS):
        off, on = post_graph(2 * k), post_graph(2 * k + 1)
        print(kind, "guard off:", off)
        print(kind, "guard on:", on)
        assert off == golden[kind], (kind, off)
        guards = [n for n in on if "guard_" in n]
        assert not [n for n in off if "guard_" in n or "_skip_kernel" in n]
        want_guard = {"adam": ["guard_borrow_kernel"], "lamb": ["guard_finish_kernel"], "sgd": ["guard_gradsq_flat_kernel", "guard_finish_kernel"]}[kind]
        assert len(guards) == len(want_guard) and all(w in g for w, g in zip(want_guard, guards)), (kind, guards)
        assert len(on) == len(off) + len(guards), "the guard adds its own launches and nothing else"
        rest = [n for n in on if "guard_" not in n]
        meterless = collections.Counter("_skip_kernel" in n for n, o in zip(rest, off) if "meter_" not in o and "mse_" not in o and "lamb_gradsq" not in o
                                        and "sgd_update" not in o)
        assert meterless == {True: sum(meterless.values())}, (kind, rest)
        for n, o in zip(rest, off):                           # twin for twin, in the parent's order
            assert n.split("(anonymous namespace)::")[1].split("(")[0].replace("_skip_kernel", "_kernel") == \
                o.split("(anonymous namespace)::")[1].split("(")[0], (n, o)
