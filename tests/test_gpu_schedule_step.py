"""mcquic_amd.schedule through parallel.GraphedTrainStep(..., scheduler=...), on the model and shards of tests/test_gpu_ema_step.py:
Compressor(32, 2, [64, 32, 16]), two 64 x 64 images, fixed uniforms, mcquic_amd.optim.SGD and mcquic_amd.optim.Adam.  The twin of a
scheduled step is an identical model and optimizer whose `lr` tensor the HOST fills, before each replay, with the float32 rate the
scheduler held at that point: the two must agree bit for bit -- the schedule inside the post graph changes WHERE the rate comes from,
never a value."""
import copy

import numpy as np
import pytest
import torch

import _schedule_ref as R

pytestmark = pytest.mark.gpu
KS, HW, N, STEPS = [64, 32, 16], 64, 2, 8
COSINE = dict(first_cycle_steps=6, cycle_mult=1.5, lrScaleRatio=0.1, warmup_steps=2, gamma=0.5)
BASE = {"sgd": 1e-2, "adam": 1e-3}


def _optimizer(kind, model, lr):
    from mcquic_amd import optim
    return optim.SGD(model.parameters(), lr=lr, momentum=0.9) if kind == "sgd" else optim.Adam(model.parameters(), lr=lr)


def _reference(kind, steps):
    """The float64 rates of the schedule, from the restatement that equals the reference exactly (tests/test_schedule_ref.py)."""
    case = dict(scheduler="CosineAnnealingWarmupRestarts", kwargs=COSINE, base_lrs=[BASE[kind]], steps=steps, last_epoch=-1)
    return R.sequence(case)[0][:, 0]


def _state(opt):
    return [v.detach().clone() for st in opt.state.values() for _, v in sorted(st.items()) if torch.is_tensor(v)]


def _same(a, b):
    a, b = list(a), list(b)
    return len(a) == len(b) and all(torch.equal(x.detach(), y.detach()) for x, y in zip(a, b))


@pytest.fixture(scope="module", params=["sgd", "adam"])
def pair(request, dev):
    """Eight replays of the scheduled step and of its host-filled twin; then what the later tests look at."""
    from mcquic_amd import monitor, parallel, schedule
    from test_gpu_ema_step import _setup
    kind = request.param
    ours, xs, us = _setup(dev)
    twin = copy.deepcopy(ours)
    opt_o = _optimizer(kind, ours, BASE[kind])
    sched = schedule.CosineAnnealingWarmupRestarts(opt_o, **COSINE)
    built = (sched._buf.clone(), sched._lrs[0].clone())
    meter = monitor.StepMeter(ours, capacity=32, pixels=N * HW * HW)
    step_o = parallel.GraphedTrainStep(ours, opt_o, xs[0], forward_kwargs={"uniforms": us}, scheduler=sched, meter=meter)
    after_ctor = (sched._buf.clone(), sched._lrs[0].clone())
    lr_t = torch.zeros((), dtype=torch.float32, device=dev)
    opt_t = _optimizer(kind, twin, lr_t)
    step_t = parallel.GraphedTrainStep(twin, opt_t, xs[0], forward_kwargs={"uniforms": us})
    recorded, losses = [], []
    for it in range(STEPS):
        recorded.append(sched._lrs[0].clone())                # the float32 rate this replay's update reads
        lr_t.copy_(recorded[-1])
        lo, lt = step_o(xs[it % 2]), step_t(xs[it % 2])
        losses.append((lo.clone(), lt.clone()))
    recorded.append(sched._lrs[0].clone())
    return dict(kind=kind, ours=ours, twin=twin, opt_o=opt_o, opt_t=opt_t, sched=sched, meter=meter, step_o=step_o, step_t=step_t, lr_t=lr_t,
                built=built, after_ctor=after_ctor, recorded=torch.stack(recorded).cpu().numpy(), losses=losses, xs=xs, rows=meter.read())


def test_constructor_leaves_the_schedule_as_it_was(pair):
    assert pair["step_o"].post is not None and pair["step_t"].post is not None
    for before, after in zip(pair["built"], pair["after_ctor"]):
        assert torch.equal(before, after), "GraphedTrainStep's prepare() / warm() moved the schedule"
    assert int(pair["built"][0][0]) == 0


def test_scheduled_step_equals_the_host_filled_twin(pair):
    assert all(torch.equal(a, b) for a, b in pair["losses"])
    assert _same(pair["ours"].parameters(), pair["twin"].parameters()), "parameters"
    so, st = _state(pair["opt_o"]), _state(pair["opt_t"])
    assert len(so) > 0 and _same(so, st), "optimizer state"
    assert pair["sched"].last_epoch == STEPS
    assert len(set(pair["recorded"].tolist())) > 6, "the rate did not move: this comparison would hold without a schedule"


def test_rates_and_meter_column_are_the_schedule(pair):
    """The float64 rates are the reference's under the leaf test's bar; the float32 tensor is their rounding; and the meter, which runs
    after the scheduler as the reference logs `get_last_lr()` after stepping, records the rate of the NEXT update.  Without a scheduler
    that column is a constant (tests/test_gpu_step_meter_step.py, and the plain step of the names test below): this assertion is what
    the parent commit cannot meet."""
    want = _reference(pair["kind"], STEPS)
    peak = np.abs(want).max()
    assert abs(pair["sched"].get_last_lr()[0] - want[STEPS]) <= 2.0 ** -50 * peak
    rec = pair["recorded"]
    # float32 rounding (half an ulp: 2^-24 relative) on top of the float64 bar
    assert (np.abs(rec.astype(np.float64) - want) <= (2.0 ** -24 + 2.0 ** -50) * peak).all(), (rec, want)
    col = pair["rows"]["lr"]
    assert pair["rows"]["steps"].tolist() == list(range(STEPS))
    assert col.tobytes() == rec[1:].tobytes(), (col, rec)
    assert len(set(col.tolist())) > 6


def test_invalidate_evaluate_and_further_replays_keep_the_sequence(pair):
    """(runs after the tests above: it moves the fixture's models on)"""
    step_o, step_t, sched, lr_t, xs = (pair[k] for k in ("step_o", "step_t", "sched", "lr_t", "xs"))
    for step, model in ((step_o, pair["ours"]), (step_t, pair["twin"])):
        step.invalidate()
        model.eval()
        with torch.no_grad():
            model.encode(xs[1])
        model.train()
    assert sched.last_epoch == STEPS, "evaluating moved the schedule"
    more = 4
    for it in range(more):
        lr_t.copy_(sched._lrs[0])
        step_o(xs[it % 2])
        step_t(xs[it % 2])
    assert sched.last_epoch == STEPS + more
    assert _same(pair["ours"].parameters(), pair["twin"].parameters())
    want = _reference(pair["kind"], STEPS + more)
    assert abs(sched.get_last_lr()[0] - want[-1]) <= 2.0 ** -50 * np.abs(want).max()
    col = pair["meter"].read()["lr"]
    assert len(col) == more and col[-1] == np.float32(sched.get_last_lr()[0])


def test_a_scheduler_of_another_optimizer_is_refused(dev):
    from mcquic_amd import optim, parallel, schedule
    p = [torch.nn.Parameter(torch.zeros(4, device=dev))]
    a, b = optim.SGD(p, lr=0.1), optim.SGD(p, lr=0.1)
    with pytest.raises(ValueError, match="another optimizer"):
        parallel.GraphedTrainStep(torch.nn.Linear(2, 2).to(dev), a, torch.zeros(1, 2, device=dev), scheduler=schedule.Placeholder(b))


def test_post_graph_kernel_names_with_and_without_a_scheduler(dev, tmp_path):
    """A fresh count of the post graph's kernels (tests/_schedule_names_worker.py under rocprofv3: a plain step, then a scheduled one):
    the plain step's post graph holds no schedule kernel, and the scheduled one holds the same kernels plus exactly one launch of it."""
    import collections
    import csv
    import glob
    import os
    import shutil
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    run = subprocess.run([prof, "--kernel-trace", "--hip-runtime-trace", "-f", "csv", "-d", str(tmp_path), "-o", "sched", "--",
                          sys.executable, os.path.join(here, "_schedule_names_worker.py")], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]

    def rows(kind):
        files = glob.glob(os.path.join(str(tmp_path), "**", f"*{kind}.csv"), recursive=True)
        assert len(files) == 1, (kind, files)
        with open(files[0]) as f:
            return list(csv.DictReader(f))
    launches = sorted(int(r["Start_Timestamp"]) for r in rows("hip_api_trace") if "GraphLaunch" in r["Function"])
    assert len(launches) >= 8, launches
    seg_plain, _, seg_sched, _ = launches[-4:]
    # (`__amd_rocclr_copyBuffer`: a call's copy of its shard into the static input, in front of the graphs and in neither of them)
    kernels = sorted((int(r["Start_Timestamp"]), r["Kernel_Name"]) for r in rows("kernel_trace") if "copyBuffer" not in r["Kernel_Name"])

    def post_graph(names):
        """A call's kernels from the optimizer's first on: the post graph (a launch is asynchronous, so the API timestamp of the post
        graph's hipGraphLaunch does not separate it from the segment graph's kernels; the worker synchronises between the two CALLS)."""
        first = max(i for i, n in enumerate(names) if "sgd_prepare_kernel" in n)
        assert sum("sgd_prepare_kernel" in n for n in names) == 1
        return collections.Counter(names[first:])
    call_plain, call_sched = [n for t, n in kernels if seg_plain <= t < seg_sched], [n for t, n in kernels if t >= seg_sched]
    plain, sched = post_graph(call_plain), post_graph(call_sched)
    assert len(call_plain) > 200 and len(call_sched) == len(call_plain) + 1, "the segment graphs are the same launches"
    print("post graph, plain step:", dict(plain))
    print("post graph, scheduled step:", dict(sched))
    assert sum(plain.values()) >= 3 and any("sgd" in n for n in plain), plain
    assert not [n for n in plain if "lr_schedule" in n]
    extra = sched - plain
    assert not (plain - sched) and sum(extra.values()) == 1 and "lr_schedule_kernel" in next(iter(extra)), (plain, sched)
