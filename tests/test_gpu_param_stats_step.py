"""mcquic_amd.monitor.ParamStats through parallel.GraphedTrainStep(..., stats=...), on the small model and shards of
tests/test_gpu_ema_step.py (built here the same way): Compressor(32, 2, [64, 32, 16]), two 64 x 64 images, fixed uniforms, optim.Adam.
The rows of the captured step are compared with the float64 reference of tests/_param_stats_ref.py evaluated on host copies taken around
an uncaptured twin step that starts from the same state; the bars are those of tests/test_gpu_param_stats_leaf.py (derived there)."""
import copy
import csv
import glob
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import _param_stats_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CH, KS, HW, N, LR = 32, [64, 32, 16], 64, 2, 1e-3


def _uniforms(n, hw, ks, dev, seed):
    g = torch.Generator().manual_seed(seed)
    us = []
    for lv, k in enumerate(ks):
        s = hw // 16 // (2 ** lv)
        us.append((torch.rand((n, 2, s, s, k), generator=g).to(dev), torch.rand((n, 2, s, s, k), generator=g).to(dev)))
    return us


def _setup(dev, seed=17):
    from mcquic_amd import Compressor
    torch.manual_seed(seed)
    model = Compressor(CH, 2, KS).to(dev).train()
    xs = [(torch.rand((N, 3, HW, HW), generator=torch.Generator().manual_seed(90 + i)) * 2 - 1).to(dev) for i in range(2)]
    return model, xs, _uniforms(N, HW, KS, dev, 14)


def _same(a, b):
    return all(torch.equal(x.detach(), y.detach()) for x, y in zip(a, b))


def _trainable(model):
    return [(n, p) for n, p in model.named_parameters() if p.requires_grad]


def test_rows_of_the_captured_step_against_the_reference(dev):
    """Four replays with every=1.  The twin runs the same update eagerly (capture_post=False), so the host can copy the weights in front
    of it and the consumed gradients (`step.flat`) and the weights behind it.  The step's own norm is the guard's here (double partials
    over the flat buffer, rounded once): G_s = G (1 + e), |e| <= 2^-24.  Every recorded grad_norm_t is ||g_t|| (1 + e_t), |e_t| <= 2^-24
    (the double sums' own error, ~1e-12, aside), so sum_t grad_norm_t^2 = G^2 (1 + e'), |e'| <= 2^-23 + 2^-48, and its float64 square
    root is G (1 + e''), |e''| <= 2^-24: the two differ by at most 2^-23 G, two float32 ulps (an ulp is at least 2^-24 of its value)."""
    from mcquic_amd import monitor, optim, parallel
    ours, xs, us = _setup(dev)
    twin = copy.deepcopy(ours)
    stats = monitor.ParamStats(ours, capacity=8)
    step_o = parallel.GraphedTrainStep(ours, optim.Adam(ours.parameters(), lr=LR), xs[0], forward_kwargs={"uniforms": us}, stats=stats,
                                       skip_nonfinite=True)
    step_t = parallel.GraphedTrainStep(twin, optim.Adam(twin.parameters(), lr=LR), xs[0], forward_kwargs={"uniforms": us}, capture_post=False,
                                       skip_nonfinite=True)
    assert step_o.post is not None and step_t.post is None
    assert stats.read()["count"] == 0 and stats.blame() is None, "the constructor left no row"
    names = [n for n, _ in _trainable(twin)]
    assert stats.names == names and len(names) > 20
    at, off = {}, 0
    for p in step_t.live:
        at[id(p)] = (off, off + p.numel())
        off += p.numel()
    rec, norms = R.Recorder(len(names), 8, 1), []
    for it in range(4):
        w0 = [p.detach().cpu().numpy().copy() for _, p in _trainable(twin)]
        step_o(xs[it % 2])
        step_t(xs[it % 2])
        flat = step_t.flat.cpu().numpy()
        grads = [flat[slice(*at[id(p)])] if id(p) in at else None for _, p in _trainable(twin)]
        rec.after([p.detach().cpu().numpy() for _, p in _trainable(twin)], grads, w0)
        norms.append((float(step_o.grad_norm), float(step_t.grad_norm)))
    assert _same(ours.parameters(), twin.parameters()), "the captured step with statistics and the eager twin without"
    got, want = stats.read(), rec.read()
    assert got["steps"].tolist() == [0, 1, 2, 3] and got["count"] == 4 and got["dropped"] == 0 and got["names"] == names
    assert (got["first_bad_step"], got["first_bad_tensor"]) == (-1, -1) and stats.blame() is None
    for name in ("grad_absmax", "grad_nonfinite"):
        assert np.array_equal(got[name].astype(np.float64), want[name]), name
    for name in ("weight_norm", "grad_norm", "update_norm"):
        ok = R.within_one_ulp(got[name], want[name])
        assert ok.all(), (name, got[name][~ok], want[name][~ok])
    assert np.all(got["update_norm"][:, [i for i, (_, p) in enumerate(_trainable(twin)) if id(p) in at]] > 0), "Adam moves every live tensor"
    for row, (g_o, g_t) in zip(got["grad_norm"], norms):
        total = float(np.sqrt(np.sum(row.astype(np.float64) ** 2)))
        print(f"sqrt(sum grad_norm_t^2) = {total!r}, the step's grad_norm = {g_o!r}")
        assert g_o == g_t and abs(total - g_o) <= 2.0 ** -23 * g_o * (1 + 1e-6)
    step_o.close()
    step_t.close()


def test_a_skipped_step_leaves_a_row_and_a_name(dev):
    """every=100: the clean first step is sampled (count 0), the NaN batch at count 1 is not -- and recorded all the same."""
    from mcquic_amd import monitor, optim, parallel
    model, xs, us = _setup(dev)
    bad = xs[1].clone()
    bad[1, 2, 7, 5] = float("nan")                            # (a data value)
    stats = monitor.ParamStats(model, capacity=4, every=100)
    step = parallel.GraphedTrainStep(model, optim.Adam(model.parameters(), lr=LR), xs[0], forward_kwargs={"uniforms": us}, stats=stats,
                                     skip_nonfinite=True)
    step(xs[0])
    before = [p.detach().clone() for p in model.parameters()]
    step(bad)
    assert int(step.guard.skip) == 1 and int(step.guard.skipped) == 1, "the step is skipped"
    assert _same(model.parameters(), before), "a skipped step leaves the parameters bit for bit"
    step(xs[1])
    assert int(step.guard.skip) == 0 and not _same(model.parameters(), before)
    got = stats.read()
    assert got["steps"].tolist() == [0, 1] and got["count"] == 3, "count 1 left a row although every=100; count 2 did not"
    assert not np.any(got["update_norm"][1]) and np.any(got["update_norm"][0] > 0)
    assert np.any(got["grad_nonfinite"][1] > 0) and not np.any(got["grad_nonfinite"][0])
    named = dict(_trainable(model))
    at, name = stats.blame()
    assert at == 1 and name in named and got["names"].index(name) == int(np.nonzero(got["grad_nonfinite"][1] > 0)[0][0]) == got["first_bad_tensor"]
    assert np.array_equal(got["weight_norm"][1], got["weight_norm"][0]), "the weights of the skipped step are the first step's"
    step.close()


def test_the_statistics_only_read(dev):
    """Three steps with `stats=` and three with `stats=None` from the same state: the same bits."""
    from mcquic_amd import monitor, optim, parallel
    a, xs, us = _setup(dev)
    b = copy.deepcopy(a)
    step_a = parallel.GraphedTrainStep(a, optim.Adam(a.parameters(), lr=LR), xs[0], forward_kwargs={"uniforms": us},
                                       stats=monitor.ParamStats(a, capacity=2, every=2))
    step_b = parallel.GraphedTrainStep(b, optim.Adam(b.parameters(), lr=LR), xs[0], forward_kwargs={"uniforms": us}, stats=None)
    assert step_a.post is not None and step_b.post is not None and _same(a.parameters(), b.parameters())
    for it in range(3):
        la, lb = step_a(xs[it % 2]), step_b(xs[it % 2])
        assert torch.equal(la, lb), it
    assert _same(a.parameters(), b.parameters()) and _same(a.buffers(), b.buffers())
    assert step_a.stats.read()["steps"].tolist() == [0, 2]
    step_a.close()
    step_b.close()


def test_post_graph_kernel_names_with_and_without_stats(dev, tmp_path):
    """A kernel trace of two post graphs (tests/_param_stats_names_worker.py under rocprofv3): Adam with the step's clipping, EMA, scheduler
    and meter, without and with `stats=`.  Without it no kernel of csrc/param_stats.hip is launched; with it the list is the same list
    plus the three new kernels, `before` directly in front of the optimizer's launches and `after`, `finish` directly behind them."""
    from _param_stats_names_worker import ARMS
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    run = subprocess.run([prof, "--kernel-trace", "--hip-runtime-trace", "-f", "csv", "-d", str(tmp_path), "-o", "stats", "--",
                          sys.executable, os.path.join(HERE, "_param_stats_names_worker.py")], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]

    def rows(what):
        files = glob.glob(os.path.join(str(tmp_path), "**", f"*{what}.csv"), recursive=True)
        assert len(files) == 1, (what, files)
        with open(files[0]) as f:
            return list(csv.DictReader(f))
    launches = sorted(int(r["Start_Timestamp"]) for r in rows("hip_api_trace") if "GraphLaunch" in r["Function"])
    calls = len(ARMS)
    assert len(launches) >= 4 * calls, launches
    cuts = launches[-2 * calls:][::2] + [float("inf")]        # the segment graph's launch of each of the last `calls` calls
    kernels = sorted((int(r["Start_Timestamp"]), r["Kernel_Name"]) for r in rows("kernel_trace") if "copyBuffer" not in r["Kernel_Name"])

    def post_graph(i):
        names = [n for t, n in kernels if cuts[i] <= t < cuts[i + 1]]
        last = max(j for j, n in enumerate(names) if "gather_flat_kernel" in n)     # the segment graph ends with the gather
        return names[last + 1:]
    off, on = post_graph(0), post_graph(1)
    print("stats=None:", off)
    print("stats=ParamStats:", on)
    assert not [n for n in off if "param_stats_" in n]
    new = [n for n in on if "param_stats_" in n]
    assert len(new) == 3 and all(w in n for w, n in zip(("param_stats_before_kernel", "param_stats_after_kernel", "param_stats_finish_kernel"), new))
    assert [n for n in on if "param_stats_" not in n] == off, "the three new kernels are the only difference"
    i0, i1, i2 = (on.index(n) for n in new)
    adam = [j for j, n in enumerate(on) if "adam_" in n]
    assert adam and adam == list(range(i0 + 1, i1)) and i2 == i1 + 1, "before | the optimizer's launches | after, finish"
