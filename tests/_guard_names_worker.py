"""Child process of tests/test_gpu_step_guard_step.py::test_post_graph_kernel_names_guard_off_and_on, run under
`rocprofv3 --kernel-trace --hip-runtime-trace`: captured training steps of the small Compressor of tests/test_gpu_ema_step.py with the whole
post graph in use (EMA, scheduler, meter), for Adam with the step's clipping, Lamb and SGD -- each once with `skip_nonfinite=False` and once
with `skip_nonfinite=True`.  The process's last hipGraphLaunch calls are [segment, post] of every step in that order with a synchronisation
between the calls, and no device work follows: the test cuts the kernel trace at those timestamps.

`python tests/_guard_names_worker.py record` builds the steps WITHOUT the keyword at all (so it runs on a tree that has no guard): that is how
tests/golden/f20_post_graph_kernel_names.json was recorded from the parent commit."""
import os
import sys

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import torch  # noqa: E402

KINDS = ("adam", "lamb", "sgd")


def build(kind, dev, extra):
    from mcquic_amd import monitor, optim, parallel, schedule
    from test_gpu_ema_step import HW, N, _setup
    model, xs, us = _setup(dev)
    if kind == "adam":
        opt, clip = optim.Adam(model.parameters(), lr=1e-3), 4.0
    elif kind == "lamb":
        opt, clip = optim.Lamb(model.parameters(), lr=1e-3), None
    else:
        opt, clip = optim.SGD(model.parameters(), lr=1e-2, momentum=0.9), None
    step = parallel.GraphedTrainStep(model, opt, xs[0], forward_kwargs={"uniforms": us}, max_grad_norm=clip, ema=optim.EMA(model, decay=0.9),
                                     scheduler=schedule.CosineAnnealingWarmupRestarts(opt, 6, warmup_steps=2),
                                     meter=monitor.StepMeter(model, capacity=8, pixels=N * HW * HW), **extra)
    return step, xs[0]


def main():
    dev = torch.device("cuda:0")
    arms = [{}] if sys.argv[1:] == ["record"] else [{"skip_nonfinite": False}, {"skip_nonfinite": True}]
    steps = [build(kind, dev, extra) for kind in KINDS for extra in arms]
    for step, x in steps:                                     # (one replay each first: nothing is launched for the first time below)
        step(x)
    torch.cuda.synchronize()
    for step, x in steps:
        assert len(step.graphs) == 1 and step.post is not None
        step(x)
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
