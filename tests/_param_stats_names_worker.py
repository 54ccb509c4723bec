"""Child process of tests/test_gpu_param_stats_step.py::test_post_graph_kernel_names_with_and_without_stats, run under
`rocprofv3 --kernel-trace --hip-runtime-trace`: two captured training steps of the small Compressor of that file with the whole post graph
in use (Adam with the step's clipping, EMA, scheduler, meter) -- the first with `stats=None`, the second with a `monitor.ParamStats`.  The
process's last hipGraphLaunch calls are [segment, post] of the two steps in that order with a synchronisation between the calls, and no
device work follows: the test cuts the kernel trace at those timestamps."""
import os
import sys

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import torch  # noqa: E402

ARMS = ("off", "on")


def build(arm, dev):
    from mcquic_amd import monitor, optim, parallel, schedule
    from test_gpu_param_stats_step import HW, N, _setup
    model, xs, us = _setup(dev)
    opt = optim.Adam(model.parameters(), lr=1e-3)
    stats = monitor.ParamStats(model, capacity=4) if arm == "on" else None
    step = parallel.GraphedTrainStep(model, opt, xs[0], forward_kwargs={"uniforms": us}, max_grad_norm=4.0, ema=optim.EMA(model, decay=0.9),
                                     scheduler=schedule.CosineAnnealingWarmupRestarts(opt, 6, warmup_steps=2),
                                     meter=monitor.StepMeter(model, capacity=8, pixels=N * HW * HW), stats=stats)
    return step, xs[0]


def main():
    dev = torch.device("cuda:0")
    steps = [build(arm, dev) for arm in ARMS]
    for step, x in steps:                                     # (one replay each first: nothing is launched for the first time below)
        step(x)
    torch.cuda.synchronize()
    for step, x in steps:
        assert len(step.graphs) == 1 and step.post is not None
        step(x)
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
