"""Child process of tests/test_gpu_step_snapshot_step.py::test_replay_launches_what_a_step_without_a_snapshot_launches, run under
`rocprofv3 --kernel-trace --hip-runtime-trace`: two captured training steps of the small Compressor of tests/test_gpu_ema_step.py (SGD, the
step's clipping, a meter), the first built as before and never shown a snapshot, the second with `keep_outputs=True` and a
`step.snapshot(...)` taken before its last replay.  The process's last hipGraphLaunch calls are [segment, post] of the two steps in that
order with a synchronisation between the calls, and no device work follows: the test cuts the kernel trace at those timestamps."""
import os
import sys

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import torch  # noqa: E402


def build(dev, keep):
    from mcquic_amd import monitor, optim, parallel
    from test_gpu_ema_step import HW, N, _setup
    model, xs, us = _setup(dev)
    extra = {"keep_outputs": True} if keep else {}
    step = parallel.GraphedTrainStep(model, optim.SGD(model.parameters(), lr=1e-2, momentum=0.9), xs[0], forward_kwargs={"uniforms": us},
                                     max_grad_norm=4.0, meter=monitor.StepMeter(model, capacity=8, pixels=N * HW * HW), **extra)
    snap = monitor.StepSnapshot(model, batch_shape=(N, 3, HW, HW), images=1) if keep else None
    return step, xs[0], snap


def main():
    dev = torch.device("cuda:0")
    steps = [build(dev, keep) for keep in (False, True)]
    for step, x, snap in steps:                               # (one replay each first: nothing is launched for the first time below)
        step(x)
        if snap is not None:
            payload = step.snapshot(snap)
            assert payload["Train/Raw"].shape == (1, 3, x.shape[2], x.shape[3])
    torch.cuda.synchronize()
    for step, x, _ in steps:
        assert len(step.graphs) == 1 and step.post is not None
        step(x)
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
