"""Child process of tests/test_gpu_reassign_step.py::test_post_graph_holds_exactly_the_two_new_launches, run under
`rocprofv3 --kernel-trace --hip-runtime-trace`: two captured training steps of the small Compressor of tests/test_gpu_ema_step.py, one
WITHOUT `reassign=` and one with, each a segment graph followed by the post graph.  The process's last four hipGraphLaunch calls are
[segment, post] of the plain step, a synchronisation, then [segment, post] of the step with reassignment, and no device work follows:
the test cuts the kernel trace at those four timestamps."""
import os
import sys

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import torch  # noqa: E402


def main():
    import mcquic_amd
    from mcquic_amd import optim, parallel
    from test_gpu_ema_step import _setup
    dev = torch.device("cuda:0")
    steps = []
    for reassigned in (False, True):
        model, xs, us = _setup(dev)
        opt = optim.SGD(model.parameters(), lr=1e-2, momentum=0.9)
        extra = {"reassign": mcquic_amd.CodebookReassign(model, freq=1000)} if reassigned else {}
        steps.append((parallel.GraphedTrainStep(model, opt, xs[0], forward_kwargs={"uniforms": us}, **extra), xs[0]))
    for step, x in steps:                                     # (one replay each first: nothing is launched for the first time below)
        step(x)
    torch.cuda.synchronize()
    for step, x in steps:
        assert len(step.graphs) == 1 and step.post is not None
        step(x)
        torch.cuda.synchronize()


if __name__ == "__main__":
    main()
