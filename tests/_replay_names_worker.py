"""Child process of tests/test_gpu_step_ops.py::test_training_step_replay_trace_holds_only_our_kernels, run under
`rocprofv3 --kernel-trace --hip-runtime-trace`: captures one training step (forward + backward) of a small Compressor as a
hipGraph, replays it once, then once more as the process's last hipGraphLaunch, with no other device work after it --
the kernels the trace records from that launch on are the replay's.  (torch.profiler is not used: it links a device activity
to the API call that launched it, and the ~600 kernels of one replay share ONE hipGraphLaunch -- it reports anything from 0
to a few hundred of them.)"""
import os
import sys

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
os.environ["MCQUIC_AMD_BRANCH_STREAMS"] = "0"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mcquic_amd import Compressor  # noqa: E402
from mcquic_amd.autograd import backward, mse_loss  # noqa: E402


def main():
    dev = torch.device("cuda:0")
    torch.manual_seed(3407)
    model = Compressor(16, 2, [64, 32, 16]).to(dev).train()
    x = (torch.rand((2, 3, 128, 128), generator=torch.Generator().manual_seed(0)) * 2 - 1).to(dev)

    def step():
        for p in model.parameters():
            p.grad = None
        xHat, _, _, _ = model(x)
        loss = mse_loss(xHat, x)
        backward(loss)
        return loss
    for _ in range(2):
        step()
    torch.cuda.synchronize()
    for p in model.parameters():
        p.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    graph.replay()
    torch.cuda.synchronize()
    graph.replay()                                  # the replay the test reads: the last hipGraphLaunch
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
