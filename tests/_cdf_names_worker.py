"""Child process of tests/test_gpu_code_bits.py::test_the_capture_holds_two_library_kernels_and_nothing_else, run under
`rocprofv3 --kernel-trace --hip-runtime-trace`: `EntropyCoder.deviceCDFs(normalize=True)` followed by `codeBits`, captured into one graph
and replayed.  The process's last hipGraphLaunch is the second replay and no device work follows it: the test reads the kernel trace
from that timestamp on."""
import os
import sys

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import torch  # noqa: E402


def main():
    from mcquic_amd.modules import entropyCoder as E
    dev = torch.device("cuda:0")
    ks = [512, 64, 7]
    coder = E.EntropyCoder(2, ks).to(dev)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for f in coder._freqEMA:
            f.copy_((torch.rand(f.shape, generator=g) ** 4 + 1e-6).to(dev))
    codes = [torch.randint(0, k, (2, 2, 17 >> lv, 9 >> lv), generator=g).to(dev) for lv, k in enumerate(ks)]

    def run():
        tables = coder.deviceCDFs(normalize=True)
        return coder.codeBits(codes, cdfs=tables)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run()
    graph.replay()                                            # (nothing is launched for the first time below)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
