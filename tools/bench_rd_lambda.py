"""`encode(x)` and `encode(x, rd_lambda=0.1)` on the headline model at 32 x 768x512, for the tree in the CURRENT directory: run it from the
root of each of two built trees in turn to compare them (docs/experiments.md section 31).  One MI355X.

    python /path/to/tools/bench_rd_lambda.py LABEL"""
import os
import statistics
import sys

sys.path.insert(0, os.getcwd())
import torch
from mcquic_amd import Compressor
dev = torch.device("cuda")
g = torch.Generator().manual_seed(1)
model = Compressor(128, 2, [8192, 2048, 512]).eval().to(dev)
with torch.no_grad():
    for f in model._quantizer._entropyCoder._freqEMA:
        f.copy_(torch.rand(f.shape, generator=g).to(dev) + 0.01)
x = (torch.rand((32, 3, 512, 768), generator=g) * 2 - 1).to(dev)
def timed(fn, reps=7, warm=3, inner=5):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner): fn()
        b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    return statistics.median(ts), min(ts), max(ts)
with torch.no_grad():
    e = timed(lambda: model.encode(x))
    r = timed(lambda: model.encode(x, rd_lambda=0.1))
print(f"{sys.argv[1]} encode {e[0]:.3f} ms ({e[1]:.3f}-{e[2]:.3f}); rd_lambda=0.1 {r[0]:.3f} ms ({r[1]:.3f}-{r[2]:.3f})")
