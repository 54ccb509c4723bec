#!/usr/bin/env python3
"""The SGD update alone on the qp=2 model's tensors (Compressor(128, 2, [8192, 2048, 512]): 666 tensors, 50.6 M float32):
mcquic_amd.optim.SGD (csrc/sgd.hip) beside torch.optim.SGD(foreach=True), without momentum, with momentum 0.9, and with clipping to
4.0 plus the non-finite guard (torch: clip_grad_norm_ in front of the step, which has no guard).  Every variant is timed twice with
device events -- called eagerly (host work included) and as a captured graph's replay (what a captured training step pays) -- in
rounds that alternate the variants; the median round is reported with the spread.  The gradients are slices of one flat buffer, as
parallel.GraphedTrainStep hands them over (4-byte aligned: the dword path), or one allocation per tensor with --own-grads (16-byte
aligned: the vector path).  Prints one JSON line.

    python tools/bench_sgd.py [--iters 100] [--rounds 5] [--own-grads]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcquic_amd import Compressor, optim  # noqa: E402


def timed(fn, iters):
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def variant(dev, shapes, flat_grads, own, momentum, guarded):
    """(eager call, graph replay) of one optimizer on its own copy of the parameters; lr 0 keeps the values where they are."""
    g = torch.Generator().manual_seed(0)
    params = [torch.nn.Parameter((torch.randn(s, generator=g) * 0.05).to(dev)) for s in shapes]
    n = sum(p.numel() for p in params)
    flat = (torch.randn(n, generator=g) * 1e-3).to(dev)
    off = 0
    for p in params:
        p.grad = flat[off: off + p.numel()].view_as(p) if flat_grads else flat[off: off + p.numel()].view_as(p).clone()
        off += p.numel()
    if own:
        opt = optim.SGD(params, lr=0.0, momentum=momentum, **(dict(max_grad_norm=4.0, skip_nonfinite=True) if guarded else {}))
        call = opt.step
    else:
        opt = torch.optim.SGD(params, lr=0.0, momentum=momentum, foreach=True)

        def call():
            if guarded:
                torch.nn.utils.clip_grad_norm_(params, 4.0, foreach=True)
            opt.step()
    for _ in range(3):                                        # state, tables, code objects
        call()
    if own:
        opt.prepare()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        call()
    graph.replay()
    torch.cuda.synchronize()
    return call, graph.replay, n


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--own-grads", action="store_true", help="one allocation per gradient (16-byte aligned) instead of slices of a flat buffer")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    shapes = [tuple(p.shape) for p in Compressor(128, 2, [8192, 2048, 512]).parameters() if p.requires_grad]
    names = {"torch_m0": (False, 0.0, False), "own_m0": (True, 0.0, False), "torch_m0.9": (False, 0.9, False), "own_m0.9": (True, 0.9, False),
             "torch_m0.9_clip": (False, 0.9, True), "own_m0.9_clip_guard": (True, 0.9, True)}
    made = {k: variant(dev, shapes, not args.own_grads, *v) for k, v in names.items()}
    times = {k: {"eager": [], "replay": []} for k in names}
    for _ in range(args.rounds):
        for k, (call, replay, _) in made.items():             # alternating: every round visits every variant
            times[k]["eager"].append(timed(call, args.iters))
            times[k]["replay"].append(timed(replay, args.iters))
    n = made["own_m0"][2]
    out = {"metric": "SGD update of the qp=2 model, ms per call (device events over --iters calls; median of --rounds alternating rounds, [min, max])",
           "tensors": len(shapes), "elements": n, "gradients": "one allocation each" if args.own_grads else "slices of one flat buffer",
           "iters": args.iters, "rounds": args.rounds}
    for k, t in times.items():
        out[k] = {mode: {"ms": round(statistics.median(v), 4), "range": [round(min(v), 4), round(max(v), 4)]} for mode, v in t.items()}
    # bytes the update itself has to move (parameters read + written, gradients read, buffer read + written; the norm's pass reads the gradients again)
    for k, per in (("own_m0", 12), ("own_m0.9", 20), ("own_m0.9_clip_guard", 24)):
        out[k]["bytes_per_element"] = per
        out[k]["replay_tb_per_s"] = round(per * n / (out[k]["replay"]["ms"] * 1e-3) / 1e12, 3)
    print(json.dumps(out))
