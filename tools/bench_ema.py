#!/usr/bin/env python3
"""The weight average alone on the qp=2 model's tensors (Compressor(128, 2, [8192, 2048, 512]): 666 tensors, 50.6 M float32):
mcquic_amd.optim.EMA.update() and .swap() (csrc/ema.hip) beside torch._foreach_lerp_ over the same tensors (what
torch.optim.swa_utils.get_ema_multi_avg_fn runs) and, in the same run, mcquic_amd.optim.Adam's update -- the EMA update moves 12 of the
Adam launch's 28 bytes per element, so its time is reported as a share of that launch (3/7 if both reach the same bandwidth).  Every
variant is timed twice with device events -- called eagerly (host work included) and as a captured graph's replay (what a captured
training step pays) -- in rounds that alternate the variants; the median round is reported with the spread.  Prints one JSON line.

    python tools/bench_ema.py [--iters 100] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcquic_amd import Compressor, optim  # noqa: E402
from bench_sgd import timed  # noqa: E402

HBM_PEAK_TB_S = 8.0                                            # MI355X, spec


def variant(dev, shapes, kind):
    """(eager call, graph replay, elements) of one variant on its own copy of the parameters."""
    g = torch.Generator().manual_seed(0)
    params = [torch.nn.Parameter((torch.randn(s, generator=g) * 0.05).to(dev)) for s in shapes]
    n = sum(p.numel() for p in params)
    if kind == "adam":
        flat = (torch.randn(n, generator=g) * 1e-3).to(dev)
        off = 0
        for p in params:
            p.grad = flat[off: off + p.numel()].view_as(p).clone()
            off += p.numel()
        opt = optim.Adam(params, lr=0.0)
        call, prepare = opt.step, opt.prepare
    elif kind == "torch_lerp":
        avg, live = [p.detach().clone() for p in params], [p.detach() for p in params]

        def call():
            torch._foreach_lerp_(avg, live, 1.0 - 0.9999)
        prepare = None
    else:
        ema = optim.EMA(params, decay=0.9999, warmup=True)
        call, prepare = (ema.update if kind == "ema_update" else ema.swap), ema.prepare
    for _ in range(4):                                        # state, tables, code objects (an even count: the swap ends where it began)
        call()
    if prepare is not None:
        prepare()
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
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    shapes = [tuple(p.shape) for p in Compressor(128, 2, [8192, 2048, 512]).parameters() if p.requires_grad]
    kinds = ["ema_update", "ema_swap", "torch_lerp", "adam"]
    made = {k: variant(dev, shapes, k) for k in kinds}
    times = {k: {"eager": [], "replay": []} for k in kinds}
    for _ in range(args.rounds):
        for k, (call, replay, _) in made.items():             # alternating: every round visits every variant
            times[k]["eager"].append(timed(call, args.iters))
            times[k]["replay"].append(timed(replay, args.iters))
    n = made["ema_update"][2]
    out = {"metric": "weight average of the qp=2 model, us per call (device events over --iters calls; median of --rounds alternating rounds, [min, max]); "
                     "ema_update includes its one-workgroup scalar kernel, adam likewise",
           "tensors": len(shapes), "elements": n, "iters": args.iters, "rounds": args.rounds, "hbm_peak_tb_per_s": HBM_PEAK_TB_S}
    for k, t in times.items():
        out[k] = {mode: {"us": round(statistics.median(v) * 1e3, 2), "range": [round(min(v) * 1e3, 2), round(max(v) * 1e3, 2)]} for mode, v in t.items()}
    # bytes each has to move per element: update reads p and avg, writes avg; swap reads and writes both; Adam reads p, g, m, v, writes p, m, v
    for k, per in (("ema_update", 12), ("ema_swap", 16), ("torch_lerp", 12), ("adam", 28)):
        tb = per * n / (out[k]["replay"]["us"] * 1e-6) / 1e12
        out[k].update(bytes_per_element=per, replay_tb_per_s=round(tb, 3), share_of_hbm_peak=round(tb / HBM_PEAK_TB_S, 3))
    out["ema_update_share_of_adam_replay"] = round(out["ema_update"]["replay"]["us"] / out["adam"]["replay"]["us"], 3)
    out["bytes_share_of_adam"] = round(12 / 28, 3)
    print(json.dumps(out))
