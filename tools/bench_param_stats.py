#!/usr/bin/env python3
"""What `GraphedTrainStep(..., stats=monitor.ParamStats(...))` adds to the post graph, one process per arm so that a checkout of the
parent commit (with its own library) can be an arm too: the README's training configuration (Compressor(128, 2, [8192, 2048, 512]),
batch 8, 256 x 256, mcquic_amd.optim.Adam), 7 rounds x 200 replays of the post graph under device events, as tools/bench_step_guard.py
times the guard; prints one JSON line with the median [min, max] in us.

    python tools/bench_param_stats.py --arm plain              # the keyword is not passed at all: runs on a tree without ParamStats
    python tools/bench_param_stats.py --arm none               # stats=None
    python tools/bench_param_stats.py --arm stats --every 100  # 2 of every 200 replays are sampled
    python tools/bench_param_stats.py --arm stats --every 1    # every replay is sampled  [--no-updates: no shadow, no `before` launch]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcquic_amd import Compressor, optim, parallel  # noqa: E402
from bench_sgd import timed  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=["plain", "none", "stats"], required=True)
    ap.add_argument("--every", type=int, default=1)
    ap.add_argument("--no-updates", action="store_true")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(3407)
    model = Compressor(128, 2, [8192, 2048, 512]).to(dev).train()
    x = (torch.rand((8, 3, 256, 256), generator=torch.Generator().manual_seed(0)) * 2 - 1).to(dev)
    opt = optim.Adam(model.parameters(), lr=1e-6)
    extra, stats = {}, None
    if args.arm == "stats":
        from mcquic_amd import monitor
        stats = monitor.ParamStats(model, capacity=64, every=args.every, updates=not args.no_updates)
    if args.arm != "plain":
        extra["stats"] = stats
    step = parallel.GraphedTrainStep(model, opt, x, **extra)
    assert step.post is not None
    for _ in range(3):
        step(x)
    times = [timed(step.post.replay, args.iters) * 1e3 for _ in range(args.rounds)]
    whole = timed(lambda: step(x), 20) * 1e3
    out = {"arm": args.arm, "every": args.every if stats is not None else None, "updates": stats.updates if stats is not None else None,
           "post_us": round(statistics.median(times), 2), "range": [round(min(times), 2), round(max(times), 2)], "step_us": round(whole, 1),
           "rows": int(stats.read()["count"]) if stats is not None else None}
    print(json.dumps(out))
    step.close()
