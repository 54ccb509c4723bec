#!/usr/bin/env python3
"""What `GraphedTrainStep(..., skip_nonfinite=True)` adds to the post graph, one process per arm so that a checkout of the parent commit
(with its own library) can be an arm too: the rehearsal's step (Compressor(128, 2, [8192, 2048, 512]), batch 8, 256 x 256,
mcquic_amd.optim.Adam with a device learning rate, the step's clipping at 4.0, EMA + cosine scheduler), 7 rounds x 200 replays of the
post graph under device events; prints one JSON line with the median [min, max] in us.

    python tools/bench_step_guard.py --arm plain     # the keyword is not passed at all: runs on a tree without the guard
    python tools/bench_step_guard.py --arm off       # skip_nonfinite=False
    python tools/bench_step_guard.py --arm on        # skip_nonfinite=True  [--no-clip: the guard reduces the flat buffer itself]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcquic_amd import Compressor, optim, parallel, schedule  # noqa: E402
from bench_sgd import timed  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--arm", choices=["plain", "off", "on"], required=True)
    ap.add_argument("--no-clip", action="store_true")
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(3407)
    model = Compressor(128, 2, [8192, 2048, 512]).to(dev).train()
    x = (torch.rand((8, 3, 256, 256), generator=torch.Generator().manual_seed(0)) * 2 - 1).to(dev)
    opt = optim.Adam(model.parameters(), lr=torch.tensor(1e-6, device=dev))
    extra = {} if args.arm == "plain" else {"skip_nonfinite": args.arm == "on"}
    step = parallel.GraphedTrainStep(model, opt, x, max_grad_norm=None if args.no_clip else 4.0, ema=optim.EMA(model, decay=0.9999),
                                     scheduler=schedule.CosineAnnealingWarmupRestarts(opt, 100000, warmup_steps=2000, lrScaleRatio=0.0), **extra)
    assert step.post is not None
    for _ in range(3):
        step(x)
    times = [timed(step.post.replay, args.iters) * 1e3 for _ in range(args.rounds)]
    whole = timed(lambda: step(x), 20) * 1e3
    out = {"arm": args.arm, "clip": not args.no_clip, "post_us": round(statistics.median(times), 2), "range": [round(min(times), 2), round(max(times), 2)],
           "step_us": round(whole, 1), "skipped": int(step.guard.skipped) if getattr(step, "guard", None) is not None else None}
    print(json.dumps(out))
    step.close()
