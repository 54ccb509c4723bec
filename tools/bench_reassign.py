#!/usr/bin/env python3
"""What `GraphedTrainStep(..., reassign=CodebookReassign(...))` adds to the post graph, one process per arm so that a checkout of the
parent commit (with its own library) can be an arm too: the README's training configuration (Compressor(128, 2, [8192, 2048, 512]),
batch 8, 256 x 256, mcquic_amd.optim.Adam), 7 rounds x 200 replays of the post graph under device events, as tools/bench_param_stats.py
times the statistics; prints one JSON line with the median [min, max] in us.

    python tools/bench_reassign.py --arm plain                 # the keyword is not passed at all: runs on a tree without CodebookReassign
    python tools/bench_reassign.py --arm none                  # reassign=None
    python tools/bench_reassign.py --arm reassign --freq 20000 # no replay fires: two launches that read the decision and return
    python tools/bench_reassign.py --arm reassign --freq 1     # every replay fires  [--dead 0.6: that share of every `_freqEMA` row is zero]
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
    ap.add_argument("--arm", choices=["plain", "none", "reassign"], required=True)
    ap.add_argument("--freq", type=int, default=20000)
    ap.add_argument("--dead", type=float, default=0.0)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(3407)
    model = Compressor(128, 2, [8192, 2048, 512]).to(dev).train()
    if args.dead > 0:
        with torch.no_grad():
            for f in model._quantizer._entropyCoder._freqEMA:
                f.mul_((torch.rand(f.shape, generator=torch.Generator().manual_seed(1)) >= args.dead).to(dev))
    x = (torch.rand((8, 3, 256, 256), generator=torch.Generator().manual_seed(0)) * 2 - 1).to(dev)
    opt = optim.Adam(model.parameters(), lr=1e-6)
    extra, re = {}, None
    if args.arm == "reassign":
        import mcquic_amd
        re = mcquic_amd.CodebookReassign(model, freq=args.freq)
    if args.arm != "plain":
        extra["reassign"] = re
    step = parallel.GraphedTrainStep(model, opt, x, **extra)
    assert step.post is not None
    for _ in range(3):
        step(x)
    times = [timed(step.post.replay, args.iters) * 1e3 for _ in range(args.rounds)]
    whole = timed(lambda: step(x), 20) * 1e3
    out = {"arm": args.arm, "freq": args.freq if re is not None else None, "dead": args.dead,
           "post_us": round(statistics.median(times), 2), "range": [round(min(times), 2), round(max(times), 2)], "step_us": round(whole, 1)}
    if re is not None:
        out.update({k: v for k, v in re.read().items() if k in ("count", "fired", "moved", "Stat/ReAssignProportion")})
    print(json.dumps(out))
    step.close()
