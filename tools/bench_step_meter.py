#!/usr/bin/env python3
"""What mcquic_amd.monitor.StepMeter adds to a training step: the post graph of parallel.GraphedTrainStep (update + frequency EMA) with and
without `meter=`, on the configuration tools/bench_train.py --graphed trains (Compressor(128, 2, [8192, 2048, 512]), batch 8, 256 x 256
crops, torch.optim.SGD(lr=1e-6)), and the meter's two launches alone as a captured graph.  Without a meter the step's post graph is the
one it was before the meter existed, launch for launch.  Both steps live in one process; the arms alternate inside every round (device
events over --iters replays; median of --rounds rounds, [min, max]).  Prints one JSON line.

    python tools/bench_step_meter.py [--iters 200] [--rounds 7]
"""
import argparse
import copy
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcquic_amd import Compressor, monitor, parallel  # noqa: E402
from bench_sgd import timed  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--crop", type=int, default=256)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(3407)
    plain = Compressor(128, 2, [8192, 2048, 512]).to(dev).train()
    metered = copy.deepcopy(plain)
    x = (torch.rand((args.batch, 3, args.crop, args.crop), generator=torch.Generator().manual_seed(0)) * 2 - 1).to(dev)
    meter = monitor.StepMeter(metered, capacity=1024, pixels=args.batch * args.crop * args.crop)
    steps = {"without": parallel.GraphedTrainStep(plain, torch.optim.SGD(plain.parameters(), lr=1e-6), x),
             "with": parallel.GraphedTrainStep(metered, torch.optim.SGD(metered.parameters(), lr=1e-6), x, meter=meter)}
    for s in steps.values():
        assert s.post is not None
        for _ in range(2):
            s(x)
    alone = monitor.StepMeter(metered, capacity=1024, pixels=args.batch * args.crop * args.crop)
    alone.prepare()
    alone.warm()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        alone.update(steps["with"].loss, steps["with"].counts)
    arms = {"post_without": steps["without"].post.replay, "post_with": steps["with"].post.replay, "meter_alone": graph.replay,
            "step_without": lambda: steps["without"](x), "step_with": lambda: steps["with"](x)}
    times = {k: [] for k in arms}
    for _ in range(args.rounds):
        for k, fn in arms.items():                            # alternating: every round visits every arm
            times[k].append(timed(fn, args.iters if k.startswith(("post", "meter")) else max(5, args.iters // 10)))
    out = {"metric": "us per replay (device events; median of alternating rounds, [min, max]); post = the update's graph, step = the whole call",
           "iters": args.iters, "rounds": args.rounds, "batch": args.batch, "crop": args.crop, "rows_recorded": int(meter.read()["count"])}
    for k, v in times.items():
        out[k] = {"us": round(statistics.median(v) * 1e3, 2), "range": [round(min(v) * 1e3, 2), round(max(v) * 1e3, 2)]}
    out["post_delta_us"] = round(statistics.median([a - b for a, b in zip(times["post_with"], times["post_without"])]) * 1e3, 2)
    out["step_delta_us"] = round(statistics.median([a - b for a, b in zip(times["step_with"], times["step_without"])]) * 1e3, 2)
    print(json.dumps(out))
    for s in steps.values():
        s.close()
