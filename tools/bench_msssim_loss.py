#!/usr/bin/env python3
"""Time of the MS-SSIM training loss (csrc/msssim_loss.hip): forward, backward (da only, and da + db) and forward + backward,
with device events, next to the uint8 validation metric (csrc/metrics.hip) at the same shape.

    python tools/bench_msssim_loss.py [--iters 20] [--json out.json]

Shapes: 8 x 3 x 256 x 256 (the configs[4] training batch) and 32 x 3 x 768 x 512 (the headline geometry).  Bytes and FLOPs
are computed from the shapes: the forward reads both inputs of every level once and writes the pooled levels; the blur is
5 moments x 2 passes x 11 taps x 2 ops per map pixel.  The backward recomputes the moments (same blur), writes and reads back
3 gradient planes per map pixel (5 with db) and blurs them again (3 planes x 2 passes x 11 taps x 2 ops per image pixel).
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcquic_amd import ops  # noqa: E402


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def levels(h, w):
    out = []
    for _ in range(5):
        out.append((h, w))
        ph, pw = h % 2, w % 2
        h, w = (h + 2 * ph - 2) // 2 + 1, (w + 2 * pw - 2) // 2 + 1
    return out


def counts(n, c, h, w):
    planes = n * c
    lv = levels(h, w)
    px = sum(a * b for a, b in lv) * planes
    mp = sum((a - 10) * (b - 10) for a, b in lv) * planes
    pooled = sum(a * b for a, b in lv[1:]) * planes
    fwd_bytes = 4 * (2 * px + 2 * pooled)
    fwd_flops = mp * 5 * 2 * 11 * 2
    bwd_bytes = 4 * (2 * px + 3 * mp * 2 + 2 * px + pooled)           # moments' inputs, g planes out + in, x / y again, dx out
    bwd_flops = fwd_flops + px * 3 * 2 * 11 * 2
    return fwd_bytes, fwd_flops, bwd_bytes, bwd_flops


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for (n, c, h, w) in [(8, 3, 256, 256), (32, 3, 768, 512)]:
        g = torch.Generator(device=dev).manual_seed(n)
        a = torch.rand((n, c, h, w), device=dev, generator=g) * 2 - 1
        b = (a + 0.05 * torch.randn((n, c, h, w), device=dev, generator=g)).clamp(-1, 1)
        one = torch.ones((), device=dev)
        loss, values, saved = ops.ms_ssim_loss(a, b)
        fwd = timed(lambda: ops.ms_ssim_loss(a, b), args.iters)
        bwd = timed(lambda: ops.ms_ssim_loss_bwd(a, b, values, saved, one), args.iters)
        bwd2 = timed(lambda: ops.ms_ssim_loss_bwd(a, b, values, saved, one, want_db=True), args.iters)

        def both():
            _, v, s = ops.ms_ssim_loss(a, b)
            ops.ms_ssim_loss_bwd(a, b, v, s, one)
        total = timed(both, args.iters)
        au8 = ((a + 1) * 127.5).round().to(torch.uint8)
        bu8 = ((b + 1) * 127.5).round().to(torch.uint8)
        u8 = timed(lambda: ops.ms_ssim(au8, bu8), args.iters)
        fb, ff, bb, bf = counts(n, c, h, w)
        row = {"shape": [n, c, h, w], "forward_ms": round(fwd, 4), "backward_ms": round(bwd, 4), "backward_with_db_ms": round(bwd2, 4),
               "forward_backward_ms": round(total, 4), "u8_metric_ms": round(u8, 4),
               "forward_over_u8": round(fwd / u8, 3), "backward_over_forward": round(bwd / fwd, 3),
               "forward_bytes": fb, "forward_flops": ff, "backward_bytes": bb, "backward_flops": bf,
               "forward_GBps": round(fb / fwd / 1e6, 1), "forward_TFLOPs": round(ff / fwd / 1e9, 2),
               "backward_GBps": round(bb / bwd / 1e6, 1), "backward_TFLOPs": round(bf / bwd / 1e9, 2)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
