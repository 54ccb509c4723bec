#!/usr/bin/env python3
"""The k-means kernels (csrc/vq_kmeans.hip) beside the assignment they follow, at the three qp=2 level shapes of the flagship
batch (32 x 768x512: level 0 is m=2, d=64, k=8192, 49 152 vectors per group), device-event timing in one process; then whole
`kmeans.fit_codebooks` iterations of the qp=2 model on one batch of 8 x 256x256.  Prints one JSON line."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcquic_amd import Compressor, kmeans, ops  # noqa: E402


def timed(fn, iters=20, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return round(s.elapsed_time(e) / iters, 4)


def leaf(m, k, d, n, h, w, dev):
    g = torch.Generator().manual_seed(0)
    x = (torch.randn((n, m * d, h, w), generator=g) * 0.1).to(dev)
    book = (torch.randn((m, k, d), generator=g) * (2 / (5 * d)) ** 0.5).to(dev)
    ops.vq_kmeans_seed(x, book, torch.tensor([0, 0], dtype=torch.int64, device=dev))          # codewords among the data: every cluster is used
    cb = ops.PackedCodebook(book)
    codes = ops.vq_assign(x, cb)
    acc = ops.KMeansAcc(m, k, d, dev)
    ops.vq_kmeans_accumulate(x, codes, acc)
    rng = torch.tensor([1, 0], dtype=torch.int64, device=dev)
    scratch = book.clone()
    out = {"shape": f"m={m} k={k} d={d} vectors/group={n * h * w}",
           "largest_cluster": int(acc.counts.max()), "empty": int((acc.counts == 0).sum()),
           "assign_ms": timed(lambda: ops.vq_assign(x, cb)),
           "accumulate_ms": timed(lambda: ops.vq_kmeans_accumulate(x, codes, acc)),
           "update_ms": timed(lambda: ops.vq_kmeans_update(scratch, acc)),
           "seed_all_ms": timed(lambda: ops.vq_kmeans_seed(x, scratch, rng)),
           "zero_ms": timed(acc.zero_)}
    return out


def fit(dev):
    torch.manual_seed(0)
    model = Compressor(128, 2, [8192, 2048, 512]).eval().to(dev)
    g = torch.Generator().manual_seed(1)
    batches = [(torch.rand((8, 3, 256, 256), generator=g) * 2 - 1).to(dev)]
    wall = {}
    for iters in (1, 1, 5):                                   # (the first call warms up: weight packing, allocator)
        torch.cuda.synchronize()
        t = time.perf_counter()
        kmeans.fit_codebooks(model, batches, iters=iters, seed=0)
        torch.cuda.synchronize()
        wall[iters] = (time.perf_counter() - t) * 1e3
    return {"model": "Compressor(128, 2, [8192, 2048, 512]), one batch of 8 x 3 x 256 x 256, all three levels",
            "fit_iters1_ms": round(wall[1], 3), "fit_iters5_ms": round(wall[5], 3), "per_iteration_ms": round((wall[5] - wall[1]) / 4, 3)}


if __name__ == "__main__":
    dev = torch.device("cuda:0")
    print(json.dumps({"metric": "k-means kernels beside mcq_vq_assign_f32 (device events), and whole fit iterations (host clock + sync)",
                      "qp2_levels": [leaf(2, 8192, 64, 32, 48, 32, dev), leaf(2, 2048, 64, 32, 24, 16, dev), leaf(2, 512, 64, 32, 12, 8, dev)],
                      "few_codewords": leaf(2, 8, 64, 32, 48, 32, dev),
                      "fit": fit(dev)}))
