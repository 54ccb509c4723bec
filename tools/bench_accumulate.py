#!/usr/bin/env python3
"""Gradient accumulation (parallel.GraphedTrainStep(accumulate=k)) measured, for docs/experiments.md:

  --gather   mcq_gather_accum_flat_f32 beside mcq_gather_flat_f32, isolated, on the three slices of the qp=2 model (decoder / quantizer /
             encoder: the tables the segmented step builds), device events around --iters launches: us, bytes moved (copy: read + write;
             accumulating past phase 0: two reads + write) and the share of the HBM rate.
  --step     the configs[4] step (8 x 256 x 256, Adam with a tensor rate, max_grad_norm=4.0: tools/train_rehearsal.py's default step):
             T = a call with accumulate=1, P = its post graph alone, then a call for every k of --ks against k (T - P) + P.

    python tools/bench_accumulate.py --gather --step [--iters 30] [--ks 2,4,8] [--out profiles/accumulate.json]
Peak memory per k: tools/train_rehearsal.py --accumulate K (one process per k)."""
import argparse
import json
import os
import sys

os.environ.setdefault("DEBUG_CLR_GRAPH_PACKET_CAPTURE", "0")
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

HBM_ACHIEVABLE, HBM_PEAK = 6.3e12, 8.0e12      # bytes/s: streaming rate reached in practice / the specification's peak


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
    return s.elapsed_time(e) * 1e3 / iters      # us


def gather(dev, iters):
    from mcquic_amd import Compressor, _lib, ops
    from mcquic_amd.tensor_list import ChunkTable
    lib = _lib.load()
    model = Compressor(128, 2, [8192, 2048, 512])
    taken, groups = set(), []
    for stage in (model._decoder, model._quantizer):
        g = [p for p in stage.parameters() if p.requires_grad and id(p) not in taken]
        taken.update(id(p) for p in g)
        groups.append(g)
    groups.append([p for p in model.parameters() if p.requires_grad and id(p) not in taken])
    flat = torch.zeros(sum(p.numel() for g in groups for p in g), device=dev)
    phase = torch.zeros(1, dtype=torch.int32, device=dev)
    rows, off = [], 0
    for name, g in zip(("decoder", "quantizer", "encoder"), groups):
        sizes = [p.numel() for p in g]
        n = sum(sizes)
        srcs = [torch.randn(s, device=dev) for s in sizes]
        table = ChunkTable(sizes, dev)
        offs = torch.tensor([0] + sizes[:-1], dtype=torch.int64).cumsum(0).to(dev)
        ptrs = torch.tensor([s.data_ptr() for s in srcs], dtype=torch.int64).to(dev)
        sl = flat[off: off + n]
        off += n
        stream = torch.cuda.current_stream().cuda_stream

        def copy():
            lib.mcq_gather_flat_f32(ptrs.data_ptr(), sl.data_ptr(), offs.data_ptr(), table.numel.data_ptr(), table.blk_tensor.data_ptr(),
                                    table.blk_first.data_ptr(), table.nblocks, stream)
        row = {"slice": name, "tensors": len(sizes), "floats": n, "mb": round(4 * n / 1e6, 1),
               "unaligned_slices": sum(1 for o in offs.tolist() if o % 4)}
        us = timed(copy, iters)
        row["copy"] = {"us": round(us, 1), "tb_per_s": round(8 * n / us / 1e6, 3), "share_of_6.3": round(8 * n / us * 1e6 / HBM_ACHIEVABLE, 3)}
        for tag, ph, traffic in (("accum_phase0", 0, 8), ("accum_mid", 1, 12), ("accum_last", 3, 12)):
            phase.fill_(ph)
            sl.zero_()
            us = timed(lambda: ops.gather_accum_flat_(ptrs, sl, offs, table, phase, 4), iters)
            row[tag] = {"us": round(us, 1), "tb_per_s": round(traffic * n / us / 1e6, 3),
                        "share_of_6.3": round(traffic * n / us * 1e6 / HBM_ACHIEVABLE, 3), "share_of_8.0": round(traffic * n / us * 1e6 / HBM_PEAK, 3)}
        rows.append(row)
        del srcs
    return rows


def step(dev, iters, ks):
    from mcquic_amd import Compressor, parallel
    gen = torch.Generator(device=dev).manual_seed(1)
    out = {}

    def build(k):
        torch.manual_seed(3407)
        model = Compressor(128, 2, [8192, 2048, 512]).to(dev).train()
        opt = torch.optim.Adam(model.parameters(), lr=torch.tensor(1e-4, device=dev), capturable=True)
        x = (torch.rand((8 * k, 3, 256, 256), generator=gen, device=dev) * 2 - 1)
        return parallel.GraphedTrainStep(model, opt, x[:8], max_grad_norm=4.0, accumulate=k), x
    s, x = build(1)
    out["T_us"] = round(timed(lambda: s(x), iters), 1)
    out["P_us"] = round(timed(s.post.replay, iters), 1)
    out["T_again_us"] = round(timed(lambda: s(x), iters), 1)      # (the spread of the same measurement)
    s.close()
    del s
    torch.cuda.empty_cache()
    T, P = out["T_us"], out["P_us"]
    out["calls"] = []
    for k in ks:
        s, x = build(k)
        us = timed(lambda: s(x), iters)
        model_us = k * (T - P) + P
        out["calls"].append({"accumulate": k, "call_us": round(us, 1), "k(T-P)+P_us": round(model_us, 1), "overhead_us": round(us - model_us, 1),
                             "overhead_per_micro_step_us": round((us - model_us) / k, 1), "loss": float(s.loss)})
        s.close()
        del s
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gather", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--ks", default="2,4,8")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {}
    if args.gather:
        out["gather"] = gather(dev, args.iters)
    if args.step:
        out["step"] = step(dev, args.iters, [int(k) for k in args.ks.split(",")])
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
