"""Adaptive quantisation on the synthetic qp = 2 model (docs/experiments.md section 34).  One MI355X.

    python tools/bench_activity.py [OUT.json]

  launches   `ops.activity_cells` and `ops.activity_weights` at 32 x 768x512 and 1 x 768x512: device events around ONE Python call
             (allocation and launch), 10 warm-up + 30 timed, median (min - max) in microseconds
  encode     `encode(x, rd_lambda=0.1, rd_map=given)` -- the path the parent commit has, unchanged here -- against
             `encode(x, rd_lambda=0.1, aq=0.5)` at 32 x 768x512, alternating A B A: the two A rows are the map path's own spread
  rate       bits per pixel by the coder's tables at rd_lambda = 0.1 with aq off, 0.5 and 1.0, on images whose texture amplitude
             varies over the picture; the tables come from the plain codes' histogram (counts + 1), since the synthetic frequency EMAs
             are uniform and lambda would be without effect.  Random-init weights: rate only, nothing about quality."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcquic_amd import ops
from mcquic_amd.utils import synthetic

dev = torch.device("cuda")


def per_call(fn, reps=30, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return [round(v, 1) for v in (statistics.median(ts), min(ts), max(ts))]


def per_encode(fn, reps=7, warm=3, inner=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) / inner)
    return [round(v, 3) for v in (statistics.median(ts), min(ts), max(ts))]


out = {}
with torch.no_grad():
    for n in (32, 1):
        x = synthetic.bench_images(0, n).to(dev)
        a, mask, _ = ops.activity_cells(x)
        lam = torch.rand(n, device=dev)
        out[f"cells_n{n}_us"] = per_call(lambda: ops.activity_cells(x))
        out[f"weights_n{n}_us"] = per_call(lambda: ops.activity_weights(a, mask, 0.5, 2.0))
        out[f"weights_lam_n{n}_us"] = per_call(lambda: ops.activity_weights(a, mask, 0.5, 2.0, lam=lam))
        print(n, {k: v for k, v in out.items() if k.endswith(f"n{n}_us")}, flush=True)

    model = synthetic.bench_model().to(dev)
    # images with something for the map to say: uniform noise whose amplitude falls from 1 to 2^-6 down the picture, per image shifted
    x = synthetic.bench_images(0, 32).to(dev)
    rows = torch.arange(synthetic.HEIGHT, device=dev, dtype=torch.float32)[None, None, :, None]
    shift = torch.arange(32, device=dev, dtype=torch.float32)[:, None, None, None] * 24
    x = (x * torch.exp2(-6.0 * ((rows + shift) % synthetic.HEIGHT) / synthetic.HEIGHT)).contiguous()
    plain = model.encode(x)
    for f, c, k in zip(model._quantizer._entropyCoder._freqEMA, plain, synthetic.QP2_MODEL["k"]):
        counts = torch.stack([torch.bincount(c[:, g].flatten(), minlength=k) for g in range(c.shape[1])]).float() + 1
        f.copy_(counts / counts.sum(-1, keepdim=True))
    given = model.activityWeights(x, 0.5)
    assert all(torch.equal(s, t) for s, t in zip(model.encode(x, rd_lambda=0.1, aq=0.5), model.encode(x, rd_lambda=0.1, rd_map=given)))
    out["encode_rd_map_ms_first"] = per_encode(lambda: model.encode(x, rd_lambda=0.1, rd_map=given))
    out["encode_aq_ms"] = per_encode(lambda: model.encode(x, rd_lambda=0.1, aq=0.5))
    out["encode_rd_map_ms_second"] = per_encode(lambda: model.encode(x, rd_lambda=0.1, rd_map=given))
    print({k: v for k, v in out.items() if k.startswith("encode")}, flush=True)

    pixels = float(synthetic.HEIGHT * synthetic.WIDTH)
    out["bpp_plain"] = float(model.codeBits(plain).sum(-1).mean()) / pixels
    for name, kw in (("aq_off", {}), ("aq_0.5", dict(aq=0.5)), ("aq_1.0", dict(aq=1.0))):
        codes = model.encode(x, rd_lambda=0.1, **kw)
        bits = model.codeBits(codes)
        out[f"bpp_{name}"] = float(bits.sum(-1).mean()) / pixels
        out[f"bpp_{name}_levels"] = [float(v) / pixels for v in bits.mean(0)]
    w = model.activityWeights(x, 1.0)
    out["w_range_aq_1.0"] = [float(w.min()), float(w.max())]
    print({k: v for k, v in out.items() if k.startswith("bpp") or k.startswith("w_")}, flush=True)
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
