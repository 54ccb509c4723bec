"""`ops.vq_assign_rate_map` against `ops.vq_assign` at the three qp = 2 levels (32 images and one) and at BASELINE configs[3]
(M = 4, K = 4096, D = 256, 32 x 48x32), docs/experiments.md section 31.  One MI355X.

    python tools/bench_rate_map.py            per-CALL times (device events around one Python call: allocation, launch, fold), then encode
                                              with and without rd_map and the two target-rate searches at 32 x 768x512
    rocprofv3 --kernel-trace -d DIR -o kt -- python tools/bench_rate_map.py trace
    python profiles/kernel_stats.py DIR/kt_results.db
                                              KERNEL times: `trace` alternates the plain and the RATE launch 40 times per shape; the
                                              summary lists every instance per launch grid"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mcquic_amd import ops, Compressor
dev = torch.device("cuda")
def timed(fn, reps=30, warm=10):
    for _ in range(warm): fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return statistics.median(ts), ts[0], ts[-1]
out = {}
g = torch.Generator(device="cpu").manual_seed(1)
TRACE = sys.argv[1:] == ["trace"]
SHAPES = [(n, 2, 64, k, h, w) for n in (32, 1) for (k, h, w) in ((8192, 48, 32), (2048, 24, 16), (512, 12, 8))] + [(32, 4, 256, 4096, 48, 32)]
for (n, m, d, k, h, w) in SHAPES:
    if True:
        x = torch.randn((n, m * d, h, w), generator=g).to(dev)
        cb = torch.randn((m, k, d), generator=g).to(dev)
        pmf = torch.rand((m, k), generator=g).to(dev) + 0.01
        cdf, _ = ops.pmf_to_quantized_cdf_dev([pmf / pmf.sum(-1, keepdim=True)])
        pack, bits = ops.PackedCodebook(cb), ops.pack_bits(cdf[0])
        lam = torch.rand((n, h, w), generator=g).to(dev)
        if TRACE:
            for _ in range(40):
                ops.vq_assign(x, pack)
                ops.vq_assign_rate_map(x, pack, bits, lam)
            torch.cuda.synchronize()
            continue
        a = timed(lambda: ops.vq_assign(x, pack))
        b = timed(lambda: ops.vq_assign_rate_map(x, pack, bits, lam))
        lam_n = lam[:, 0, 0].contiguous()
        c = timed(lambda: ops.vq_assign_rate_map(x, pack, bits, lam_n))
        out[f"n{n}_m{m}_d{d}_k{k}_{h}x{w}"] = dict(plain_us=a, map_us=b, per_image_us=c, ratio=b[0] / a[0])
        print(f"n{n} m{m} d{d} k{k} {h}x{w} per call: plain {a[0]:.1f} us, grid map {b[0]:.1f} us ({b[0] / a[0]:.3f}x), per image {c[0]:.1f} us", flush=True)
if TRACE:
    sys.exit(0)
model = Compressor(192, 2, [8192, 2048, 512]).eval().to(dev)
with torch.no_grad():
    for f in model._quantizer._entropyCoder._freqEMA:
        f.copy_(torch.rand(f.shape, generator=g).to(dev) + 0.01)
x = torch.rand((32, 3, 512, 768), generator=g).to(dev) * 2 - 1
with torch.no_grad():
    plain = model.encode(x)
    bpp0 = float(model.codeBits(plain).sum()) / (32 * 512 * 768)
    e = timed(lambda: model.encode(x), reps=5, warm=2)
    r = timed(lambda: model.encode(x, rd_lambda=0.1), reps=5, warm=2)
    mp = timed(lambda: model.encode(x, rd_map=torch.full((32,), 0.1, device=dev)), reps=5, warm=2)
    host = timed(lambda: model.encode_to_rate(x, 0.9 * bpp0, iters=12), reps=3, warm=1)
    devs = timed(lambda: model.encode_to_rate(x, 0.9 * bpp0, iters=12, per_image=True), reps=3, warm=1)
print(f"encode {e[0] / 1e3:.2f} ms, rd_lambda=0.1 {r[0] / 1e3:.2f} ms, rd_map[n] {mp[0] / 1e3:.2f} ms; search host-read {host[0] / 1e3:.2f} ms, per-image {devs[0] / 1e3:.2f} ms (plain {bpp0:.4f} bpp)")
out["model"] = dict(encode_us=e, rd_lambda_us=r, rd_map_us=mp, search_host_us=host, search_per_image_us=devs)
print(json.dumps(out))
