"""Timings of docs/experiments.md section 28 (one MI355X): the entropy coder's table build on the host (`EntropyCoder.updateFreqAndCDF`) against
`deviceCDFs()` / `deviceCDFs(normalize=True)` at the qp=2 shape m = 2, k = [8192, 2048, 512] for a uniform table, one with half the symbols
dead and a skewed one; then `validate(bits="coded")` against `bits="estimated"` on ten 768x512 images.  Wall time around a call with the device
idle before and after, medians; prints one JSON document (and writes it to --out).

    python tools/bench_cdf.py [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mcquic_amd import Compressor, validate as V  # noqa: E402
from mcquic_amd.modules import entropyCoder as E  # noqa: E402

dev = torch.device("cuda:0")
out = {}

def wall(fn, reps):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(); t = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t) * 1e3)
    ts.sort()
    return {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1], "reps": reps}

for name in ("uniform", "half_dead", "trained_like"):
    coder = E.EntropyCoder(2, [8192, 2048, 512]).to(dev)
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        for f in coder._freqEMA:
            if name == "half_dead":
                r = torch.rand(f.shape, generator=g) + 0.1
                r[:, torch.rand(f.shape[1], generator=g) < 0.5] = 0.0
                f.copy_(r.to(dev))
            elif name == "trained_like":
                f.copy_((torch.rand(f.shape, generator=g) ** 6 + 1e-9).to(dev))
    def host():
        coder.updateFreqAndCDF()
    def device(norm):
        def go():
            coder.resetFreqAndCDF(); coder.deviceCDFs(norm)
        return go
    out[name] = {"updateFreqAndCDF_host": wall(host, 7), "deviceCDFs": wall(device(False), 50), "deviceCDFs_normalize": wall(device(True), 50)}
    # device time alone of the one launch
    coder.deviceCDFs(True)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(20):
        coder.resetFreqAndCDF(); coder.deviceCDFs(True)
    b.record(); torch.cuda.synchronize()
    out[name]["deviceCDFs_normalize_event_ms_per_call"] = a.elapsed_time(b) / 20
    print(name, json.dumps(out[name]), flush=True)

torch.manual_seed(0)
model = Compressor(128, 2, [8192, 2048, 512]).eval().to(dev)
x = (torch.rand(10, 3, 768, 512, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(dev)
for mode in ("coded", "estimated"):
    out["validate_" + mode] = wall(lambda: V.validate(model, x, gather=False, bits=mode), 10)
    print(mode, json.dumps(out["validate_" + mode]), flush=True)
rows_c = V.validate(model, x, gather=False); rows_e = V.validate(model, x, gather=False, bits="estimated")
out["bpp_coded_mean"] = float(rows_c[:, 2].mean()); out["bpp_estimated_mean"] = float(rows_e[:, 2].mean())
out["psnr_equal"] = bool(torch.equal(rows_c[:, :2], rows_e[:, :2]))
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
args = ap.parse_args()
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out))
