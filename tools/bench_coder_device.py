"""Timings of docs/experiments.md section 29 (one MI355X): the entropy coder on the host (`EntropyCoder.compress` / `decompress`,
csrc/rans.cpp on host threads) against the device coder (`compressDevice().tobytes()` / `decompressDevice`, csrc/rans_dev.hip), in one
process and under the same tables, at the qp=2 shape m = 2, k = [8192, 2048, 512] with codes drawn from a skewed table:
    10 x 768x512 (the speed protocol's batch), 32 x 768x512, 1 x 3584x3840 (13.8 MP: one stream of 107 520 symbols on level 0).
Every arm starts from codes (or bytes) where its caller has them -- codes on the device, bytes on the host -- and ends with bytes on the
host (or codes on the device), so copies and synchronisations are inside the window: wall time around a call that ends in a device
synchronise, after a warm-up, median of `--reps`; for the device arms also the device time alone from events around 10 calls.  The
bytes of the two sides are compared before anything is timed.  Section 33's columns follow in the same process and protocol: the
lane-interleaved layout on the host (`compress(codes, lanes="auto")`), on the device at auto and on the device forced to 64 lanes
(csrc/rans_lanes.hip), with each arm's bytes over the plain streams' bytes.  Prints one JSON document (and writes it to --out).

    python tools/bench_coder_device.py [--reps 15] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from mcquic_amd.modules import entropyCoder as E  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=15)
ap.add_argument("--out", default=None)
args = ap.parse_args()

dev = torch.device("cuda:0")
M, KS = 2, [8192, 2048, 512]
SHAPES = {"10x768x512": (10, 768, 512), "32x768x512": (32, 768, 512), "1x3584x3840": (1, 3584, 3840)}


def wall(fn, reps):
    fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize(); t = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t) * 1e3)
    ts.sort()
    return {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1], "reps": reps}


def events(fn, calls=10):
    fn(); torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


coder = E.EntropyCoder(M, KS).to(dev)
g = torch.Generator().manual_seed(0)
with torch.no_grad():
    for f in coder._freqEMA:
        f.copy_((torch.rand(f.shape, generator=g) ** 6 + 1e-9).to(dev))
freq = coder.NormalizedFreq
out = {"m": M, "k": KS}
for name, (n, height, width) in SHAPES.items():
    codes = []
    for lv in range(len(KS)):
        h, w = height >> (4 + lv), width >> (4 + lv)
        per_group = [torch.multinomial(freq[lv][j].cpu(), n * h * w, replacement=True, generator=g).reshape(n, h, w) for j in range(M)]
        codes.append(torch.stack(per_group, 1).contiguous().to(dev))
    binaries, sizes = coder.compress(codes)
    streams = coder.compressDevice(codes)
    assert streams.tobytes() == binaries, "the device coder's bytes differ from the host coder's"
    assert all(torch.equal(a, b) for a, b in zip(coder.decompressDevice(binaries, sizes), codes))
    row = {"symbols_per_image": [int(c[0].numel()) for c in codes], "streams": n * len(KS),
           "bytes": sum(len(b) for binary in binaries for b in binary),
           "compress_host": wall(lambda: coder.compress(codes), args.reps),
           "compress_device_tobytes": wall(lambda: coder.compressDevice(codes).tobytes(), args.reps),
           "compress_device_kernels_event_ms": events(lambda: coder.compressDevice(codes, out=streams)),
           "decompress_host": wall(lambda: coder.decompress(binaries, sizes), args.reps),
           "decompress_device_from_bytes": wall(lambda: coder.decompressDevice(binaries, sizes), args.reps),
           "decompress_device_kernel_event_ms": events(lambda: coder.decompressDevice(streams, sizes, check=False))}
    # the lanes layout (section 30): the host lanes coder, the device at auto and the device forced to 64, same protocol; sizes beside
    lanes_host, _ = coder.compress(codes, lanes="auto")
    for tag, lanes in (("auto", "auto"), ("64", 64)):
        dev_streams = coder.compressDevice(codes, lanes=lanes)
        lanes_bytes = dev_streams.tobytes()
        assert lanes_bytes == coder.compress(codes, lanes=lanes)[0], "the device lanes coder's bytes differ from the host lanes coder's"
        assert all(torch.equal(a, b) for a, b in zip(coder.decompressDevice(lanes_bytes, sizes, lanes=True), codes))
        row[f"lanes_{tag}"] = {
            "widths": [int(b[3]) for b in lanes_bytes[0]], "bytes": sum(len(b) for binary in lanes_bytes for b in binary),
            "size_over_plain": sum(len(b) for binary in lanes_bytes for b in binary) / row["bytes"],
            "compress_device_tobytes": wall(lambda: coder.compressDevice(codes, lanes=lanes).tobytes(), args.reps),
            "compress_device_kernels_event_ms": events(lambda: coder.compressDevice(codes, out=dev_streams, lanes=lanes)),
            "decompress_device_from_bytes": wall(lambda: coder.decompressDevice(lanes_bytes, sizes, lanes=True), args.reps),
            "decompress_device_kernel_event_ms": events(lambda: coder.decompressDevice(dev_streams, sizes, check=False, lanes=True))}
    row["lanes_host_auto"] = {"compress_host": wall(lambda: coder.compress(codes, lanes="auto"), args.reps),
                              "decompress_host": wall(lambda: coder.decompress(lanes_host, sizes, lanes=True), args.reps)}
    out[name] = row
    print(name, json.dumps(row), flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
print(json.dumps(out))
