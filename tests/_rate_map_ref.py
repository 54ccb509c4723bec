"""References of rate control per image and per region (`rd_map`), NumPy only: the assignment argmin_k (|x - c_k|^2 + lambda_v bits_k) with
one lambda per latent vector in float64, the kernel's sequence fl32(fma(lambda_v, bits32_k, dist32)) in float32, the level maps of
mcq_rate_map_levels_f32 in float32, and the per-image search rule of mcq_rate_search_step restated on a bpp curve or a recorded trace."""
import numpy as np

import _rate_ref as RR

MAP_LAMBDAS = (0.0, 0.25, 3.0)
MAPS = ((1, 1), (5, 7), (9, 33))      # one vector; odd, inside one 32-pixel block; 297 vectors: past a workgroup's 256 and across block seams


def map_lambdas(n: int, h: int, w: int, seed: int) -> np.ndarray:
    """float32 [n, h, w]: lambda per vector drawn from MAP_LAMBDAS (the CPU and the GPU test draw the same)."""
    rng = np.random.default_rng([31, seed, n, h, w])
    return np.asarray(MAP_LAMBDAS, dtype=np.float32)[rng.integers(0, len(MAP_LAMBDAS), size=(n, h, w))]


def bits_f32(cdf: np.ndarray) -> np.ndarray:
    """float32 [m, k]: fl32(16 - log2((double) width)), +inf at width 0."""
    return RR.penalty_table(cdf).astype(np.float32)


def lam_flat(lam: np.ndarray, m: int, h: int, w: int) -> np.ndarray:
    """lambda [n] or [n, h, w] -> float64 [m, n h w] (shared by the groups), the layout of `_rate_ref.flat_of`."""
    lam = np.asarray(lam, dtype=np.float64)
    n = lam.shape[0]
    full = np.broadcast_to(lam.reshape(n, 1, 1) if lam.ndim == 1 else lam, (n, h, w)).reshape(1, n * h * w)
    return np.repeat(full, m, 0)


def costs(x, codebook, bits, lam) -> np.ndarray:
    """float64 [m, n h w, k]: |x_v - c_k|^2 + lambda_v bits_k (0 * inf counts as inf: an empty slot never wins)."""
    n, _, h, w = x.shape
    m = codebook.shape[0]
    v = RR._vectors(np.asarray(x, dtype=np.float64), m)
    c = np.asarray(codebook, dtype=np.float64)
    dist = np.zeros((m, v.shape[1], c.shape[1]))
    for j in range(c.shape[2]):                                      # (channel by channel: no [m, V, k, d] temporary)
        dist += (v[:, :, None, j] - c[:, None, :, j]) ** 2
    lv = lam_flat(lam, m, h, w)[:, :, None]
    b = np.asarray(bits, dtype=np.float64)[:, None, :]
    with np.errstate(invalid="ignore"):
        return dist + np.where(np.isinf(b), np.inf, lv * np.where(np.isinf(b), 0.0, b))


def argmin_map(x, codebook, bits, lam) -> np.ndarray:
    n, _, h, w = x.shape
    return RR.codes_of(np.argmin(costs(x, codebook, bits, lam), -1), n, h, w)


def audit(x, codebook, bits, lam, got):
    """`_rate_ref.audit` with one lambda per vector: (positions that differ from the float64 argmin, those the bound
    (d + 4) 2^-23 (|x|^2 + |c|^2 + 2 |x.c| + lambda_v bits) does not excuse)."""
    n, _, h, w = x.shape
    m, k, d = codebook.shape
    cost = costs(x, codebook, bits, lam)
    want = np.argmin(cost, -1)
    g = RR.flat_of(np.asarray(got))
    bad = g != want
    if not bad.any():
        return 0, 0
    inside = (g >= 0) & (g < k)
    gc = np.clip(g, 0, k - 1)
    lv = lam_flat(lam, m, h, w)
    fb = np.where(np.isinf(bits), 0.0, bits)

    def bound(codes):
        return RR.excuse_bound(x, codebook, fb, 0.0, codes) + (d + 4) * 2.0 ** -23 * lv * np.take_along_axis(fb, codes, 1)
    gap = np.abs(np.take_along_axis(cost, gc[..., None], -1)[..., 0] - np.take_along_axis(cost, want[..., None], -1)[..., 0])
    ok = inside & np.isfinite(gap) & (gap <= np.maximum(bound(gc), bound(want)))
    return int(bad.sum()), int((bad & ~ok).sum())


def emulate_assign_f32(x, codebook, cdf, lam) -> np.ndarray:
    """The kernel's sequence: dist32 = fl32(fma(-2, inter32, fl32(x2 + c2))) as `_rate_ref.emulate_assign_f32` forms it, then
    cost = fl32(fma(lambda_v, bits32_k, dist32)) (the product of two float32 is exact in float64); NaN (0 * inf) never wins; first
    index on ties.  int64 [n, m, h, w]."""
    n, _, h, w = x.shape
    m, k, d = codebook.shape
    v = RR._vectors(np.asarray(x, dtype=np.float32), m)
    cb = np.asarray(codebook, dtype=np.float32)
    x2 = np.zeros(v.shape[:2], dtype=np.float32)
    for j in range(d):
        x2 = (x2 + (v[:, :, j] * v[:, :, j]).astype(np.float32)).astype(np.float32)
    inter = np.zeros((m, v.shape[1], k), dtype=np.float32)
    for j in range(0, d, 2):
        step = (v[:, :, None, j] * cb[:, None, :, j]).astype(np.float32)
        if j + 1 < d:
            step = (step + (v[:, :, None, j + 1] * cb[:, None, :, j + 1]).astype(np.float32)).astype(np.float32)
        inter = (inter + step).astype(np.float32)
    s2 = (x2[:, :, None] + RR.c2_f32(cb)[:, None, :]).astype(np.float32)
    dist = (s2.astype(np.float64) - 2.0 * inter.astype(np.float64)).astype(np.float32)
    lv = lam_flat(np.asarray(lam, dtype=np.float32), m, h, w).astype(np.float32).astype(np.float64)[:, :, None]
    with np.errstate(invalid="ignore"):
        cost = (lv * bits_f32(cdf).astype(np.float64)[:, None, :] + dist.astype(np.float64)).astype(np.float32)
    cost = np.where(np.isnan(cost), np.float32(np.inf), cost)
    return RR.codes_of(np.argmin(cost, -1), n, h, w)


def level_maps(rd_map: np.ndarray, scales):
    """mcq_rate_map_levels_f32 in float32: ([level buffers], error int32 [n]).  [n]: scale_l * map.  [n, h0, w0]: level l, cell (y, x) =
    the level-(l - 1) cells (2y .. 2y + 1, 2x .. 2x + 1) that exist, summed in row-major order and divided by their count, on the
    unscaled map; then times scale_l.  Negative, NaN and infinite values count as 0 and set the image's error word."""
    a = np.asarray(rd_map, dtype=np.float32)
    n = a.shape[0]
    with np.errstate(invalid="ignore"):
        bad = ~(a >= 0) | np.isinf(a)
    err = bad.reshape(n, -1).any(-1).astype(np.int32)
    cur = np.where(bad, np.float32(0), a).astype(np.float32)
    plain = [cur]
    if a.ndim == 3:
        for _ in range(1, len(scales)):
            hp, wp = cur.shape[1:]
            h, w = (hp + 1) // 2, (wp + 1) // 2
            nxt = np.zeros((n, h, w), dtype=np.float32)
            for y in range(h):
                for x in range(w):
                    s = np.zeros(n, dtype=np.float32)
                    cnt = 0
                    for yy in (2 * y, 2 * y + 1):
                        for xx in (2 * x, 2 * x + 1):
                            if yy < hp and xx < wp:
                                s = (s + cur[:, yy, xx]).astype(np.float32)
                                cnt += 1
                    nxt[:, y, x] = (s / np.float32(cnt)).astype(np.float32)
            plain.append(nxt)
            cur = nxt
    else:
        plain = plain * len(scales)
    return [(np.float32(s) * p).astype(np.float32) for s, p in zip(scales, plain)], err


def next_lambda(lo: float, hi: float) -> float:
    """The bracket's next point as the float32 the kernel takes: a sixteenth of the upper end while the lower is 0, else the geometric mean."""
    return float(np.float32(hi / 16.0 if lo == 0.0 else np.sqrt(np.float64(lo) * np.float64(hi))))


def search(bpp_of, target: float, lambda_max: float, iters: int):
    """The per-image rule on a bpp curve `bpp_of(lambda)`: (answer, [(lambda tried, bpp)] for all iters + 2 lockstep trials -- a finished
    image rides along at its answer)."""
    lambda_max = float(np.float32(lambda_max))
    trials = iters + 2
    trace, lam, lo, hi, done = [], 0.0, 0.0, lambda_max, False
    for t in range(trials):
        bpp = bpp_of(lam)
        trace.append((lam, bpp))
        if done:
            continue
        met = bpp <= target
        if t == 0:
            if met:
                done, hi = True, 0.0
            lam = hi
            continue
        if t == 1:
            if not met:
                done, lam = True, hi
                continue
        elif met:
            hi = lam
        else:
            lo = lam
        mid = next_lambda(lo, hi) if t + 1 < trials else hi
        if t + 1 < trials and lo < mid < hi:
            lam = mid
        else:
            done, lam = True, hi
    return lam, trace


def replay(bpps, target: float, lambda_max: float):
    """The lambdas the rule tries when trial t answers `bpps[t]`: (lambdas [trials], answer)."""
    it = iter(list(bpps))
    answer, trace = search(lambda lam: next(it), target, lambda_max, len(bpps) - 2)
    return [t[0] for t in trace], answer
