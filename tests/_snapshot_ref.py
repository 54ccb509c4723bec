"""References for the log-payload kernels (csrc/step_snapshot.hip), independent of them; tests/test_snapshot_ref.py pins each against the
real thing (np.histogram, torch's ops on the CPU), so that the GPU tests lean on something that was itself checked.

`histogram`: numpy's algorithm restated step by step from numpy/lib/_histograms_impl.py (`_get_outer_edges`, `_get_bin_edges`, the
uniform-bin fast path of `histogram`) and numpy/_core/function_base.py (`linspace`), in float64: what np.histogram returns for the
values widened to float64.  (For a float32 ARRAY numpy >= 2 keeps first_edge, the edges and the index arithmetic in float32; the
kernels take the float64 form, whose edges are the exact ones of the widened -- identical -- values.)"""
import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-6                      # Consts.Eps


def linspace(first: float, last: float, bins: int) -> np.ndarray:
    """np.linspace(first, last, bins + 1) for float64 scalars: y = arange * step (arange / div * delta if the step is 0), += first,
    and the last element is `last` itself."""
    first, last = np.float64(first), np.float64(last)
    div = bins
    delta = last - first
    y = np.arange(0, bins + 1, dtype=np.float64)
    step = delta / div
    if step == 0:
        y = y / div
        y = y * delta
    else:
        y = y * step
    y = y + first
    y[-1] = last
    return y


def histogram(v, bins: int):
    """(counts int64 [bins], edges float64 [bins + 1], (finite, non-finite)): np.histogram(finite part of v as float64, bins)."""
    v = np.asarray(v).reshape(-1)
    ok = np.isfinite(v)
    a = v[ok].astype(np.float64)
    stats = (int(ok.sum()), int((~ok).sum()))
    if a.size == 0:
        first, last = np.float64(0.0), np.float64(1.0)
    else:
        first, last = a.min(), a.max()
    if first == last:
        first = first - 0.5
        last = last + 0.5
    edges = linspace(first, last, bins)
    denom = last - first
    f = ((a - first) / denom) * bins
    idx = f.astype(np.intp)
    idx[idx == bins] -= 1
    idx[a < edges[idx]] -= 1
    up = (a >= edges[idx + 1]) & (idx != bins - 1)
    idx[up] += 1
    return np.bincount(idx, minlength=bins).astype(np.int64), edges, stats


def log_distance64(x) -> np.ndarray:
    """log10(clamp(-x, min = eps)) in float64 with eps = float32(1e-6) (the kernel's argument is a float); a NaN passes through."""
    nx = -np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.log10(np.where(np.isnan(nx), nx, np.maximum(nx, np.float64(np.float32(EPS)))))


def ulp_distance(got: np.ndarray, want64: np.ndarray) -> float:
    """Worst |got - want| in units of float32 spacing at the float64 reference value (both finite)."""
    got, want64 = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want64, dtype=np.float64).reshape(-1)
    spacing = np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
    return float(np.max(np.abs(got - want64) / spacing))


def detransform(x: torch.Tensor) -> torch.Tensor:
    """DeTransform.forward (mcquic/utils/vision.py:143-146) with min -1, max 1, from torch ops on the CPU."""
    x = (x - (-1.0)) / (1.0 - (-1.0))
    return (x * (255 + 1.0 - 1e-3)).clamp(0.0, 255.0).byte()


def code_image(codes: torch.Tensor, keep=None) -> torch.Tensor:
    """visualizeIntermediate (mcquic/validate/validator.py:30-38) written out op by op on the CPU, group 0 taken BEFORE the arithmetic
    (element-wise ops commute with the slice; the maximum is still the whole tensor's); 0 for an all-zero tensor (documented)."""
    codes = codes.cpu()
    n, m, h, w = codes.shape
    keep = n if keep is None else keep
    mx = codes.max()
    if int(mx) == 0:
        return torch.zeros((keep, 1, 4 * h, 4 * w), dtype=torch.uint8)
    t = codes[:keep, :1].float() / mx
    t = (t - 0.5) * 2
    img = detransform(t)
    out = torch.empty((keep, 1, 4 * h, 4 * w), dtype=torch.uint8)
    for dy in range(4):
        for dx in range(4):
            out[:, :, dy::4, dx::4] = img                      # nearest, scale 4: out[y, x] = in[y // 4, x // 4]
    return out


def normalized_freq(freqs):
    """Per level: (group 0 of f / sum f, entries with f / sum f > 1e-6 over all groups), the row sum exact (math.fsum) and rounded to
    float32 once, quotient and comparison in float32 as torch evaluates `freq > 1e-6` on a float32 tensor."""
    import math
    rows, used, entries = [], 0, 0
    for f in freqs:
        f = np.asarray(f, dtype=np.float32)
        s = np.array([np.float32(math.fsum(float(v) for v in row)) for row in f], dtype=np.float32)[:, None]
        p = (f / s).astype(np.float32)
        rows.append(p[0])
        used += int((p > np.float32(1e-6)).sum())
        entries += p.size
    return rows, np.float32(used) / np.float32(entries)


def histogram_cases(chunk: int):
    """name -> (float32 values, bins): the identity-transform cases.  `chunk`: the elements one workgroup takes per trip."""
    g = np.random.default_rng(20251020)
    normal = lambda n: g.standard_normal(n).astype(np.float32)
    cases = {"n=1": (np.array([0.75], np.float32), 64)}
    for n in (63, 64, 65, chunk - 1, chunk, chunk + 1, 100003):
        cases[f"n={n}"] = (normal(n), 64)
    cases["integers 0..64"] = (np.arange(65, dtype=np.float32), 64)
    cases["all equal"] = (np.full(1000, -3.25, np.float32), 64)
    cases["all equal, not a dyadic value"] = (np.full(777, 0.1, np.float32), 7)
    for bins in (1, 64, 4096):
        cases[f"bins={bins}"] = (normal(3 * chunk + 17), bins)
    cases["scaled 1e-30"] = ((normal(5000).astype(np.float64) * 1e-30).astype(np.float32), 64)
    cases["scaled 1e30"] = ((normal(5000).astype(np.float64) * 1e30).astype(np.float32), 64)
    cases["few distinct values on bin edges"] = (g.integers(0, 9, 3 * chunk).astype(np.float32) / 8.0, 8)
    return cases


def sprinkled(n: int = 20000):
    g = np.random.default_rng(7)
    x = g.standard_normal(n).astype(np.float32)
    x[g.choice(n, 37, replace=False)] = np.nan
    x[5], x[n - 1], x[n // 2] = np.inf, -np.inf, np.inf
    return x


def logit_cases():
    """Seeded logits [2, 2, 8] and [4, 4, 512]: magnitudes from 1e-12 to 1e4, mostly negative (distances), some positive so that the
    clamp acts, plus the clamp's own corner values."""
    g = np.random.default_rng(11)
    out = {}
    for shape in ((2, 2, 8), (4, 4, 512)):
        n = int(np.prod(shape))
        mag = 10.0 ** g.uniform(-12, 4, n)
        sign = np.where(g.uniform(size=n) < 0.15, 1.0, -1.0)
        x = (sign * mag).astype(np.float32)
        x[:4] = [-1e-6, -np.float32(1e-6), 0.0, -1.0]
        out[str(shape)] = x.reshape(shape)
    return out
