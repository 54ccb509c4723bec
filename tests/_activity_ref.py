"""Float64 NumPy restatement of the adaptive-quantisation map (csrc/rate_activity.hip): `AlignedPadding`'s reflect padding through
np.pad, the luma with the three constants at their float32 values, the centred variance of every 16 x 16 cell, log2, the masked mean,
clamp, exp2 and the roi / lam products -- and the images and error bounds the CPU and GPU tests share."""
import numpy as np

FLOOR = 2.0 ** -14
KR, KG, KB = (float(np.float32(v)) for v in (0.299, 0.587, 0.114))
U = 2.0 ** -24                       # float32's unit roundoff
# The kernel's sums are balanced trees of depth 8 (4 values in a lane as (a + b) + (c + d), then six butterfly steps), so a sum of 256
# terms carries 8 roundings, not 255.  T = 8 + 1 (the square) + 1 (the + 2^-14) roundings stand between the centred lumas and log2's
# argument; T + 4 = 8 (the mean's tree) + 3 (the luma: one product, two fma) + 1 (Y - mu) + 2 spare bound a centred luma's absolute error
# while |Y| <= 1.
T = 10
GEOMS = ((128, 128), (130, 200), (129, 257))       # no padding; both axes, even split; 127 + 127 with the odd splits 63 / 64
KINDS = ("gauss", "uniform", "contrast")
EXCUSED_CAP = 0.01


def pad_split(h: int, w: int, base: int = 128):
    """(top, bottom, left, right) of `AlignedPadding`: the smaller half first."""
    hpad, wpad = (base - h % base) % base, (base - w % base) % base
    return hpad // 2, hpad - hpad // 2, wpad // 2, wpad - wpad // 2


def padded(x: np.ndarray, base: int = 128) -> np.ndarray:
    top, bottom, left, right = pad_split(x.shape[-2], x.shape[-1], base)
    if max(top, bottom) > x.shape[-2] - 1 or max(left, right) > x.shape[-1] - 1:
        raise RuntimeError("Padding size should be less than the corresponding input dimension")
    return np.pad(x, ((0, 0), (0, 0), (top, bottom), (left, right)), mode="reflect")


def luma(x: np.ndarray) -> np.ndarray:
    x = x.astype(np.float64)
    return KB * x[:, 2] + (KG * x[:, 1] + KR * x[:, 0])


def cells(x: np.ndarray, base: int = 128):
    """(a, v, mask) float64 / float64 / bool [n, h0, w0] of a float32 image batch [n, 3, H, W]."""
    y = luma(padded(x, base))
    n, hp, wp = y.shape
    c = y.reshape(n, hp // 16, 16, wp // 16, 16).transpose(0, 1, 3, 2, 4).reshape(n, hp // 16, wp // 16, 256)
    mask = ~np.isfinite(c).all(-1)
    with np.errstate(invalid="ignore", over="ignore"):
        mu = c.sum(-1) / 256.0
        v = ((c - mu[..., None]) ** 2).sum(-1) / 256.0
        a = np.log2(v + FLOOR)
    a[mask] = 0.0
    v[mask] = 0.0
    return a, v, mask


def exponents(a: np.ndarray, mask: np.ndarray, strength: float) -> np.ndarray:
    """strength * (a - abar) before the clamp, abar the image's mean over its unmasked cells (0 where there is none)."""
    e = np.zeros_like(a)
    for i in range(a.shape[0]):
        keep = ~mask[i]
        abar = a[i][keep].mean() if keep.any() else 0.0
        e[i] = strength * (a[i] - abar)
    return e


def weights(a: np.ndarray, mask: np.ndarray, strength: float, clip: float, roi=None, lam=None):
    """(w, out) float64 [n, h0, w0]: w = exp2(clamp(e)), 1 where masked; out = w * roi * lam, a bad roi value NaN."""
    w = np.exp2(np.clip(exponents(a, mask, strength), -clip, clip))
    w[mask] = 1.0
    out = w.copy()
    if roi is not None:
        r = np.asarray(roi, dtype=np.float64)
        r = np.where((r >= 0) & np.isfinite(r), r, np.nan)
        out = out * (r[:, None, None] if r.ndim == 1 else r)
    if lam is not None:
        out = out * np.asarray(lam, dtype=np.float64)[:, None, None]
    return w, out


def tol_a(v: np.ndarray, a: np.ndarray) -> np.ndarray:
    """|a - a_ref| allowed per cell: delta = (T + 4) u on every centred luma moves v by at most 2 delta sqrt(v) + delta^2, the T
    roundings above it by T u v; log2 turns that into / ((v + 2^-14) ln 2), and its own rounding adds 2 u |a|."""
    delta = (T + 4) * U
    return (2 * delta * np.sqrt(v) + delta * delta + T * U * v) / ((v + FLOOR) * np.log(2.0)) + 2 * U * np.abs(a)


def tol_w(ta: np.ndarray, strength: float) -> np.ndarray:
    """|w / w_ref - 1| allowed per cell of one image: the cell's own a and the mean (at most the worst cell's) move the exponent."""
    return np.log(2.0) * strength * (ta + ta.max(axis=(-2, -1), keepdims=True)) + 4 * U


def near_clip(a: np.ndarray, mask: np.ndarray, ta: np.ndarray, strength: float, clip: float) -> np.ndarray:
    """Cells whose exponent lies within its own error of a clip boundary: the clamp may fall either way there."""
    e = exponents(a, mask, strength)
    return (np.abs(np.abs(e) - clip) <= strength * (ta + ta.max(axis=(-2, -1), keepdims=True))) & ~mask


def make_image(kind: str, n: int, h: int, w: int, seed: int) -> np.ndarray:
    """float32 [n, 3, h, w] in [-1, 1].  "contrast": noise whose amplitude falls by 2^-9 from the left edge to the right and differs
    per image, so the activities span the floor's knee and the weights both clip boundaries."""
    rng = np.random.default_rng([seed, n, h, w, KINDS.index(kind)])
    if kind == "gauss":
        x = np.clip(rng.normal(0.0, 0.3, size=(n, 3, h, w)), -1, 1)
    elif kind == "uniform":
        x = rng.uniform(-1, 1, size=(n, 3, h, w))
    else:
        amp = np.exp2(-9.0 * np.arange(w) / max(w - 1, 1))[None, None, None, :] * np.exp2(-np.arange(n))[:, None, None, None]
        x = rng.uniform(-0.5, 0.5, size=(n, 3, 1, 1)) + amp * rng.uniform(-0.5, 0.5, size=(n, 3, h, w))
    return x.astype(np.float32)
