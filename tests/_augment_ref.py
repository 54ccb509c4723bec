"""The training input transform, stated independently in float64 (NumPy / torch-CPU) from its formulas -- not from the kernel:

    resample of the crop box (the separable triangle filter of F.interpolate(mode="bilinear", antialias=True,
    align_corners=False) on the crop: support max(in / out, 1) per axis, weights normalised per output pixel, taps clipped to the
    box) -> gamma (the four modes of mcquic/utils/vision.py:108-129) -> gains on channels 0 and 2 -> clamp to [0, 1] -> flips
    -> (v - 0.5) / 0.5.

tests/test_augment_ref.py pins `resample` to ATen's CPU kernel; tests/test_gpu_augment.py holds the HIP pass against `pipeline`."""
import numpy as np

# the table's columns (include/mcquic_hip.h: MCQ_AUG_*), written out here so that the reference does not import the package
TOP, LEFT, BOX_H, BOX_W, GAMMA_MODE, GAMMA, GAIN0, GAIN2, HFLIP, VFLIP, GAIN_ROW, FALLBACK, OUTPUT = range(13)
COLUMNS = 16
SRGB_TO_LINEAR, LINEAR_TO_SRGB, POWER, IDENTITY = range(4)
OUT_NORMALIZED, OUT_CLAMPED, OUT_RAW = range(3)


def taps(o: int, n_in: int, n_out: int):
    """(first source index, normalised weights) of output index `o` on an axis that maps n_in samples to n_out."""
    scale = n_in / n_out
    support = scale if scale >= 1.0 else 1.0
    invscale = 1.0 / scale if scale >= 1.0 else 1.0
    center = scale * (o + 0.5)
    lo = max(int(center - support + 0.5), 0)
    hi = min(int(center + support + 0.5), n_in)
    w = []
    for j in range(lo, hi):                                   # the explicit tap loop
        t = abs((j - center + 0.5) * invscale)
        w.append(1.0 - t if t < 1.0 else 0.0)
    total = sum(w)
    return lo, [v / total for v in w]


def resample(crop: np.ndarray, size) -> np.ndarray:
    """[C, h, w] float64 -> [C, H, W]: columns first, then rows (the order of ATen's separable pass)."""
    crop = np.asarray(crop, dtype=np.float64)
    c, h, w = crop.shape
    H, W = size
    tmp = np.zeros((c, h, W))
    for x in range(W):
        lo, wt = taps(x, w, W)
        for j, v in enumerate(wt):
            tmp[:, :, x] += v * crop[:, :, lo + j]
    out = np.zeros((c, H, W))
    for y in range(H):
        lo, wt = taps(y, h, H)
        for j, v in enumerate(wt):
            out[:, y, :] += v * tmp[:, lo + j, :]
    return out


def gamma(x: np.ndarray, mode: int, g: float) -> np.ndarray:
    if mode == SRGB_TO_LINEAR:
        return np.where(x < 0.0031308, 12.92 * x, 1.055 * np.abs(x) ** (1 / 2.4) - 0.055)
    if mode == LINEAR_TO_SRGB:
        return np.where(x < 0.04045, x / 12.92, (np.abs(x + 0.055) / 1.055) ** 2.4)
    if mode == POWER:
        return np.clip(np.clip(x, 0.0, None) ** g, 0.0, 1.0)
    return x


def pipeline(src, size, params) -> np.ndarray:
    """src [N, 3, Hs, Ws] uint8 or float (NumPy), params [N, 16] -> [N, 3, H, W] float64."""
    src = np.asarray(src)
    x = src.astype(np.float64) / 255.0 if src.dtype == np.uint8 else src.astype(np.float64)
    params = np.asarray(params, dtype=np.float64)
    out = []
    for n in range(x.shape[0]):
        p = params[n]
        top, left, h, w = (int(p[k]) for k in (TOP, LEFT, BOX_H, BOX_W))
        v = resample(x[n, :, top: top + h, left: left + w], size)
        v = gamma(v, int(p[GAMMA_MODE]), float(p[GAMMA]))
        v = v * np.array([p[GAIN0], 1.0, p[GAIN2]])[:, None, None]
        mode = int(p[OUTPUT])
        if mode != OUT_RAW:
            v = np.clip(v, 0.0, 1.0)
        if p[HFLIP] != 0:
            v = v[:, :, ::-1]
        if p[VFLIP] != 0:
            v = v[:, ::-1, :]
        if mode == OUT_NORMALIZED:
            v = (v - 0.5) / 0.5
        out.append(v)
    return np.stack(out)


def identity_params(n: int, src_size) -> np.ndarray:
    p = np.zeros((n, COLUMNS), dtype=np.float32)
    p[:, BOX_H], p[:, BOX_W] = src_size
    p[:, GAMMA_MODE] = IDENTITY
    p[:, GAMMA] = p[:, GAIN0] = p[:, GAIN2] = 1.0
    p[:, GAIN_ROW] = -1.0
    return p
