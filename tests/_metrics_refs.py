"""References for the stages of the validation metric (mcquic_amd/csrc/metrics.hip), for tests/test_gpu_metrics_leaf.py (which holds the
kernels to them) and tests/test_metrics_refs.py (which holds them to oracle/metrics_ref.py and to torch on the CPU).  Nothing here
imports mcquic_amd or the oracle: numpy float64 from the definitions.

  maps64      the SSIM and contrast-structure maps of one level: a separable 11-tap 'valid' blur of x, y, x^2, y^2, xy with the float32
              window widened to float64, data range 255.
  tile_sums   float64 sums of a map over the kernel's 16 x 118 tile grid; of maps64 the truth S64, of the oracle's float32 maps the
              float32 restatement S32.
  halve64     2 x 2 mean with a zero row / column in front of an odd side, divisor 4.
  combine64   prod over levels of relu(v)^w (the CS mean on levels 0..3, the SSIM mean on the last), mean over channels.

Planes are [P, H, W]."""
import numpy as np

TH, TW, HALO, LEVELS = 16, 118, 10, 5
# mcquic/validate/metrics.py:22-37 for size 11, sigma 1.5 in float32 (tests/test_metrics_refs.py: the oracle's gauss_window() and the
# library's mcq_ms_ssim_window), widened
WIN64 = np.array([float.fromhex(h) for h in ("0x1.0d957p-10", "0x1.f1fe02p-8", "0x1.26eb18p-5", "0x1.bff0fep-4", "0x1.b43c3ep-3", "0x1.10656p-2",
                                              "0x1.b43c3ep-3", "0x1.bff0fep-4", "0x1.26eb18p-5", "0x1.f1fe02p-8", "0x1.0d957p-10")])
# metrics.py:19 as float32 (the oracle's torch.tensor(MS_WEIGHTS)), widened
LEVEL_W64 = np.array([0.0448, 0.2856, 0.3001, 0.2363, 0.1333], np.float32).astype(np.float64)
C1, C2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
# map sizes (H - 10, W - 10) of the level kernel's seam shapes: one ragged row / column, exact multiples of the tile, a second and a third tile
SEAM_HOS, SEAM_WOS = (1, 15, 16, 17, 33), (1, 117, 118, 119, 237)


def blur64(q):
    """'valid' blur along rows, then along columns: [P, H, W] -> [P, H - 10, W - 10]."""
    q = np.asarray(q, np.float64)
    ho, wo = q.shape[1] - HALO, q.shape[2] - HALO
    v = sum(WIN64[t] * q[:, t:t + ho] for t in range(11))
    return sum(WIN64[t] * v[:, :, t:t + wo] for t in range(11))


def maps64(x, y):
    """(ssim, cs) [P, H - 10, W - 10] float64 of x, y [P, H, W] (any real dtype), data range 255."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    mu1, mu2 = blur64(x), blur64(y)
    s1, s2, s12 = blur64(x * x) - mu1 * mu1, blur64(y * y) - mu2 * mu2, blur64(x * y) - mu1 * mu2
    cs = (2.0 * s12 + C2) / (s1 + s2 + C2)
    return (2.0 * mu1 * mu2 + C1) / (mu1 * mu1 + mu2 * mu2 + C1) * cs, cs


def tile_grid(ho, wo):
    """(tiles_y, tiles_x) of a ho x wo map."""
    return (ho + TH - 1) // TH, (wo + TW - 1) // TW


def tile_counts(ho, wo):
    """[tiles_y, tiles_x] float64: the positions of each tile that lie inside the ho x wo map."""
    ty, tx = tile_grid(ho, wo)
    rows = np.minimum(TH, ho - TH * np.arange(ty))
    cols = np.minimum(TW, wo - TW * np.arange(tx))
    return (rows[:, None] * cols[None, :]).astype(np.float64)


def tile_sums(m, valid=None):
    """[P, tiles_y, tiles_x] float64 sums of m [P, >= ho, >= wo] over the tile grid of the valid map; valid = (ho, wo), default all of m.
    Positions outside the valid map are not read."""
    ho, wo = (m.shape[1], m.shape[2]) if valid is None else valid
    ty, tx = tile_grid(ho, wo)
    m = np.asarray(m, np.float64)[:, :ho, :wo]
    out = np.zeros((m.shape[0], ty, tx))
    for i in range(ty):
        for j in range(tx):
            out[:, i, j] = m[:, i * TH:(i + 1) * TH, j * TW:(j + 1) * TW].reshape(m.shape[0], -1).sum(axis=1)
    return out


def halve64(x):
    """[P, H, W] -> [P, ceil(H / 2), ceil(W / 2)] float64: zero padding on the top / left of an odd side, divisor 4."""
    x = np.asarray(x, np.float64)
    p_, h, w = x.shape
    ph, pw = h & 1, w & 1
    p = np.zeros((p_, h + ph, w + pw))
    p[:, ph:, pw:] = x
    return (p[:, 0::2, 0::2] + p[:, 0::2, 1::2] + p[:, 1::2, 0::2] + p[:, 1::2, 1::2]) / 4.0


def pyramid64(x):
    """[x_0 .. x_4] float64."""
    out = [np.asarray(x, np.float64)]
    for _ in range(LEVELS - 1):
        out.append(halve64(out[-1]))
    return out


def combine64(levels):
    """levels [5, N, C, 2] ({ssim, cs} means) -> [N] float64."""
    levels = np.asarray(levels, np.float64)
    v = np.concatenate([levels[:4, :, :, 1], levels[4:, :, :, 0]], axis=0)        # cs on levels 0..3, ssim on the last
    return np.prod(np.maximum(v, 0.0) ** LEVEL_W64[:, None, None], axis=0).mean(axis=1)
