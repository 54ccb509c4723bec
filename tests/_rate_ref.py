"""References of the rate-constrained assignment argmin_k (|x - c_k|^2 + lambda * bits_k), NumPy only.

`penalty_table` / `penalised_argmin` are float64 (first index on ties).  `norms_f32` restates the rounding sequence the pack entry
documents for its norm section, `emulate_assign_f32` the kernel's (x2 + c2') - 2 inter in float32, so that the CPU tests can say how
often float32 may pick another code than float64 on the seeds the GPU tests use.  `make_case` draws those seeds' inputs."""
import numpy as np

PACK_KS = (5, 128, 129, 512)          # one codeword tile; a full tile (the spare norm tile right behind it); the seam with a one-row tail; four tiles
PACK_DS = (1, 3, 64)                  # one channel (half a k-step); odd; the unrolled d = 64 instance
PACK_MS = (1, 2)
LAMBDAS = (0.25, 3.0)
MAPS = ((1, 1), (5, 7))
EXCUSED_CAP = 0.01                    # share of positions whose code may differ from float64's inside the rounding bound


def table_from_pmf(pmf: np.ndarray) -> np.ndarray:
    """A valid 16-bit table uint32 [m, k + 1] (cdf[0] = 0, cdf[k] = 65536, every width >= 1) from probabilities [m, k]: width_i =
    1 + floor(p_i (65536 - k)), the remainder to the widest slot."""
    pmf = np.asarray(pmf, dtype=np.float64)
    m, k = pmf.shape
    widths = 1 + np.floor(pmf / pmf.sum(-1, keepdims=True) * (65536 - k)).astype(np.int64)
    for g in range(m):
        widths[g, np.argmax(widths[g])] += 65536 - widths[g].sum()
    assert (widths >= 1).all() and (widths.sum(-1) == 65536).all()
    cdf = np.zeros((m, k + 1), dtype=np.int64)
    cdf[:, 1:] = np.cumsum(widths, -1)
    return cdf.astype(np.uint32)


def penalty_table(cdf: np.ndarray) -> np.ndarray:
    """bits [m, k] float64 = 16 - log2(cdf[i + 1] - cdf[i]); +inf for a slot of width 0."""
    width = np.diff(np.asarray(cdf, dtype=np.int64), axis=-1).astype(np.float64)
    with np.errstate(divide="ignore"):
        return np.where(width > 0, 16.0 - np.log2(np.where(width > 0, width, 1.0)), np.inf)


def _vectors(x: np.ndarray, m: int) -> np.ndarray:
    """[n, m d, h, w] -> [m, n h w, d] (channel = g d + j)."""
    n, c, h, w = x.shape
    d = c // m
    return x.reshape(n, m, d, h * w).transpose(1, 0, 3, 2).reshape(m, n * h * w, d)


def costs(x: np.ndarray, codebook: np.ndarray, bits: np.ndarray, lam: float) -> np.ndarray:
    """float64 [m, n h w, k]: |x_v - c_k|^2 + lam * bits_k."""
    v = _vectors(np.asarray(x, dtype=np.float64), codebook.shape[0])
    c = np.asarray(codebook, dtype=np.float64)
    dist = ((v[:, :, None, :] - c[:, None, :, :]) ** 2).sum(-1)
    return dist + (float(lam) * np.asarray(bits, dtype=np.float64)[:, None, :] if lam != 0 else 0.0)


def codes_of(flat: np.ndarray, n: int, h: int, w: int) -> np.ndarray:
    """[m, n h w] -> int64 [n, m, h, w]."""
    m = flat.shape[0]
    return flat.reshape(m, n, h, w).transpose(1, 0, 2, 3).astype(np.int64)


def flat_of(codes: np.ndarray) -> np.ndarray:
    """int64 [n, m, h, w] -> [m, n h w]."""
    n, m, h, w = codes.shape
    return codes.transpose(1, 0, 2, 3).reshape(m, n * h * w)


def penalised_argmin(x: np.ndarray, codebook: np.ndarray, bits: np.ndarray, lam: float) -> np.ndarray:
    """int64 [n, m, h, w], first index on ties (np.argmin's rule)."""
    n, _, h, w = x.shape
    return codes_of(np.argmin(costs(x, codebook, bits, lam), -1), n, h, w)


def excuse_bound(x: np.ndarray, codebook: np.ndarray, bits: np.ndarray, lam: float, codes_flat: np.ndarray) -> np.ndarray:
    """float64 [m, n h w]: (d + 4) 2^-23 (|x|^2 + |c|^2 + 2 |x.c| + lam bits) for the codeword c a position holds -- the bound of the
    kernel's rounding sequence (d products and sums of the inner product, the two norms' sums, the penalty's two roundings, the two
    additions of the epilogue)."""
    m, k, d = codebook.shape
    v = _vectors(np.asarray(x, dtype=np.float64), m)
    c = np.take_along_axis(np.asarray(codebook, dtype=np.float64), codes_flat[:, :, None], 1)        # [m, V, d]
    b = np.take_along_axis(np.asarray(bits, dtype=np.float64), codes_flat, 1)
    mag = (v ** 2).sum(-1) + (c ** 2).sum(-1) + 2 * np.abs((v * c).sum(-1)) + float(lam) * b
    return (d + 4) * 2.0 ** -23 * mag


def audit(x, codebook, bits, lam, got: np.ndarray):
    """(positions that differ from float64's argmin, those of them the bound does NOT excuse).  A differing position is excused only
    when the float64 costs of the two candidates differ by at most the bound (taken at the candidate where it is larger: the two
    computed costs each carry half of (d + 4) 2^-23 of their magnitude)."""
    cost = costs(x, codebook, bits, lam)
    want = np.argmin(cost, -1)
    g = flat_of(np.asarray(got))
    bad = g != want
    if not bad.any():
        return 0, 0
    inside = (g >= 0) & (g < codebook.shape[1])
    gc = np.clip(g, 0, codebook.shape[1] - 1)
    gap = np.abs(np.take_along_axis(cost, gc[..., None], -1)[..., 0] - np.take_along_axis(cost, want[..., None], -1)[..., 0])
    bound = np.maximum(excuse_bound(x, codebook, bits, lam, gc), excuse_bound(x, codebook, bits, lam, want))
    return int(bad.sum()), int((bad & ~(inside & (gap <= bound))).sum())


def c2_f32(codebook: np.ndarray) -> np.ndarray:
    """float32 [m, k]: s = s + c_j * c_j over j in order, every product and sum rounded to float32 (the norm kernels' loop)."""
    cb = np.asarray(codebook, dtype=np.float32)
    s = np.zeros(cb.shape[:2], dtype=np.float32)
    for j in range(cb.shape[2]):
        s = (s + (cb[:, :, j] * cb[:, :, j]).astype(np.float32)).astype(np.float32)
    return s


def norms_f32(codebook: np.ndarray, cdf: np.ndarray, lam: float) -> np.ndarray:
    """float32 [m, k]: fl32(c2 + fl32(lam * fl32(16 - log2((double) width)))), log2 and the subtraction in float64; +inf at width 0."""
    bits = penalty_table(cdf)
    finite = np.isfinite(bits)
    b32 = np.where(finite, bits, 0.0).astype(np.float32)
    pen = (np.float32(lam) * b32).astype(np.float32)
    out = (c2_f32(codebook) + pen).astype(np.float32)
    return np.where(finite, out, np.float32(np.inf)).astype(np.float32)


def norm_section_layout(m: int, k: int):
    """Where the norm section [m][ntile + 1][64][4] of a packed codebook holds what: (group, codeword, kind) per float, kind 0 = the
    norm of codeword `word` < k, 1 = a padded codeword (+inf), 2 = the upper half-wave (0)."""
    ntile = (k + 127) // 128
    i = np.arange(m * (ntile + 1) * 256)
    q, lane, rest = i & 3, (i >> 2) & 63, i >> 8
    tile, g = rest % (ntile + 1), rest // (ntile + 1)
    word = tile * 128 + 32 * q + (lane & 31)
    kind = np.where(lane >> 5 != 0, 2, np.where((tile < ntile) & (word < k), 0, 1))
    return g, word, kind


def emulate_assign_f32(x: np.ndarray, codebook: np.ndarray, norms: np.ndarray) -> np.ndarray:
    """The kernel's sequence in float32: x2 summed over the channels in order, the inner product accumulated two channels per step
    (one MFMA k-step; the pair's order inside the instruction is the emulation's guess), dist = fma(-2, inter, x2 + c2'); first
    index on ties.  int64 [n, m, h, w]."""
    n, _, h, w = x.shape
    m, k, d = codebook.shape
    v = _vectors(np.asarray(x, dtype=np.float32), m)
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
    s2 = (x2[:, :, None] + np.asarray(norms, dtype=np.float32)[:, None, :]).astype(np.float32)
    dist = (s2.astype(np.float64) - 2.0 * inter.astype(np.float64)).astype(np.float32)           # (2 inter is exact: one rounding, like the fma)
    return codes_of(np.argmin(dist, -1), n, h, w)


def make_case(m: int, k: int, d: int, h: int, w: int, n: int = 2, seed: int = 0):
    """Seeded inputs of one assignment case: x [n, m d, h, w] and codebook [m, k, d] standard Gaussians (float32), and a table from a
    Dirichlet(1) draw, so that the penalties are distinct."""
    rng = np.random.default_rng([20261021, seed, m, k, d, h, w])
    x = rng.standard_normal((n, m * d, h, w)).astype(np.float32)
    codebook = rng.standard_normal((m, k, d)).astype(np.float32)
    cdf = table_from_pmf(rng.dirichlet(np.ones(k), size=m))
    return x, codebook, cdf


def dominant_table(m: int, k: int, symbol: int) -> np.ndarray:
    """Every slot of width 1 but `symbol`, which holds the rest of the 65536."""
    widths = np.ones((m, k), dtype=np.int64)
    widths[:, symbol] = 65536 - (k - 1)
    cdf = np.zeros((m, k + 1), dtype=np.int64)
    cdf[:, 1:] = np.cumsum(widths, -1)
    return cdf.astype(np.uint32)
