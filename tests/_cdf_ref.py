"""Pure-numpy restatements for the device CDF tables and the code-length sum (csrc/vq_cdf.hip):

  quantized_cdf(pmf)        the table rule of `mcq_pmf_to_quantized_cdf` (csrc/rans.cpp) at precision 16, step for step, the steal loop
                            as the sequential loop it is defined as; returns (cdf uint32 [k + 1], status)
  quantized_cdf_closed(pmf) the same table with the steal loop in the closed form csrc/vq_cdf.hip evaluates (a transcription of the
                            kernel's steps; tests/test_cdf_ref.py holds it to quantized_cdf without a GPU)
  normalise(raw)            the `normalize` rule: the row sum in double, rounded once to float32, then a float32 division
  code_bits(codes, tables)  sum over groups and positions of 16 - log2(cdf[c + 1] - cdf[c]) in float64, per image and level
  cases()                   the rows the CPU pin (tests/test_cdf_ref.py) and the device test (tests/test_gpu_quantized_cdf.py) share

tests/test_cdf_ref.py pins quantized_cdf to the library's host function on cases(); the device kernels are then compared with this file."""
import numpy as np

OK, BAD_ELEMENT, ZERO_TOTAL, NO_DONOR = 0, 1, 2, 3


def quantized_cdf(pmf):
    p = np.asarray(pmf, dtype=np.float32)
    k = p.shape[0]
    cdf = np.zeros(k + 1, dtype=np.uint32)
    if np.any(p < 0) or not np.all(np.isfinite(p)):
        return cdf, BAD_ELEMENT
    x = (p * np.float32(65536.0)).astype(np.float64)            # (a power of two: the float32 product is exact)
    if np.any(x >= 4294967296.0):
        return cdf, BAD_ELEMENT                                 # (the host's conversion to uint32 is undefined there)
    c = (np.floor(np.abs(x) + 0.5) * np.sign(x)).astype(np.uint64)      # std::round: halves away from zero
    total = int(c.sum())
    if total >= 1 << 32:
        return cdf, BAD_ELEMENT                                 # (the host's uint32 total would wrap)
    if total == 0:
        return cdf, ZERO_TOTAL
    q = (np.uint64(65536) * c) // np.uint64(total)
    cdf[1:] = np.cumsum(q).astype(np.uint32)
    cdf[k] = 65536
    cdf = cdf.astype(np.int64)
    for i in range(k):
        if cdf[i] == cdf[i + 1]:
            freq = cdf[1:] - cdf[:-1]
            spare = np.where(freq > 1, freq, np.int64(1) << 40)
            j = int(np.argmin(spare))                           # the first index among those of least frequency > 1
            if spare[j] == np.int64(1) << 40:
                return cdf.astype(np.uint32), NO_DONOR
            if j < i:
                cdf[j + 1: i + 1] -= 1
            else:
                cdf[i + 1: j + 1] += 1
    return cdf.astype(np.uint32), OK


def quantized_cdf_closed(pmf):
    """Valid rows only.  Widths after step 5; Z empty bins; donors give in ascending (width, index) order, each width - 1 counts: F = the
    least width with cap(F) = sum over {1 < w <= F} of (w - 1) >= Z by bisection, donors below F end at 1, those of width F give in
    index order (owed / (F - 1) of them everything, the next one the remainder); the table is the scan of the final widths."""
    p = np.asarray(pmf, dtype=np.float32)
    k = p.shape[0]
    c = np.floor(p.astype(np.float64) * 65536.0 + 0.5).astype(np.uint64)
    w = ((np.uint64(65536) * c) // np.uint64(int(c.sum()))).astype(np.int64)
    w[k - 1] = 65536 - (w.sum() - w[k - 1])
    empty = int((w == 0).sum())
    if empty:
        def cap(width):
            return int(np.where((w > 1) & (w <= width), w - 1, 0).sum())
        if cap(65536) < empty:
            return None
        lo, hi = 2, 65536
        while lo < hi:
            mid = (lo + hi) >> 1
            if cap(mid) >= empty:
                hi = mid
            else:
                lo = mid + 1
        full, rem = divmod(empty - cap(lo - 1), lo - 1)
        final = w.copy()
        final[(w == 0) | ((w > 1) & (w < lo))] = 1
        at = np.flatnonzero(w == lo)
        final[at[:full]] = 1
        if rem:
            final[at[full]] = lo - rem
        w = final
    return np.concatenate([[0], np.cumsum(w)]).astype(np.uint32)


def normalise(raw):
    raw = np.asarray(raw, dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = raw.astype(np.float64).sum(-1, keepdims=True).astype(np.float32)
        return (raw / s).astype(np.float32)


def code_bits(codes, tables):
    """codes: per level int64 [n, m, h, w]; tables: per level uint32 [m, k + 1] -> float64 [n, levels]."""
    n = codes[0].shape[0]
    out = np.zeros((n, len(codes)), dtype=np.float64)
    for lv, (code, table) in enumerate(zip(codes, tables)):
        table = np.asarray(table).astype(np.int64)
        for g in range(code.shape[1]):
            c = np.asarray(code[:, g]).reshape(n, -1)
            width = (table[g][c + 1] - table[g][c]).astype(np.float64)
            out[:, lv] += (16.0 - np.log2(width)).sum(-1)
    return out


def _rng(seed):
    return np.random.default_rng(seed)


def _pmf(k, seed, dead=0.0, power=2.0):
    g = _rng(seed)
    p = g.random(k) ** power + 1e-7
    if dead:
        p[g.random(k) < dead] = 0.0
    return (p / p.sum()).astype(np.float32)


def _counts(widths):
    """A row whose scaled counts are `widths` and, in one more bin at the end, the rest of 65536: the total is 65536, so step 3 keeps them."""
    c = np.array(list(widths) + [65536 - sum(widths)], np.float64)
    return (c / 65536.0).astype(np.float32)


def cases():
    """name -> float32 row; every one a valid table (status 0)."""
    out = {}
    out["k2"] = np.array([0.25, 0.75], np.float32)
    out["k2_one_empty"] = np.array([0.0, 1.0], np.float32)
    out["k3_one_zero"] = np.array([0.5, 0.0, 0.5], np.float32)
    out["k65"] = _pmf(65, 1)
    out["k65_dead"] = _pmf(65, 2, dead=0.4)
    out["k1000"] = _pmf(1000, 3)
    out["k1000_dead"] = _pmf(1000, 4, dead=0.3, power=6.0)
    one = np.zeros(513, np.float32)
    one[200] = 1.0
    out["all_mass_on_one"] = one                                 # 512 steals from one donor, below and above it
    # ties among donors: widths 2, 2, 2 around zeros -- the first of the least must give first, then the next
    out["donor_ties"] = _counts([0, 4, 2, 0, 2, 0, 2, 0, 0, 4, 0])
    # a donor below i and a donor above i in one row: index 1 (width 2) serves bin 0 from above, then index 2 (width 3) serves bins 4, 5
    # from below, then index 3 (width 5) serves bin 6 from below
    out["both_directions"] = _counts([0, 2, 3, 5, 0, 0, 0, 6])
    # a steal changes what later steps see: the only width-2 donor is used up by bin 0 (it keeps width 1, no donor any more), so bin 2
    # goes to the next larger donor although the first still lies beside it.  (A steal moves one count from the donor to bin i and leaves
    # every other width alone, so it never empties or fills a LATER bin: what an earlier steal changes for a later step is the donor.)
    out["donor_used_up"] = _counts([0, 2, 0, 5, 0, 9])
    big = _pmf(8192, 5, dead=0.55, power=4.0)
    out["k8192_more_than_half_zero"] = big
    out["k8192_uniform"] = np.full(8192, 1.0 / 8192, np.float32)
    out["k8192_plain"] = _pmf(8192, 6)
    # exact .5 products: p * 65536 = c + 0.5 exactly (p has few bits), rounded away from zero
    half = np.array([1.5, 2.5, 0.5, 3.5, 4.5, 100.5, 0.5, 7.5], np.float64) / 65536.0
    out["exact_halves"] = half.astype(np.float32)
    out["exact_halves_in_a_pmf"] = np.concatenate([half, [1.0 - half.sum()]]).astype(np.float32)
    out["k512_tiny_tail"] = _pmf(512, 7, power=12.0)
    return out


def bad_cases(k=65):
    """name -> (row, status): the rows for which the host function returns MCQ_EINVAL.  Its fourth cause, no donor left, needs more
    symbols than counts: the widths of a row always sum to 65536, so with k < 65536 bins one of them exceeds 1 at every step of the
    steal loop.  The device kernel takes k <= 8192 (its LDS row), where that status cannot arise; it keeps the check all the same."""
    nan = _pmf(k, 11)
    nan[k // 2] = np.nan
    inf = _pmf(k, 12)
    inf[3] = np.inf
    neg = _pmf(k, 13)
    neg[k - 1] = -1e-3
    return {"nan": (nan, BAD_ELEMENT), "inf": (inf, BAD_ELEMENT), "negative": (neg, BAD_ELEMENT), "all_zero": (np.zeros(k, np.float32), ZERO_TOTAL)}
