"""Inputs of the StepMeter leaf tests (tests/test_gpu_step_meter.py on the device, tests/test_meter_ref.py for the float32 figures on
the CPU): level sets, frequency tables with entries on both sides of CodeUsage's threshold, and the count patterns."""
import numpy as np

# (m_l, k_l): one entry (entropy exactly 0); a row shorter than a wave; k no multiple of 64 / 256; the product's three levels at full
# width; groups that differ per level (VariousMQuantizer)
LEVEL_SETS = {"1x1": [(1, 1)], "2x3": [(2, 3)], "64+257": [(1, 64), (3, 257)], "product": [(2, 8192), (2, 2048), (2, 512)],
              "various-m": [(4, 65), (1, 1023)]}
COUNT_KINDS = ("random", "zero-group", "one-hot", "uniform", "above-2^24")
THRESHOLD, MARGIN = 1e-6, 2.0 ** -20


def freqs(levels, seed):
    """float32 [m, k] tables: random, 30 % of the entries 0, and in every row with k >= 3 entry 1 at 1e-6 (1 + 2^-20) of the row's sum and
    entry 2 at 1e-6 (1 - 2^-20) of it (float32 rounds at 2^-24: the two stay on their sides).  Rows are left unnormalised, as an EMA is."""
    rng = np.random.default_rng(seed)
    out = []
    for m, k in levels:
        f = rng.random((m, k)).astype(np.float32)
        f[rng.random((m, k)) < 0.3] = 0.0
        f[:, 0] = np.maximum(f[:, 0], np.float32(0.25))       # (no all-zero row)
        if k >= 3:
            for g in range(m):
                for _ in range(4):                            # (the two entries move the sum by 2e-6 of itself: converges at once)
                    s = f[g].astype(np.float64).sum()
                    f[g, 1] = np.float32(THRESHOLD * (1 + MARGIN) * s)
                    f[g, 2] = np.float32(THRESHOLD * (1 - MARGIN) * s)
        out.append(f)
    return out


def counts(levels, kind, seed):
    """int64 [m, k] histograms of one step."""
    rng = np.random.default_rng(seed)
    out = [rng.integers(0, 50, (m, k), dtype=np.int64) for m, k in levels]
    if kind == "zero-group":                                  # no code of the first level's first group was used
        out[0][0, :] = 0
    elif kind == "one-hot":                                   # every code of the last level's first group is the same one
        out[-1][0, :] = 0
        out[-1][0, levels[-1][1] // 2] = 7
    elif kind == "uniform":                                   # every codeword equally often, everywhere
        out = [np.full((m, k), 3, dtype=np.int64) for m, k in levels]
    elif kind == "above-2^24":                                # a count float32 cannot hold, next to small ones
        out[0][0, 0] = (1 << 24) + 1
    elif kind != "random":
        raise ValueError(kind)
    return out


def losses(n, seed):
    """float32 losses in [0.01, 0.5]: 3 to 20 dB under upper bound 1."""
    return (0.01 + 0.49 * np.random.default_rng(seed).random(n)).astype(np.float32)
