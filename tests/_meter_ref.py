"""The telemetry row of mcquic_amd.monitor.StepMeter restated with numpy in float64, from the formulas and the reference, sharing no
code with mcquic_amd/monitor.py or csrc/step_meter.hip:

    db          Decibel.forward, mcquic/validate/utils.py:6-12:            -10 log10(loss / upperBound^2)
    db_ema      EMATracker.forward, mcquic/validate/utils.py:22-28:        the first value while the shadow is NaN, then
                                                                           shadow -= (1 - momentum) (shadow - db)
    watchdog    mcquic/train/trainer.py:435-437:                           isnan(moment) or moment < 0.1 (here also a loss or a norm
                                                                           that is not finite), remembered with its step number
    code_usage  Compressor.CodeUsage, mcquic/modules/compressor.py:211-212: mean over all entries of all levels of (f / sum f > 1e-6)
    bpp         IdealBPP, mcquic/validate/handlers.py:110-187:             sum over levels and groups of count * entropy(histogram), per pixel
    per level   usage (used / entries), ema_entropy (entropy of the normalised frequency rows, mean over groups), hit (codewords with a
                non-zero count / entries), step_entropy (sum_g total_g H_g / sum_g total_g, 0 without codes)

`dtype=np.float32` evaluates the same sums in float32: the order of magnitude a float32 kernel's error should have.  `ema_f32` is the
EMATracker recurrence in float32, rounding where torch's float32 kernels round; the kernel must match it bit for bit."""
import numpy as np

HEAD = 8


def _xlog2x(x):
    out = np.zeros_like(x)
    pos = x > 0
    out[pos] = x[pos] * np.log2(x[pos])
    return out


def level_partials(freq, counts, dtype=np.float64):
    """freq [m, k] (float32 values), counts [m, k] (int64) -> used, ema_entropy, hit, total, step_bits, each [m]."""
    f = np.asarray(freq).astype(dtype)
    c = np.asarray(counts).astype(np.int64)
    s = f.sum(-1, keepdims=True, dtype=dtype)
    p = np.divide(f, s, out=np.zeros_like(f), where=s > 0)
    used = (p > dtype(1e-6)).sum(-1)                           # strict
    ema_entropy = -_xlog2x(p).sum(-1, dtype=dtype)
    hit = (c != 0).sum(-1)
    total = c.sum(-1)
    t = total.astype(dtype)[:, None]
    q = np.divide(c.astype(dtype), t, out=np.zeros(c.shape, dtype), where=t > 0)
    step_bits = total.astype(dtype) * -_xlog2x(q).sum(-1, dtype=dtype)
    return used, ema_entropy, hit, total, step_bits


def decibel(loss, upper_bound=1.0):
    with np.errstate(all="ignore"):
        return -10.0 * np.log10(np.float64(loss) / np.float64(upper_bound) ** 2)


def row(freqs, counts, loss, pixels, upper_bound=1.0, dtype=np.float64):
    """The columns that depend on this step alone: a float64 vector [8 + 4 levels] with NaN where `db_ema`, `grad_norm`, `lr` and
    `skipped` go (they are inputs or carried state), and the per-level partials."""
    out = np.full(HEAD + 4 * len(freqs), np.nan)
    out[0], out[1] = loss, decibel(loss, upper_bound)
    used_all = entries_all = 0
    bits_all = 0.0
    parts = []
    for l, (f, c) in enumerate(zip(freqs, counts)):
        used, ent, hit, total, bits = level_partials(f, c, dtype)
        parts.append((used, ent, hit, total, bits))
        m, k = np.asarray(f).shape
        o = HEAD + 4 * l
        out[o] = used.sum() / (m * k)
        out[o + 1] = ent.astype(np.float64).sum() / m
        out[o + 2] = hit.sum() / (m * k)
        out[o + 3] = bits.astype(np.float64).sum() / total.sum() if total.sum() > 0 else 0.0
        used_all += int(used.sum())
        entries_all += m * k
        bits_all += float(bits.astype(np.float64).sum())
    out[6] = used_all / entries_all
    out[7] = bits_all / pixels
    return out, parts


def ema_f32(shadow, db, momentum=0.99):
    """One EMATracker.forward in float32: `shadow` and `db` are float32 values, 1 - momentum is a Python float that torch casts to float32."""
    shadow, db = np.float32(shadow), np.float32(db)
    if np.isnan(shadow):
        return db
    with np.errstate(all="ignore"):
        d = np.float32(shadow - db)
        t = np.float32(np.float32(1.0 - momentum) * d)
        return np.float32(shadow - t)


def is_bad(loss, grad_norm, shadow, floor=0.1):
    bad = not np.isfinite(loss) or (grad_norm is not None and not np.isfinite(grad_norm)) or bool(np.isnan(shadow))
    return bad or (floor is not None and bool(np.float32(shadow) < np.float32(floor)))
