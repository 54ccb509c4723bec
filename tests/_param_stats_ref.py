"""The float64 reference of mcquic_amd.monitor.ParamStats, written from the column definitions and the recording rule (not from
csrc/param_stats.hip): numpy only, no device.  Shared by tests/test_param_stats_ref.py (hand-computed cases),
tests/test_gpu_param_stats_leaf.py and tests/test_gpu_param_stats_step.py.

    columns(w_after, g, w_before)      the five columns of one tensor, float64
    Recorder(tensors, capacity, every) the state words, the ring and `read()` of a run of `after()` calls
    within_one_ulp(got, want)          the bar of the three norms"""
import numpy as np

COLUMNS = ("weight_norm", "grad_norm", "grad_absmax", "grad_nonfinite", "update_norm")


def columns(w_after, g, w_before=None, updates=True):
    """[weight_norm, grad_norm, grad_absmax, grad_nonfinite, update_norm] of one tensor in float64.  `g` None: a gradient of zeros.
    `w_before` None with `updates`: a row that does not read the shadow (update_norm 0); without `updates`: NaN."""
    w = np.asarray(w_after, dtype=np.float64).ravel()
    g = np.zeros_like(w) if g is None else np.asarray(g, dtype=np.float64).ravel()
    finite = g[np.isfinite(g)]
    if not updates:
        upd = np.nan
    elif w_before is None:
        upd = 0.0
    else:
        upd = np.sqrt(np.sum((w - np.asarray(w_before, dtype=np.float64).ravel()) ** 2))
    return np.array([np.sqrt(np.sum(w * w)), np.sqrt(np.sum(finite * finite)), np.max(np.abs(finite)) if finite.size else 0.0,
                     float(g.size - finite.size), upd])


def is_recorded(count, every, skip):
    """(recorded, sampled) of the `after()` that finds `count`: sampled when count % every == 0, recorded when sampled or skipped."""
    sampled = count % every == 0
    return sampled or bool(skip), sampled


class Recorder:
    """What a ParamStats holds after a run of `after()` calls: feed it the float64 rows."""

    def __init__(self, tensors, capacity, every, updates=True):
        self.tensors, self.capacity, self.every, self.updates = tensors, capacity, every, updates
        self.count, self.rows, self.first_bad_step, self.first_bad_tensor = 0, 0, -1, -1
        self.steps = np.zeros(capacity, dtype=np.int64)
        self.ring = np.zeros((capacity, tensors, len(COLUMNS)))
        self.last_read = 0

    def after(self, w_after, grads, w_before, skip=False):
        """One step over lists of per-tensor arrays; `w_before`: the weights in front of the optimizer (read on sampled steps only).
        Returns (recorded, sampled)."""
        recorded, sampled = is_recorded(self.count, self.every, skip)
        if recorded:
            slot = self.rows % self.capacity
            for t in range(self.tensors):
                self.ring[slot, t] = columns(w_after[t], grads[t], w_before[t] if sampled else None, self.updates)
            bad = np.nonzero(self.ring[slot, :, 3] > 0)[0]
            if bad.size and self.first_bad_step < 0:
                self.first_bad_step, self.first_bad_tensor = self.count, int(bad[0])
            self.steps[slot] = self.count
            self.rows += 1
        self.count += 1
        return recorded, sampled

    def read(self):
        first = max(self.last_read, self.rows - self.capacity)
        dropped = max(0, first - self.last_read)
        slots = np.arange(first, max(first, self.rows)) % self.capacity
        out = {"steps": self.steps[slots].copy(), "dropped": dropped, "count": self.count, "first_bad_step": self.first_bad_step,
               "first_bad_tensor": self.first_bad_tensor}
        for i, name in enumerate(COLUMNS):
            out[name] = self.ring[slots][:, :, i].copy()
        self.last_read = max(self.last_read, self.rows)
        return out


def within_one_ulp(got, want):
    """Is every float32 of `got` within one float32 ulp (the spacing at the float64 `want`) of `want`?  NaN matches NaN, inf inf."""
    got, want = np.asarray(got, dtype=np.float32), np.asarray(want, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        close = np.abs(got.astype(np.float64) - want) <= ulp
    same = (np.isnan(got) & np.isnan(want)) | (got.astype(np.float64) == want)
    return close | same
