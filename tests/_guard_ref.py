"""float64 restatement of the step guard (csrc/step_guard.hip): the flag, the norm and the counters, from the gradients alone.

    skip = !isfinite(G),  G = sqrt(sum g^2) over every gradient (float64 squares and sums: 1e19 per element does not overflow)
    skipped += skip;  consecutive = consecutive + 1 if skip else 0;  grad_norm = float32(G)

`np.sum` over float64 squares (pairwise) is the reference; the kernels' fixed trees differ from it by float64 rounding only, far below
the float32 rounding of the stored norm."""
import math

import numpy as np


def norm(grads) -> float:
    """G over a list of arrays (any shapes), in float64; inf / NaN propagate as IEEE has them."""
    total = 0.0
    with np.errstate(over="ignore", invalid="ignore"):
        for g in grads:
            g = np.asarray(g, dtype=np.float64).ravel()
            total += float(np.sum(g * g))
    return math.sqrt(total) if total == total and total >= 0.0 else float("nan")


def step(record, grads):
    """One guard call: `record` = dict(skip, grad_norm, skipped, consecutive) -> the next record."""
    G = norm(grads)
    skip = 0 if math.isfinite(G) else 1
    return dict(skip=skip, grad_norm=np.float32(G), skipped=record["skipped"] + skip, consecutive=record["consecutive"] + 1 if skip else 0)


def fresh():
    return dict(skip=0, grad_norm=np.float32(0.0), skipped=0, consecutive=0)


def run(batches):
    """The records after each of a sequence of gradient lists."""
    rec, out = fresh(), []
    for grads in batches:
        rec = step(rec, grads)
        out.append(rec)
    return out
