"""The exponential moving average as mcquic_amd.optim.EMA specifies it, restated in float64 with torch on the CPU, from the formulas and
not from torch.optim.swa_utils (tests/test_ema_ref.py compares the two).  It shares no code with mcquic_amd/optim.py.  One update:

    n = updates made before this one
    d_t = decay;  with warm-up  d_t = min(decay, (1 + n) / (10 + n))
    avg += (1 - d_t) (p - avg)
"""
import torch


def decay_at(decay: float, n: int, warmup: bool) -> float:
    """d_t of the update that follows `n` earlier ones."""
    return min(decay, (1.0 + n) / (10.0 + n)) if warmup else decay


class RefEMA:
    """`averages`: float64 CPU copies of `params` at construction; `update(params)` takes the current values.  `decays` records every
    d_t used, `num_updates` counts."""

    def __init__(self, params, decay, warmup=False):
        self.averages = [p.detach().double().cpu().clone() for p in params]
        self.decay, self.warmup = float(decay), warmup
        self.num_updates, self.decays = 0, []

    def update(self, params, decay=None):
        d = decay_at(self.decay if decay is None else float(decay), self.num_updates, self.warmup)
        self.decays.append(d)
        for a, p in zip(self.averages, params):
            a += (1.0 - d) * (p.detach().double().cpu() - a)
        self.num_updates += 1
