"""SGD as mcquic_amd.optim.SGD specifies it, restated in float64 with torch on the CPU, from the formulas and not from torch.optim.SGD
(tests/test_sgd_ref.py compares the two).  It shares no code with mcquic_amd/optim.py.  One update over a list of tensors:

    G = sqrt(sum over every tensor of sum grad^2)                          (only with max_grad_norm or skip_nonfinite)
    skip_nonfinite and G not finite: nothing changes, skipped += 1
    c = min(1, max_grad_norm / (G + 1e-6))  (1 without max_grad_norm);  g = c grad
    g = -g if maximize;  g += weight_decay p
    momentum != 0:  buf = g on the first update that is not skipped, else buf = momentum buf + (1 - dampening) g
                    g = g + momentum buf if nesterov else buf
    p -= lr g
"""
import itertools
import math

import torch


def settings():
    """Every valid combination of momentum {0, 0.9} x dampening {0, 0.1} x nesterov x weight_decay {0, 1e-2} x maximize (Nesterov
    needs a momentum and no dampening: 20 of the 32)."""
    out = []
    for m, d, n, w, x in itertools.product([0.0, 0.9], [0.0, 0.1], [False, True], [0.0, 1e-2], [False, True]):
        if n and (m == 0.0 or d != 0.0):
            continue
        out.append(dict(momentum=m, dampening=d, nesterov=n, weight_decay=w, maximize=x))
    return out


def setting_id(kw):
    return ",".join(f"{k[:3]}={v}" for k, v in kw.items())


class RefSGD:
    """`params`: float64 CPU tensors, updated in place.  After `update(grads)`: `grad_norm` (None without either option), `skipped`,
    `steps` (updates that went through), `bufs` (None before the first one, or without momentum)."""

    def __init__(self, params, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, maximize=False, max_grad_norm=None,
                 skip_nonfinite=False):
        assert all(p.dtype == torch.float64 and p.device.type == "cpu" for p in params)
        self.params, self.lr = params, lr
        self.momentum, self.dampening, self.weight_decay, self.nesterov, self.maximize = momentum, dampening, weight_decay, nesterov, maximize
        self.max_grad_norm, self.skip_nonfinite = max_grad_norm, skip_nonfinite
        self.bufs = [None] * len(params)
        self.steps, self.skipped, self.grad_norm = 0, 0, None

    def update(self, grads, lr=None):
        lr = self.lr if lr is None else lr
        grads = [g.detach().double().cpu() for g in grads]
        c = 1.0
        if self.max_grad_norm is not None or self.skip_nonfinite:
            G = math.sqrt(sum(float((g * g).sum()) for g in grads))
            self.grad_norm = G
            if self.skip_nonfinite and not math.isfinite(G):
                self.skipped += 1
                return
            if self.max_grad_norm is not None:
                c = min(1.0, self.max_grad_norm / (G + 1e-6))
        first = self.steps == 0
        for i, (p, grad) in enumerate(zip(self.params, grads)):
            g = grad * c
            if self.maximize:
                g = -g
            g = g + self.weight_decay * p
            if self.momentum != 0.0:
                self.bufs[i] = g.clone() if first else self.momentum * self.bufs[i] + (1.0 - self.dampening) * g
                g = g + self.momentum * self.bufs[i] if self.nesterov else self.bufs[i]
            p -= lr * g
        self.steps += 1
