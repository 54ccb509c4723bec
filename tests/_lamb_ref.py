"""LAMB written from its specification (the docstring of mcquic_amd.optim.Lamb; apex FusedLAMB's published algorithm) with torch
element-wise operations and tensor.norm(): dtype- and device-generic, so it is the float64 truth on the CPU and the float32
restatement on the device.  It shares no code with mcquic_amd/optim.py.  After a step `grad_norm` holds G and `ratios[group]` the
||p|| / ||u|| of the group's tensors that had a gradient."""
import torch


class RefLamb(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, bias_correction=True, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, adam_w_mode=True,
                 grad_averaging=True, max_grad_norm=1.0, use_nvlamb=False):
        super().__init__(params, dict(lr=lr, bias_correction=bias_correction, betas=betas, eps=eps, weight_decay=weight_decay,
                                      grad_averaging=grad_averaging, max_grad_norm=max_grad_norm))
        self.adam_w_mode, self.use_nvlamb = adam_w_mode, use_nvlamb
        self.grad_norm, self.ratios = None, {}

    @torch.no_grad()
    def step(self, closure=None):
        grads = [p.grad for g in self.param_groups for p in g["params"] if p.grad is not None]
        G = torch.stack([g.norm() for g in grads]).norm()
        self.grad_norm = G
        for gi, group in enumerate(self.param_groups):
            limit = group["max_grad_norm"]
            c = torch.where(G > limit, G / limit, torch.ones_like(G))
            b1, b2 = group["betas"]
            b3 = 1.0 - b1 if group["grad_averaging"] else 1.0
            t = group["step"] = group.get("step", 0) + 1
            bc1 = 1.0 - b1 ** t if group["bias_correction"] else 1.0
            bc2 = 1.0 - b2 ** t if group["bias_correction"] else 1.0
            lr, wd, eps = group["lr"], group["weight_decay"], group["eps"]
            lr = lr.to(G.dtype) if torch.is_tensor(lr) else lr
            self.ratios[gi] = []
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st["exp_avg"], st["exp_avg_sq"] = torch.zeros_like(p), torch.zeros_like(p)
                m, v = st["exp_avg"], st["exp_avg_sq"]
                g = p.grad / c
                if not self.adam_w_mode:
                    g = g + wd * p
                m.mul_(b1).add_(g, alpha=b3)
                v.mul_(b2).add_(g * g, alpha=1.0 - b2)
                u = (m / bc1) / ((v / bc2).sqrt() + eps)
                if self.adam_w_mode:
                    u = u + wd * p
                pn, un = p.norm(), u.norm()
                self.ratios[gi].append(pn / un)
                r = lr
                if self.use_nvlamb or wd != 0:
                    r = torch.where((pn != 0) & (un != 0), lr * (pn / un), lr * torch.ones_like(pn))
                p.sub_(r * u)
