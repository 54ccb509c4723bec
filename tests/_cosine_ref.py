"""Float64 reference of the codebook cosine regulariser (mcquic/loss/__init__.py:32-41) and of its gradient, in row chunks: at
k = 8192 no [k, k] float64 plane exists at once.

    loss   = sum over groups and pairs i < j of clamp(cos_ij, 0, 2),  cos_ij = <c_i, c_j> / s_ij,  s_ij = sqrt(n_i n_j)
    grad_i = sum_{j != i, 0 <= cos_ij <= 2} ( c_j / s_ij - cos_ij c_i / n_i )          (gamma = dout = 1)

The gradient jumps by c_j / s_ij where a cosine crosses 0, and a float32 evaluation may land on the other side of 0 than float64
does.  The pairs where that is legitimate are the AMBIGUOUS ones, |cos64| <= tau(d) = 2 (d + 4) 2^-24: a float32 dot product of
length d is off by at most d u sum|a_t b_t| (u = 2^-24), sum|a_t b_t| <= s_ij by Cauchy-Schwarz, and the factor 2 and the + 4
cover the two norms, the square root and the division.  `slack[g, i]` = sum over the ambiguous j of |c_j|_inf / s_ij bounds what
those pairs can move row i by."""
import math

import torch


def tau(d: int) -> float:
    return 2.0 * (d + 4) * 2.0 ** -24


def make_codebook(m: int, k: int, d: int, seed: int) -> torch.Tensor:
    """[m, k, d] float32 at the model's initialisation scale: group g is the g-th randn(k, d) draw of one generator."""
    gen = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randn(k, d, generator=gen) * math.sqrt(2 / (5 * d)) for _ in range(m)])


class CosineRef:
    """loss (float), grad [m, k, d] float64, pairs (per group an int64 [n, 2] of the ambiguous (i, j), i < j), slack [m, k] float64."""

    def __init__(self, loss, grad, pairs, slack):
        self.loss, self.grad, self.pairs, self.slack = loss, grad, pairs, slack

    @property
    def n_ambiguous(self) -> int:
        return sum(int(p.shape[0]) for p in self.pairs)

    @property
    def ambiguous_rows(self) -> float:
        """Fraction of the rows with a non-empty A(i)."""
        return float((self.slack > 0).double().mean())


def cosine_ref(codebook: torch.Tensor, want_grad: bool = True, chunk: int = 512) -> CosineRef:
    cb = codebook.detach().cpu().double()
    m, k, d = cb.shape
    t = tau(d)
    loss = 0.0
    grad = torch.zeros_like(cb) if want_grad else None
    slack = torch.zeros(m, k, dtype=torch.float64)
    pairs = []
    cols = torch.arange(k)
    for g in range(m):
        c = cb[g]
        n = (c * c).sum(-1)
        cinf = c.abs().amax(-1)
        found = []
        for r0 in range(0, k, chunk):
            rows = torch.arange(r0, min(k, r0 + chunk))
            s = (n[rows, None] * n[None, :]).sqrt()
            cos = (c[rows] @ c.T) / s
            off = rows[:, None] != cols[None, :]
            upper = cols[None, :] > rows[:, None]
            loss += float(torch.where(upper, cos.clamp(0.0, 2.0), torch.zeros_like(cos)).sum())
            amb = off & (cos.abs() <= t)
            slack[g, rows] = torch.where(amb, cinf[None, :] / s, torch.zeros_like(s)).sum(-1)
            ij = (amb & upper).nonzero()
            if ij.numel():
                found.append(torch.stack([rows[ij[:, 0]], ij[:, 1]], dim=1))
            if want_grad:
                mask = (off & (cos >= 0.0) & (cos <= 2.0)).double()
                grad[g, rows] = (mask / s) @ c - ((mask * cos).sum(-1) / n[rows])[:, None] * c[rows]
        pairs.append(torch.cat(found) if found else torch.zeros(0, 2, dtype=torch.int64))
    return CosineRef(loss, grad, pairs, slack)


def torch_formula(codebook: torch.Tensor) -> torch.Tensor:
    """The reference's formula as written (mcquic/loss/__init__.py:32-41), in the dtype of `codebook`."""
    losses = []
    for c in codebook:
        pairwise = c @ c.T
        norm = (c ** 2).sum(-1)
        cos = pairwise / (norm[:, None] * norm).sqrt()
        losses.append(cos.triu(1).clamp(0.0, 2).sum())
    return sum(losses)


def loss_error(got: float, ref: float) -> float:
    """Relative error of a loss (absolute where the reference is 0)."""
    return abs(got - ref) / abs(ref) if ref != 0 else abs(got)


def grad_error(got: torch.Tensor, ref: CosineRef, scale: float = 1.0):
    """(err, worst row): the largest per-row excess max(0, |got_i - scale ref_i|_inf - |scale| slack_i) over max |scale ref|.
    Rows without an ambiguous pair have slack 0: they get no allowance."""
    want = ref.grad * scale
    dev = (got.detach().cpu().double() - want).abs().amax(-1)
    excess = (dev - abs(scale) * ref.slack).clamp_min(0.0)
    top = float(want.abs().max())
    return float(excess.max()) / (top if top > 0 else 1.0), int(excess.argmax())
