"""Reference of the gradient-accumulation arithmetic of parallel.GraphedTrainStep(accumulate=k), written from its definition in
torch on the CPU; nothing here calls the library.

Per element, in float32, micro-step `phase` of k (k >= 2):
    phase 0            acc = g
    0 < phase < k-1    acc = acc + g
    phase = k-1        acc = (acc + g) * fl(1 / k)          one add, then one multiply
so k micro-steps leave (((g0 + g1) + ...) + g_{k-1}) * fl(1 / k), fl(1 / k) being the float32 quotient 1.0f / (float)k.  The code
counts are int64 and are summed exactly (overwritten at phase 0); the loss is one float32 that follows the gradients' rule."""
import torch


def inv_k(k: int) -> torch.Tensor:
    """fl(1 / k): the correctly rounded float32 quotient."""
    return torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(k), dtype=torch.float32)


def accum(acc: torch.Tensor, g: torch.Tensor, phase: int, k: int) -> torch.Tensor:
    """The accumulator after micro-step `phase` (float32 CPU tensors; at phase 0 `acc` is not looked at)."""
    assert k >= 2 and 0 <= phase < k and g.dtype == torch.float32
    r = g.clone() if phase == 0 else acc + g
    return r * inv_k(k) if phase == k - 1 else r


def accum_all(gs) -> torch.Tensor:
    """All k = len(gs) micro-steps in order."""
    acc = None
    for j, g in enumerate(gs):
        acc = accum(acc, g, j, len(gs))
    return acc


def accum_counts(acc, c: torch.Tensor, phase: int) -> torch.Tensor:
    """The int64 count accumulator after micro-step `phase`: exact."""
    assert c.dtype == torch.int64
    return c.clone() if phase == 0 else acc + c


def mean_rounded_once(gs) -> torch.Tensor:
    """What the rule is NOT: the float64 sum divided by k, rounded to float32 once."""
    return (sum(g.double() for g in gs) / len(gs)).float()


def hard_values(n: int, seed: int) -> torch.Tensor:
    """n float32 values that tell summation orders and flushed denormals apart: normals over many binades, +-0, denormals (the
    smallest one included), and triples a, b, c (consecutive elements of three tensors drawn with seeds s, s+1, s+2 line up by index)
    of mixed sign and magnitude, for which (a + b) + c != a + (b + c) occurs."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, generator=g) * torch.exp2(torch.randint(-12, 13, (n,), generator=g).float())
    kind = torch.randint(0, 16, (n,), generator=g)
    x[kind == 0] = 0.0
    x[kind == 1] = -0.0
    den = torch.randint(1, 1 << 23, (n,), generator=g, dtype=torch.int32).view(torch.float32)       # positive denormals
    x = torch.where(kind == 2, den, x)
    x = torch.where(kind == 3, -den, x)
    x = torch.where(kind == 4, torch.tensor(1, dtype=torch.int32).view(torch.float32).expand(n), x)
    return x.contiguous()
