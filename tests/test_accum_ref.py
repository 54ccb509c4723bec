"""CPU: the accumulation rule of GraphedTrainStep(accumulate=k) as tests/_accum_ref.py states it -- what the GPU tests compare the kernels
with bit for bit -- and the host side of the two entry points (declared, bound, refusing bad arguments without a device)."""
import os
import re

import pytest
import torch

import _accum_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bits(t):
    return t.contiguous().view(torch.int32)


def test_same_tensor_twice_gives_it_back():
    """k = 2: (g + g) * 0.5 is exact for every float32 whose double does not overflow -- +-0 keep their sign, denormals their bits."""
    g = A.hard_values(1 << 14, 31)
    assert bool((g.view(torch.int32) == 1).any()) and bool((g == 0).any())
    out = A.accum_all([g, g])
    assert torch.equal(_bits(out), _bits(g))
    assert float(A.inv_k(2)) == 0.5 and float(A.inv_k(4)) == 0.25 and float(A.inv_k(3)) == float(torch.tensor(1 / 3, dtype=torch.float32))


@pytest.mark.parametrize("k", [3, 4])
def test_the_rule_is_not_the_mean_rounded_once(k):
    """The in-order float32 sum times fl(1 / k) differs from the float64 mean rounded once, and from another summation order, on the
    inputs the GPU test uses: a kernel with the wrong order cannot pass there.  (Found by search at this seed; the counts are asserted.)"""
    gs = [A.hard_values(1 << 12, 100 + j) for j in range(k)]
    rule = A.accum_all(gs)
    once = A.mean_rounded_once(gs)
    differs = int((_bits(rule) != _bits(once)).sum())
    assert differs > 0, "no element tells the rule from the once-rounded mean"
    back = A.accum_all(gs[::-1])                               # ((g_{k-1} + ...) + g0): the reversed order
    assert int((_bits(rule) != _bits(back)).sum()) > 0, "no element tells the summation order"
    # and it IS the definition, written out once more without the helper
    acc = gs[0].clone()
    for g in gs[1:]:
        acc = acc + g
    assert torch.equal(_bits(rule), _bits(acc * A.inv_k(k)))


def test_counts_sum_exactly_and_loss_is_the_mean():
    gen = torch.Generator().manual_seed(5)
    cs = [torch.randint(0, 1 << 40, (1000,), generator=gen, dtype=torch.int64) for _ in range(4)]
    cs[1][0] = 1 << 40
    acc = None
    for j, c in enumerate(cs):
        acc = A.accum_counts(acc, c, j)
    assert torch.equal(acc, cs[0] + cs[1] + cs[2] + cs[3]) and int(acc.max()) > 1 << 40
    assert int(acc[0]) == sum(int(c[0]) for c in cs)            # (python integers: no float on the way)
    losses = [torch.tensor(v, dtype=torch.float32) for v in (0.1234567, 0.7654321, 0.3333333)]
    got = float(A.accum_all(losses))
    assert abs(got - sum(float(v) for v in losses) / 3) <= 2 ** -24 * 4 * got


def test_entry_points_are_declared_bound_and_refuse_bad_arguments():
    from mcquic_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mcquic_hip.h")).read()
    for name in ("mcq_gather_accum_flat_f32", "mcq_accum_step_scalars"):
        assert name in _lib.SYMBOLS and re.search(r"\b%s\s*\(" % name, header) and getattr(lib, name) is not None
    one = 4096                                                 # (a non-null address: refused before anything is launched)
    assert lib.mcq_gather_accum_flat_f32(one, one, one, one, one, one, 1, one, 1, None) == _lib.MCQ_EINVAL       # k = 1: the copy kernel's job
    assert lib.mcq_gather_accum_flat_f32(one, one, one, one, one, one, 1, None, 2, None) == _lib.MCQ_EINVAL      # no phase word
    assert lib.mcq_gather_accum_flat_f32(None, one, one, one, one, one, 1, one, 2, None) == _lib.MCQ_EINVAL
    assert lib.mcq_gather_accum_flat_f32(one, one, one, one, one, one, 0, one, 2, None) == _lib.MCQ_EINVAL
    assert lib.mcq_accum_step_scalars(one, one, 8, one, one, one, 1, None) == _lib.MCQ_EINVAL
    assert lib.mcq_accum_step_scalars(one, one, 8, one, one, None, 2, None) == _lib.MCQ_EINVAL
    assert lib.mcq_accum_step_scalars(None, None, 0, None, None, one, 2, None) == _lib.MCQ_EINVAL                # nothing to do
    assert lib.mcq_accum_step_scalars(one, None, 8, None, None, one, 2, None) == _lib.MCQ_EINVAL
    assert lib.mcq_accum_step_scalars(one, one, 0, None, None, one, 2, None) == _lib.MCQ_EINVAL
    assert lib.mcq_accum_step_scalars(None, None, 0, one, None, one, 2, None) == _lib.MCQ_EINVAL


def test_accumulate_is_a_keyword_of_the_step_with_default_one():
    """(The step itself needs a device: tests/test_gpu_accum_step.py.)"""
    import inspect
    from mcquic_amd import parallel
    assert inspect.signature(parallel.GraphedTrainStep.__init__).parameters["accumulate"].default == 1
