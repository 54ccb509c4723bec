"""CPU: the references of tests/_soft_bwd_refs.py against float64 autograd.  The forward is written out in torch -- the distance
|x|^2 - 2 x.C + |C|^2 of every vector to every codeword of its group and the soft dequantisation hot * C[index] -- and a given
(ddist, dDeq) is backpropagated; rowsum is the row sum of ddist, as the softmax backward hands it over.  soft_bwd64 must agree to
1e-12 of the largest entry, soft_bwd_int must EQUAL soft_bwd64 on integer data, the one-chain float32 form stays within its own
forward error bound of float64, and the scale is what its name says."""
import pytest
import torch

import _soft_bwd_cases as K
import _soft_bwd_refs as S

SHAPES = [(2, 3, 5, 3, 4, 7), (1, 1, 1, 1, 1, 1), (3, 2, 33, 2, 2, 40), (2, 2, 8, 4, 8, 128)]


def _autograd(ddist, x, cb, ddeq, index, hot):
    n, m, h, w, k = ddist.shape
    d = cb.shape[2]
    xr, cr = x.double().requires_grad_(), cb.double().requires_grad_()
    xv = xr.reshape(n, m, d, h * w).permute(0, 1, 3, 2)                                   # [n, m, hw, d]
    dist = (xv * xv).sum(-1, keepdim=True) - 2 * torch.einsum("ngvj,gcj->ngvc", xv, cr) + (cr * cr).sum(-1)[None, :, None, :]
    g = torch.arange(m).reshape(1, m, 1).expand(n, m, h * w)
    deq = hot.double().reshape(n, m, h * w, 1) * cr[g, index.reshape(n, m, h * w)]        # [n, m, hw, d]
    deq = deq.permute(0, 1, 3, 2).reshape(n, m * d, h, w)
    torch.autograd.backward([dist, deq], [ddist.double().reshape(n, m, h * w, k), ddeq.double()])
    return xr.grad, cr.grad


@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
@pytest.mark.parametrize("kind", ["int", "uniform"])
def test_soft_bwd64_is_float64_autograd(shape, kind):
    n, m, d, h, w, k = shape
    ddist, _, x, cb, ddeq, hot = (S.int_inputs if kind == "int" else S.uniform_inputs)(*shape, seed=21)
    index = K.index_pattern(n, m, h, w, k)
    rowsum = ddist.double().sum(-1)                                  # (float64: autograd sums the row itself)
    want_dx, want_dc = _autograd(ddist, x, cb, ddeq, index, hot)
    dx, dc = S.soft_bwd64(ddist, rowsum, x, cb, ddeq, index, hot)
    for got, want, what in ((dx, want_dx, "dx"), (dc, want_dc, "dC")):
        assert got.dtype == torch.float64 and got.shape == want.shape
        assert float((got - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1.0), what
    if kind == "int":
        ix, ic = S.soft_bwd_int(ddist, rowsum.float(), x, cb, ddeq, index, hot)
        assert ix.dtype == torch.int64 and torch.equal(ix.double(), dx) and torch.equal(ic.double(), dc)


def test_scatter_adds_duplicates_and_groups_apart():
    """Three vectors on one codeword add up; a group's hits land in its own codebook."""
    n, m, d, h, w, k = 1, 2, 2, 1, 3, 4
    z = torch.zeros
    index = torch.tensor([2, 2, 2, 0, 1, 0]).reshape(n, m, h, w)
    hot = torch.tensor([1.0, 2.0, 3.0, 1.0, 1.0, -1.0]).reshape(n, m, h, w)
    ddeq = torch.ones((n, m * d, h, w))
    for fn in (S.soft_bwd64, S.soft_bwd_seq_f32, S.soft_bwd_int):
        _, dc = fn(z((n, m, h, w, k)), z((n, m, h, w)), z((n, m * d, h, w)), z((m, k, d)), ddeq, index, hot)
        want = z((m, k, d))
        want[0, 2] = 6.0
        want[1, 1] = 1.0                                             # (group 1, codeword 0: 1 - 1)
        assert torch.equal(dc.to(torch.float32), want), fn.__name__
    _, sc = S.soft_bwd_scale64(z((n, m, h, w, k)), z((n, m, h, w)), z((n, m * d, h, w)), z((m, k, d)), ddeq, index, hot)
    assert float(sc[1, 0, 0]) == 2.0 and float(sc[0, 2, 1]) == 6.0     # the scale of a sum that cancels is its terms'


@pytest.mark.parametrize("shape", SHAPES, ids=[str(s) for s in SHAPES])
def test_seq_f32_and_scale(shape):
    n, m, d, h, w, k = shape
    ddist, rowsum, x, cb, ddeq, hot = S.uniform_inputs(*shape, seed=22)
    index = K.index_pattern(n, m, h, w, k)
    args = (ddist, rowsum, x, cb, ddeq, index, hot)
    dx64, dc64 = S.soft_bwd64(*args)
    sx, sc = S.soft_bwd_scale64(*args)
    assert bool((sx >= dx64.abs() * (1 - 1e-12)).all()) and bool((sc >= dc64.abs() * (1 - 1e-12)).all())
    qx, qc = S.soft_bwd_seq_f32(*args)
    assert qx.dtype == torch.float32 and qc.dtype == torch.float32
    u = 2.0 ** -24
    # a chain of t fma steps and the three roundings of the combination: (t + 3) u of the terms' magnitudes, first order
    assert S.rel_err(qx, dx64, sx) <= 1.01 * (k + 3) * u
    assert S.rel_err(qc, dc64, sc) <= 1.01 * (n * h * w + 4) * u
    ix = S.int_inputs(*shape, seed=23)
    iargs = (ix[0], ix[1], ix[2], ix[3], ix[4], index, ix[5])
    want_x, want_c = S.soft_bwd_int(*iargs)
    got_x, got_c = S.soft_bwd_seq_f32(*iargs)
    assert torch.equal(got_x.to(torch.int64), want_x) and torch.equal(got_c.to(torch.int64), want_c), "integer data: the float32 chain is exact"


def test_index_pattern_is_in_range_and_differs_by_group():
    for c in K.CASES:
        idx = K.index_pattern(c.n, c.m, c.h, c.w, c.k)
        assert idx.dtype == torch.int64 and tuple(idx.shape) == (c.n, c.m, c.h, c.w)
        assert int(idx.min()) >= 0 and int(idx.max()) < c.k, c.name
        if c.m > 1 and c.k > 11:
            assert not torch.equal(idx[:, 0], idx[:, 1]), c.name
