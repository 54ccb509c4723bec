"""CPU: the references of tests/_wgrad_refs.py against float64 torch.autograd over F.conv2d, at every geometry the GPU test
(tests/test_gpu_wgrad_leaf.py) launches -- stride 2 and the x^2 operand included."""
import pytest
import torch
import torch.nn.functional as F

import _wgrad_cases as K
import _wgrad_refs as W

GEOMS = sorted({(c.n, c.cin, c.h, c.w, c.cout, c.ks, c.stride, sq) for c in K.CASES for sq in K.squares(c)})
_IDS = ["{}x{}->{} {}x{} k{} s{}{}".format(n, ci, co, h, w, ks, st, " sq" if sq else "") for n, ci, h, w, co, ks, st, sq in GEOMS]


def _autograd64(x, dy, ks, stride, square):
    cout, cin = dy.shape[1], x.shape[1]
    wt = torch.zeros((cout, cin, ks, ks), dtype=torch.float64, requires_grad=True)
    b = torch.zeros((cout,), dtype=torch.float64, requires_grad=True)
    xd = x.double()
    y = F.conv2d(xd * xd if square else xd, wt, b, stride=stride, padding=ks // 2)
    assert y.shape == dy.shape
    y.backward(dy.double())
    return wt.grad, b.grad


@pytest.mark.parametrize("geom", GEOMS, ids=_IDS)
def test_references_against_float64_autograd(geom):
    n, cin, h, w, cout, ks, stride, square = geom
    pixels = n * W.out_hw(h, w, ks, stride)[0] * W.out_hw(h, w, ks, stride)[1]
    assert 27 * pixels < 2 ** 24, "the exactness premise of the integer data set"
    x, dy = W.uniform_inputs(n, cin, h, w, cout, ks, stride, 11)
    dw64, db64 = W.wgrad64(x, dy, ks, stride, square)
    aw, ab = _autograd64(x, dy, ks, stride, square)
    assert dw64.dtype == torch.float64 and dw64.shape == aw.shape and db64.shape == ab.shape
    assert float((dw64 - aw).abs().max()) <= 1e-12 * float(aw.abs().max()), "wgrad64 dW against autograd"
    assert float((db64 - ab).abs().max()) <= 1e-12 * float(ab.abs().max()), "wgrad64 db against autograd"
    sw, sb = W.wgrad_scale64(x, dy, ks, stride, square)
    assert bool((sw >= dw64.abs()).all()) and bool((sb >= db64.abs()).all())
    # one float32 chain of K products: within K u of the exact sum, relative to the magnitude of its terms
    qw, qb = W.wgrad_seq_f32(x, dy, ks, stride, square)
    assert qw.dtype == torch.float32 and qb.dtype == torch.float32
    assert W.rel_err(qw, dw64, sw) <= pixels * W.U and W.rel_err(qb, db64, sb) <= pixels * W.U
    # integer data: the int64 sums are the float64 sums, and the float32 chain reaches them exactly
    xi, di = W.int_inputs(n, cin, h, w, cout, ks, stride, 12)
    assert float(xi.abs().max()) <= 3 and float(di.abs().max()) <= 3
    iw, ib = W.wgrad_int(xi, di, ks, stride, square)
    ew, eb = W.wgrad64(xi, di, ks, stride, square)
    assert iw.dtype == torch.int64 and torch.equal(iw.double(), ew) and torch.equal(ib.double(), eb)
    assert int(iw.abs().max()) < 2 ** 24
    aw, ab = _autograd64(xi, di, ks, stride, square)
    assert torch.equal(iw.double(), aw) and torch.equal(ib.double(), ab)
    if pixels <= 256:
        zw, zb = W.wgrad_seq_f32(xi, di, ks, stride, square)
        assert torch.equal(zw.double(), ew) and torch.equal(zb.double(), eb)


def test_a_misplaced_pixel_shows_in_the_integer_sums():
    """What the exact data set is for: one input pixel moved by one column changes the int64 sums."""
    x, dy = W.int_inputs(1, 2, 4, 8, 2, 3, 1, 5)
    x[0, 0, 1, 2], x[0, 0, 1, 3] = 3.0, -2.0
    dy[0, 0, 1, 2] = 1.0
    a = W.wgrad_int(x, dy, 3, 1)[0]
    x2 = x.clone()
    x2[0, 0, 1, 2], x2[0, 0, 1, 3] = x[0, 0, 1, 3], x[0, 0, 1, 2]
    assert not torch.equal(a, W.wgrad_int(x2, dy, 3, 1)[0])
