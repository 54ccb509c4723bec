"""References for the weight-gradient kernels (csrc/wgrad_rows.hip, csrc/wgrad_t16.h, the NHWC form of csrc/train_ops.hip): what
tests/test_gpu_wgrad_leaf.py compares a launch with (tests/test_wgrad_refs.py holds them to float64 autograd on the CPU).  Nothing
here imports mcquic_amd: every reference is the mathematics, written with torch / numpy on the CPU.

    dW[co][ci][ky][kx] = sum_{n, yo, xo} dY[n][co][yo][xo] * X'[n][ci][stride yo + ky - k/2][stride xo + kx - k/2]      (zero padding)
    db[co]             = sum_{n, yo, xo} dY[n][co][yo][xo]                                     X' = X, or X^2 with `square`

  wgrad64       the definition in float64: one einsum per tap over the shifted slice of the zero-padded input (no autograd)
  wgrad_scale64 the same sums over |dY| |X'| (db: |dY|): the magnitude of an entry's terms, what a sum that cancels is accurate
                relative to
  wgrad_seq_f32 every entry as ONE float32 chain over all pixels in (image, row, column) order, product and addition rounded
                separately.  Every kernel form sums shorter chains (a wave's walks, a tile's images) and folds them, so this is the
                yardstick -- the role conv_seq_f32 plays in tests/_conv_refs.py
  wgrad_int     the same sums in int64 for integer-valued inputs: with |X|, |dY| <= 3 every term is at most 9 (27 squared), every
                partial sum in any order an integer below 2^24 while 27 N Ho Wo < 2^24, hence exact in float32 -- a kernel must
                return these very values

Every function takes x [N, Cin, H, W], dy [N, Cout, Ho, Wo], the kernel size (1 or 3), the stride (1 or 2) and `square`, and returns
(dW [Cout, Cin, k, k], db [Cout])."""
import numpy as np
import torch
import torch.nn.functional as F

F32 = torch.float32
F64 = torch.float64
U = 2.0 ** -24          # unit roundoff of float32


def _taps(xp, ks, stride, ho, wo):
    """The ks ks shifted slices [N, Cin, Ho, Wo] of `xp` zero-padded by ks // 2, tap (ky, kx) at index ky ks + kx."""
    pad = ks // 2
    xp = F.pad(xp, (pad, pad, pad, pad))
    return [xp[:, :, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride] for ky in range(ks) for kx in range(ks)]


def _check(x, dy, ks, stride):
    n, _, h, w = x.shape
    pad = ks // 2
    assert ks in (1, 3) and stride in (1, 2)
    assert dy.shape[0] == n and tuple(dy.shape[2:]) == ((h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1)


def _sums(xp, d, ks, stride):
    cout, cin, ho, wo = d.shape[1], xp.shape[1], d.shape[2], d.shape[3]
    dw = torch.stack([torch.einsum("nohw,nihw->oi", d, s) for s in _taps(xp, ks, stride, ho, wo)], dim=-1)
    return dw.reshape(cout, cin, ks, ks), d.sum(dim=(0, 2, 3))


def wgrad64(x, dy, ks, stride=1, square=False):
    _check(x, dy, ks, stride)
    xd = x.double()
    return _sums(xd * xd if square else xd, dy.double(), ks, stride)


def wgrad_scale64(x, dy, ks, stride=1, square=False):
    _check(x, dy, ks, stride)
    xd = x.double().abs()
    return _sums(xd * xd if square else xd, dy.double().abs(), ks, stride)


def wgrad_seq_f32(x, dy, ks, stride=1, square=False):
    """acc = fl(acc + fl(dY X')) pixel by pixel in (image, row, column) order, all (co, ci, tap) at once; db = the chain over dY."""
    _check(x, dy, ks, stride)
    assert x.dtype == F32 and dy.dtype == F32
    n, cout, ho, wo = dy.shape
    cin = x.shape[1]
    xs = torch.stack(_taps(x * x if square else x, ks, stride, ho, wo), dim=2)      # [n, cin, taps, ho, wo]
    xs = xs.permute(0, 3, 4, 1, 2).reshape(n * ho * wo, 1, cin, ks * ks).contiguous()
    d = dy.permute(0, 2, 3, 1).reshape(n * ho * wo, cout).contiguous()
    acc = torch.zeros((cout, cin, ks * ks), dtype=F32)
    db = torch.zeros((cout,), dtype=F32)
    for k in range(n * ho * wo):
        acc = acc + d[k, :, None, None] * xs[k]
        db = db + d[k]
    return acc.reshape(cout, cin, ks, ks), db


def wgrad_int(x, dy, ks, stride=1, square=False):
    """int64 sums of integer-valued inputs (any dtype that holds them exactly)."""
    _check(x, dy, ks, stride)
    assert bool((x == x.round()).all()) and bool((dy == dy.round()).all()), "integer-valued inputs only"
    xi, di = x.to(torch.int64), dy.to(torch.int64)
    if square:
        xi = xi * xi
    cout, cin, ho, wo = dy.shape[1], x.shape[1], dy.shape[2], dy.shape[3]
    dn = di.numpy()
    dw = np.stack([np.einsum("nohw,nihw->oi", dn, s.numpy()) for s in _taps(xi, ks, stride, ho, wo)], axis=-1)
    return torch.from_numpy(dw.reshape(cout, cin, ks, ks)), di.sum(dim=(0, 2, 3))


def rel_err(got, want64, scale64):
    """max |got - want| / scale; an entry whose every term is zero counts relative to the smallest normal float32."""
    assert torch.isfinite(got).all(), "non-finite result"
    return float(((got.double() - want64).abs() / scale64.clamp_min(2.0 ** -126)).max())


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def out_hw(h, w, ks, stride):
    pad = ks // 2
    return (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1


def int_inputs(n, cin, h, w, cout, ks, stride, seed):
    """x, dy: integers drawn from [-3, 3], stored as float32."""
    g = torch.Generator().manual_seed(seed)
    ho, wo = out_hw(h, w, ks, stride)
    return (torch.randint(-3, 4, (n, cin, h, w), generator=g).to(F32), torch.randint(-3, 4, (n, cout, ho, wo), generator=g).to(F32))


def uniform_inputs(n, cin, h, w, cout, ks, stride, seed):
    """x, dy: uniform float32 in [-1, 1)."""
    g = torch.Generator().manual_seed(seed)
    ho, wo = out_hw(h, w, ks, stride)
    return (torch.rand((n, cin, h, w), generator=g, dtype=F32) * 2 - 1, torch.rand((n, cout, ho, wo), generator=g, dtype=F32) * 2 - 1)
