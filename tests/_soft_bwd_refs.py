"""References for the two backward contractions of the soft assignment (mcq_vq_soft_bwd_f32: csrc/vq_train.hip, csrc/vq_bwd_mfma.hip):
what tests/test_gpu_soft_bwd_leaf.py compares a launch with (tests/test_soft_bwd_refs.py holds them to float64 autograd on the CPU).
Nothing here imports mcquic_amd: every reference is the mathematics, written with torch / numpy on the CPU.

    dx[v][j]    = 2 x[v][j] rowsum[v]   - 2 sum_c ddist[v][c] C[g][c][j]
    dC[g][c][j] = 2 C[g][c][j] colsum_c - 2 sum_v ddist[v][c] x[v][j] + sum_{v: index_v = c} hot_v dDeq[v][j]      colsum_c = sum_v ddist[v][c]

v runs over the latent vectors (image, pixel) of group g.  Every function takes the entry point's tensors in its layouts

    ddist [N, m, h, w, k]   rowsum, index (int64), hot [N, m, h, w]   x, ddeq [N, m d, h, w]   cb [m, k, d]

(rowsum is an INPUT: the softmax backward hands it over, the contraction does not re-sum ddist) and returns (dx [N, m d, h, w], dC [m, k, d]).

  soft_bwd64        the definition in float64 (einsum; the scatter by index_put with accumulation)
  soft_bwd_scale64  the same sums over the magnitudes of their terms: 2 |x| |rowsum| + 2 sum |ddist| |C| and
                    2 |C| sum_v |ddist| + 2 sum |ddist| |x| + sum |hot| |dDeq| -- what a sum that cancels is accurate relative to
  soft_bwd_seq_f32  every entry as ONE float32 fma chain: dx over all k codewords in order, dC over all vectors in (image, pixel) order
                    with the column sum as a plain float32 chain and the scatter as an fma chain beside it; the results are combined
                    as the kernels write them (products and sums rounded one by one).  Every kernel form builds shorter chains and
                    folds them (vq_dx_kernel: runs of 64; the tiled forms: four slices; the MFMA forms: 16 / 8 slices), vq_dc_kernel
                    is this very chain -- the yardstick, the role wgrad_seq_f32 plays in tests/_wgrad_refs.py
  soft_bwd_int      the same sums in int64 for integer-valued inputs: with every |value| <= 3 (so |rowsum| <= 3 k, |colsum| <= 3 N h w) no
                    partial sum in any order exceeds 36 k (dx) or 45 N h w (dC): integers below 2^24 while 45 max(k, N h w) < 2^24,
                    hence exact in float32 -- a kernel must return these very values"""
import numpy as np
import torch

F32 = torch.float32
F64 = torch.float64


def _dims(ddist, x, cb):
    n, m, h, w, k = ddist.shape
    d = cb.shape[2]
    assert tuple(cb.shape) == (m, k, d) and tuple(x.shape) == (n, m * d, h, w)
    return n, m, d, h * w, k


def _views(ddist, rowsum, x, ddeq, index, hot, n, m, d, hw, k):
    """ddist [n, m, hw, k], rowsum [n, m, hw, 1], x / ddeq [n, m, hw, d] (vector-major), index / hot [n, m, hw]."""
    def vec(t):
        return t.reshape(n, m, d, hw).permute(0, 1, 3, 2)
    return ddist.reshape(n, m, hw, k), rowsum.reshape(n, m, hw, 1), vec(x), vec(ddeq), index.reshape(n, m, hw), hot.reshape(n, m, hw)


def _back(dxv, n, m, d, hw, shape):
    """dx from vector-major [n, m, hw, d] to the latent's [N, m d, h, w]."""
    return dxv.permute(0, 1, 3, 2).reshape(shape).contiguous()


def _scatter(dc, index, rows):
    """dc[g][index[n, g, p]] += rows[n, g, p, :] over every (n, p), duplicates added up."""
    n, m, hw = index.shape
    g = torch.arange(m).reshape(1, m, 1).expand(n, m, hw)
    dc.index_put_((g.reshape(-1), index.reshape(-1)), rows.reshape(n * m * hw, -1), accumulate=True)
    return dc


def soft_bwd64(ddist, rowsum, x, cb, ddeq, index, hot):
    n, m, d, hw, k = _dims(ddist, x, cb)
    dd, rs, xv, dq, idx, hv = _views(ddist.double(), rowsum.double(), x.double(), ddeq.double(), index, hot.double(), n, m, d, hw, k)
    c = cb.double()
    dxv = 2 * xv * rs - 2 * torch.einsum("ngvc,gcj->ngvj", dd, c)
    dc = 2 * c * dd.sum(dim=(0, 2))[:, :, None] - 2 * torch.einsum("ngvc,ngvj->gcj", dd, xv)
    _scatter(dc, idx, hv[..., None] * dq)
    return _back(dxv, n, m, d, hw, x.shape), dc


def soft_bwd_scale64(ddist, rowsum, x, cb, ddeq, index, hot):
    n, m, d, hw, k = _dims(ddist, x, cb)
    dd, rs, xv, dq, idx, hv = _views(ddist.double().abs(), rowsum.double().abs(), x.double().abs(), ddeq.double().abs(), index,
                                     hot.double().abs(), n, m, d, hw, k)
    c = cb.double().abs()
    dxv = 2 * xv * rs + 2 * torch.einsum("ngvc,gcj->ngvj", dd, c)
    dc = 2 * c * dd.sum(dim=(0, 2))[:, :, None] + 2 * torch.einsum("ngvc,ngvj->gcj", dd, xv)
    _scatter(dc, idx, hv[..., None] * dq)
    return _back(dxv, n, m, d, hw, x.shape), dc


def _fma(a, b, c):
    """float32 fma(a, b, c): the product of two float32 is exact in float64, the sum is rounded once there and once to float32."""
    return (a.double() * b.double() + c.double()).to(F32)


def soft_bwd_seq_f32(ddist, rowsum, x, cb, ddeq, index, hot):
    assert all(t.dtype == F32 for t in (ddist, rowsum, x, cb, ddeq, hot))
    n, m, d, hw, k = _dims(ddist, x, cb)
    dd, rs, xv, dq, idx, hv = _views(ddist, rowsum, x, ddeq, index, hot, n, m, d, hw, k)
    acc = torch.zeros((n, m, hw, d), dtype=F32)
    for c in range(k):                                               # one chain over the codewords, every (vector, channel) at once
        acc = _fma(dd[:, :, :, c:c + 1], cb[None, :, c, None, :], acc)
    dxv = (2.0 * xv) * rs - 2.0 * acc
    acc = torch.zeros((m, k, d), dtype=F32)
    cs = torch.zeros((m, k, 1), dtype=F32)
    sc = torch.zeros((m, k, d), dtype=F32)
    g = torch.arange(m)
    for a in range(n):                                               # one chain over the vectors, every (group, codeword, channel) at once
        for p in range(hw):
            col = dd[a, :, p, :, None]
            acc = _fma(col, xv[a, :, p, None, :], acc)
            cs = cs + col
            hit = idx[a, :, p]
            sc[g, hit] = _fma(hv[a, :, p, None], dq[a, :, p], sc[g, hit])
    dc = ((2.0 * cb) * cs - 2.0 * acc) + sc
    return _back(dxv, n, m, d, hw, x.shape), dc


def soft_bwd_int(ddist, rowsum, x, cb, ddeq, index, hot):
    """int64 sums of integer-valued inputs (any dtype that holds them exactly)."""
    for t in (ddist, rowsum, x, cb, ddeq, hot):
        assert bool((t == t.round()).all()), "integer-valued inputs only"
    n, m, d, hw, k = _dims(ddist, x, cb)
    i64 = torch.int64
    dd, rs, xv, dq, idx, hv = _views(ddist.to(i64), rowsum.to(i64), x.to(i64), ddeq.to(i64), index, hot.to(i64), n, m, d, hw, k)
    c = cb.to(i64)
    dxv = 2 * xv * rs - 2 * torch.from_numpy(np.einsum("ngvc,gcj->ngvj", dd.numpy(), c.numpy()))
    dc = 2 * c * dd.sum(dim=(0, 2))[:, :, None] - 2 * torch.from_numpy(np.einsum("ngvc,ngvj->gcj", dd.numpy(), xv.numpy()))
    _scatter(dc, idx, hv[..., None] * dq)
    return _back(dxv, n, m, d, hw, x.shape), dc


def rel_err(got, want64, scale64):
    """max |got - want| / scale; an entry whose every term is zero counts relative to the smallest normal float32."""
    assert torch.isfinite(got).all(), "non-finite result"
    return float(((got.double() - want64).abs() / scale64.clamp_min(2.0 ** -126)).max())


# ---- inputs ------------------------------------------------------------------------------------------------------------------------------
def _shapes(n, m, d, h, w, k):
    return (n, m, h, w, k), (n, m * d, h, w), (m, k, d), (n, m * d, h, w), (n, m, h, w)


def int_inputs(n, m, d, h, w, k, seed):
    """(ddist, rowsum, x, cb, ddeq, hot): integers drawn from [-3, 3] as float32; rowsum the exact row sum of ddist."""
    g = torch.Generator().manual_seed(seed)
    ddist, x, cb, ddeq, hot = (torch.randint(-3, 4, s, generator=g).to(F32) for s in _shapes(n, m, d, h, w, k))
    return ddist, ddist.sum(-1), x, cb, ddeq, hot


def uniform_inputs(n, m, d, h, w, k, seed):
    """(ddist, rowsum, x, cb, ddeq, hot): uniform float32 in [-1, 1); rowsum the float32 rounding of the float64 row sum."""
    g = torch.Generator().manual_seed(seed)
    ddist, x, cb, ddeq, hot = (torch.rand(s, generator=g, dtype=F32) * 2 - 1 for s in _shapes(n, m, d, h, w, k))
    return ddist, ddist.double().sum(-1).to(F32), x, cb, ddeq, hot
