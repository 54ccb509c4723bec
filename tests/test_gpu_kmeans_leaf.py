"""GPU: the k-means kernels (csrc/vq_kmeans.hip) against the float64 restatement tests/_kmeans_ref.py.

Bounds (none taken from what the kernels give):
  counts, empty   exact.
  sums            V 2^-52 sum |x_v[j]| per entry: the reordering bound of a double sum of V exact float32 terms.
  sqsums          (V + d) 2^-52 sum |x_v|^2.
  codewords       1 float32 ulp of float32(ref_sum / count) (the ulp covers the one double-rounding boundary); unused ones bit-unchanged.
  inertia         1e-12 sum_v (|x_v|^2 + |c_old|^2) per group: fewer than V + 3 d + 3 double operations on terms bounded by that sum.
  seed            bit for bit the vectors picked from mcq_hash_uniform_f32's draws.
V = 30 has fewer vectors than codes and less than a wave; V = 264 crosses the 64-entry chunks (and the 256-entry step) with a
ragged tail."""
import functools

import numpy as np
import pytest
import torch

import _kmeans_ref as R

pytestmark = pytest.mark.gpu

SHAPES = [(1, 8, 192), (2, 4, 8), (2, 16, 64), (3, 64, 128)]
MAPS = [(2, 3, 5), (3, 8, 11)]
# + one case past the grid: d = 80 (a second pass over the channels) and V = 800 with few codewords (four waves per codeword)
CASES = [s + g for s in SHAPES for g in MAPS] + [(1, 80, 5, 5, 8, 20)]
OUTLIERS = (2, 16, 64, 3, 8, 11)                 # the case that carries one -1 and one k among its codes
EPS = 2.0 ** -52


def _bits(t):
    return t.view({torch.float64: torch.int64, torch.float32: torch.int32}.get(t.dtype, t.dtype))


def _batch(gen, m, d, k, N, h, w, used):
    x = torch.randn((N, m * d, h, w), generator=gen, dtype=torch.float32)
    codes = used[torch.randint(0, len(used), (N, m, h, w), generator=gen)]
    return x, codes


@functools.lru_cache(maxsize=None)
def _case(m, d, k, N, h, w):
    """Inputs and the reference's results for one case, computed once: two batches, a codebook, the reference after batch 1
    (accumulators, update) and after both batches (accumulators)."""
    gen = torch.Generator().manual_seed(1000 * k + 10 * d + N)
    used = torch.randperm(k, generator=gen)[: max(1, (3 * k) // 4)]         # about a quarter of the codewords never used
    x1, c1 = _batch(gen, m, d, k, N, h, w, used)
    x2, c2 = _batch(gen, m, d, k, N, h, w, used)
    if (m, d, k, N, h, w) == OUTLIERS:
        c1[1, 0, 2, 3] = -1
        c1[2, 1, 7, 10] = k
    cb = torch.randn((m, k, d), generator=gen, dtype=torch.float32)
    acc1 = R.accumulate(x1.numpy(), c1.numpy(), R.new_acc(m, k, d))
    acc12 = R.accumulate(x2.numpy(), c2.numpy(), tuple(a.copy() for a in acc1))
    return dict(x1=x1, c1=c1, x2=x2, c2=c2, cb=cb, acc1=acc1, acc12=acc12, upd1=R.update(cb.numpy(), acc1))


def _abs_sums(xs, cs, m, k):
    """Per codeword: sum |x_v[j]| [m, k, d], sum |x_v|^2 [m, k], over the vectors the reference counts."""
    d = xs[0].shape[1] // m
    a, s = np.zeros((m, k, d)), np.zeros((m, k))
    for x, c in zip(xs, cs):
        xv, cv = R.vectors(x.numpy(), m), R.code_rows(c.numpy())
        for g in range(m):
            ok = (cv[g] >= 0) & (cv[g] < k)
            np.add.at(a[g], cv[g][ok], np.abs(xv[g][ok]))
            np.add.at(s[g], cv[g][ok], (xv[g][ok] ** 2).sum(-1))
    return a, s


def _check_acc(acc, ref, xs, cs, m, k, d):
    V = sum(x.shape[0] * x.shape[2] * x.shape[3] for x in xs)
    a, s = _abs_sums(xs, cs, m, k)
    assert np.array_equal(acc.counts.cpu().numpy(), ref[2])
    err = np.abs(acc.sums.cpu().numpy() - ref[0])
    print("sums: worst error / bound", float((err / np.maximum(V * EPS * a, 1e-300)).max()))
    assert (err <= V * EPS * a).all()
    qerr = np.abs(acc.sqsums.cpu().numpy() - ref[1])
    print("sqsums: worst error / bound", float((qerr / np.maximum((V + d) * EPS * s, 1e-300)).max()))
    assert (qerr <= (V + d) * EPS * s).all()


@pytest.mark.parametrize("m,d,k,N,h,w", CASES)
def test_accumulate_and_update(dev, m, d, k, N, h, w):
    from mcquic_amd import ops
    c = _case(m, d, k, N, h, w)
    acc = ops.KMeansAcc(m, k, d, dev)
    ops.vq_kmeans_accumulate(c["x1"].to(dev), c["c1"].to(dev), acc)
    _check_acc(acc, c["acc1"], [c["x1"]], [c["c1"]], m, k, d)
    cb = c["cb"].to(dev)
    inertia, empty = ops.vq_kmeans_update(cb, acc)
    new, ref_inertia, ref_empty = c["upd1"]
    got, counts = cb.cpu().numpy(), c["acc1"][2]
    used = counts > 0
    assert used.any() and (~used).any()
    ulp = np.maximum(np.spacing(np.abs(new)), np.spacing(np.abs(got)))
    assert (np.abs(got.astype(np.float64) - new.astype(np.float64))[used] <= ulp[used]).all()
    assert np.array_equal(got[~used].view(np.int32), c["cb"].numpy()[~used].view(np.int32))
    assert np.array_equal(empty.cpu().numpy(), ref_empty)
    # sum over the counted vectors of |x_v|^2 + |c_old(code_v)|^2, per group
    scale = c["acc1"][1].sum(-1) + (counts * (c["cb"].numpy().astype(np.float64) ** 2).sum(-1)).sum(-1)
    ierr = np.abs(inertia.cpu().numpy() - ref_inertia)
    print("inertia: worst error / bound", float((ierr / (1e-12 * scale)).max()))
    assert (ierr <= 1e-12 * scale).all()


@pytest.mark.parametrize("m,d,k,N,h,w", CASES)
def test_second_batch_adds_onto_the_first(dev, m, d, k, N, h, w):
    from mcquic_amd import ops
    c = _case(m, d, k, N, h, w)
    acc = ops.KMeansAcc(m, k, d, dev)
    ops.vq_kmeans_accumulate(c["x1"].to(dev), c["c1"].to(dev), acc)
    ops.vq_kmeans_accumulate(c["x2"].to(dev), c["c2"].to(dev), acc)
    _check_acc(acc, c["acc12"], [c["x1"], c["x2"]], [c["c1"], c["c2"]], m, k, d)
    acc.zero_()
    assert not acc.sums.any() and not acc.sqsums.any() and not acc.counts.any()


@pytest.mark.parametrize("m,d,k,N,h,w", CASES)
def test_two_runs_are_bit_identical(dev, m, d, k, N, h, w):
    from mcquic_amd import ops
    c = _case(m, d, k, N, h, w)
    runs = []
    for _ in range(2):
        acc = ops.KMeansAcc(m, k, d, dev)
        ops.vq_kmeans_accumulate(c["x1"].to(dev), c["c1"].to(dev), acc)
        ops.vq_kmeans_accumulate(c["x2"].to(dev), c["c2"].to(dev), acc)
        cb = c["cb"].to(dev)
        inertia, empty = ops.vq_kmeans_update(cb, acc)
        runs.append([acc.sums, acc.sqsums, acc.counts, cb, inertia, empty])
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("m,d,k,N,h,w", CASES)
def test_seed_picks_the_generators_vectors(dev, m, d, k, N, h, w):
    from mcquic_amd import ops
    c = _case(m, d, k, N, h, w)
    rng = torch.tensor([1234 + k, 3], dtype=torch.int64, device=dev)
    u = ops.hash_uniform(rng, 2, (m, k)).cpu().numpy()
    x = c["x1"].to(dev)
    cb = c["cb"].to(dev)
    ops.vq_kmeans_seed(x, cb, rng)
    assert np.array_equal(cb.cpu().numpy().view(np.int32), R.seed(c["x1"].numpy(), c["cb"].numpy(), u).view(np.int32))
    counts = c["acc1"][2]                                    # zeros at the codewords batch 1 never used
    cb = c["cb"].to(dev)
    ops.vq_kmeans_seed(x, cb, rng, torch.from_numpy(counts).to(dev))
    want = R.seed(c["x1"].numpy(), c["cb"].numpy(), u, counts)
    assert np.array_equal(cb.cpu().numpy().view(np.int32), want.view(np.int32))
    assert np.array_equal(want[counts > 0].view(np.int32), c["cb"].numpy()[counts > 0].view(np.int32))


def test_cpu_tensors_are_rejected(dev):
    from mcquic_amd import ops
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.KMeansAcc(1, 2, 2, "cpu")
    acc = ops.KMeansAcc(1, 2, 2, dev)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.vq_kmeans_accumulate(torch.zeros(1, 2, 1, 1), torch.zeros(1, 1, 1, 1, dtype=torch.int64, device=dev), acc)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.vq_kmeans_update(torch.zeros(1, 2, 2), acc)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.vq_kmeans_seed(torch.zeros(1, 2, 1, 1), torch.zeros(1, 2, 2, device=dev), torch.zeros(2, dtype=torch.int64, device=dev))
