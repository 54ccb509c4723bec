"""mcquic_amd.monitor.ParamStats (csrc/param_stats.hip) on a hand-made list of float32 tensors whose sizes sit at every seam of the
256-lane workgroup and the 4096-element chunk, against the float64 reference of tests/_param_stats_ref.py.

Bars: grad_absmax, grad_nonfinite, steps, count and the blame words are exact.  The three norms are within ONE float32 ulp of the
float64 reference, which is derived and not measured: the kernels form every product and difference in double and sum in double, so
another summation order moves a sum by ~1e-16 relative (n * 2^-53 at worst, n <= 8193: 1e-12); the square root is taken in double and
rounded to float32 ONCE, so it can differ from the reference's rounding only where the double lies at a float32 rounding boundary.
The values are seeded normals scaled per tensor over 1e-20 .. 1e+15: float32 squares of the first flush, the last ones lose the sum."""
import numpy as np
import pytest
import torch

import _param_stats_ref as R

pytestmark = pytest.mark.gpu
SIZES = [0, 1, 255, 256, 257, 4095, 4096, 4097, 8193]        # the last: three chunks, a ragged end
SCALES = [1.0] + np.logspace(-20, 15, len(SIZES) - 1).tolist()
NAN, INF = float("nan"), float("inf")
EXACT = ("grad_absmax", "grad_nonfinite")
NORMS = ("weight_norm", "grad_norm", "update_norm")


def _tensors(dev, seed=5, flat_grads=False):
    """Parameters with gradients.  `flat_grads`: the gradients are dense views of ONE buffer, as a training step binds them -- 4-byte
    aligned only (offsets 0, 0, 1, 256, 512, 769, ...: some chunks take the 16-byte path, some the dword loop); else every tensor has
    its own allocation (all 16-byte paths, with the ragged tails)."""
    gen = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter((torch.randn(n, generator=gen) * s).to(dev)) for n, s in zip(SIZES, SCALES)]
    grads = [(torch.randn(n, generator=gen) * s) for n, s in zip(SIZES, SCALES)]
    if flat_grads:
        flat, off = torch.cat(grads).to(dev), 0
        for p, n in zip(params, SIZES):
            p.grad = flat[off: off + n]
            off += n
    else:
        for p, g in zip(params, grads):
            p.grad = g.to(dev)
    return params


def _host(ts):
    return [t.detach().cpu().numpy().copy() for t in ts]


def _move(params, gen, factor=1e-3):
    """What an optimizer would do between before() and after(): every weight moves, by about `factor` of its scale."""
    with torch.no_grad():
        for p, s in zip(params, SCALES):
            p.add_((torch.randn(p.numel(), generator=gen) * (s * factor)).to(p.device))


def _one_step(stats, rec, params, gen, skip=None, flag=False):
    """before, move, after on the device and on the reference; (recorded, sampled)."""
    w0 = _host(params)
    stats.before()
    _move(params, gen)
    stats.after(skip=skip)
    return rec.after(_host(params), _host([p.grad for p in params]), w0, skip=flag)


def _compare(got, want):
    assert got["steps"].tolist() == want["steps"].tolist() and got["dropped"] == want["dropped"] and got["count"] == want["count"]
    assert (got["first_bad_step"], got["first_bad_tensor"]) == (want["first_bad_step"], want["first_bad_tensor"])
    for name in EXACT:
        assert np.array_equal(got[name].astype(np.float64), want[name]), name
    for name in NORMS:
        ok = R.within_one_ulp(got[name], want[name])
        assert ok.all(), (name, got[name][~ok], want[name][~ok])
    assert all(got[name].dtype == np.float32 and got[name].shape == (len(got["steps"]), len(SIZES)) for name in R.COLUMNS)
    with np.errstate(divide="ignore", invalid="ignore"):
        assert np.array_equal(got["update_ratio"], got["update_norm"] / got["weight_norm"], equal_nan=True)


def _blame_run(dev):
    """Three steps: a clean one; one with NaN as the first element of a chunk, +inf as the last element of a chunk and -inf as the last
    element of the ragged tail (tensor 8) beside an all-NaN tensor 2; one with an inf in tensor 1 alone."""
    from mcquic_amd import monitor
    params = _tensors(dev, flat_grads=True)
    stats, rec, gen = monitor.ParamStats(params, capacity=4), R.Recorder(len(SIZES), 4, 1), torch.Generator().manual_seed(6)
    assert stats.blame() is None
    _one_step(stats, rec, params, gen)
    clean = [p.grad.clone() for p in params]
    params[8].grad[4096], params[8].grad[4095], params[8].grad[8192] = NAN, INF, -INF
    params[2].grad.fill_(NAN)
    _one_step(stats, rec, params, gen)
    assert stats.blame() == (1, "2")
    for p, g in zip(params, clean):
        p.grad.copy_(g)
    params[1].grad[0] = -INF
    _one_step(stats, rec, params, gen)
    return stats, rec


def test_every_column_at_every_seam_and_the_blame_words(dev):
    stats, rec = _blame_run(dev)
    assert stats.blame() == (1, "2"), "the lower index of two tensors, kept when a later step has a lower one"
    got, want = stats.read(), rec.read()
    _compare(got, want)
    assert got["names"] == [str(i) for i in range(len(SIZES))] and got["steps"].tolist() == [0, 1, 2]
    assert got["grad_nonfinite"][1].tolist() == [0, 0, 255, 0, 0, 0, 0, 0, 3] and got["grad_nonfinite"][2].tolist() == [0, 1, 0, 0, 0, 0, 0, 0, 0]
    assert got["grad_norm"][1, 2] == 0 and got["grad_absmax"][1, 2] == 0 and got["grad_norm"][1, 8] > 0
    assert not np.any(got["weight_norm"][:, 0]) and not np.any(got["update_norm"][:, 0]), "a tensor without elements: zeros"
    assert np.all(got["update_norm"][:, 1:] > 0) and np.all(np.isfinite(got["weight_norm"]))
    assert stats.read()["steps"].tolist() == []


def test_two_runs_give_identical_bits(dev):
    a, _ = _blame_run(dev)
    b, _ = _blame_run(dev)
    assert torch.equal(a._buf, b._buf) and torch.equal(a._shadow, b._shadow)


def test_sampling_skip_and_ring_wrap(dev):
    """every=2, capacity=3, seven calls, the flag set on the unsampled call at count 3: rows at 0, 2, 3, 4, 6, the last three kept."""
    from mcquic_amd import monitor
    params = _tensors(dev, seed=7)
    stats, rec, gen = monitor.ParamStats(params, capacity=3, every=2), R.Recorder(len(SIZES), 3, 2), torch.Generator().manual_seed(8)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    for c in range(7):
        flag.fill_(int(c == 3))
        shadow, ring = stats._shadow.clone() if c else None, stats._buf.clone()
        recorded, sampled = _one_step(stats, rec, params, gen, skip=flag, flag=c == 3)
        assert (recorded, sampled) == (c % 2 == 0 or c == 3, c % 2 == 0)
        if not sampled:
            assert torch.equal(stats._shadow, shadow), f"call {c} is not sampled: the shadow stays"
        else:
            assert shadow is None or not torch.equal(stats._shadow, shadow)
        if not recorded:
            ring[0] += 1
            assert torch.equal(stats._buf, ring), f"call {c} is not recorded: only count moves"
    got, want = stats.read(), rec.read()
    _compare(got, want)
    assert got["steps"].tolist() == [3, 4, 6] and got["dropped"] == 2 and got["count"] == 7
    assert not np.any(got["update_norm"][0]), "the forced row does not read the (stale) shadow"
    assert np.all(got["update_norm"][1:, 1:] > 0)
    assert stats.blame() is None


def test_without_updates_there_is_no_shadow(dev):
    from mcquic_amd import monitor
    params = _tensors(dev, seed=9)
    stats, rec, gen = monitor.ParamStats(params, capacity=2, updates=False), R.Recorder(len(SIZES), 2, 1, updates=False), torch.Generator().manual_seed(10)
    for _ in range(2):
        _one_step(stats, rec, params, gen)
    assert stats._shadow is None
    got = stats.read()
    _compare(got, rec.read())
    assert np.isnan(got["update_norm"]).all() and got["update_norm"].shape == (2, len(SIZES))


def test_warm_and_checkpoint_keep_every_bit(dev):
    from mcquic_amd import monitor
    stats, _ = _blame_run(dev)
    buf, shadow = stats._buf.clone(), stats._shadow.clone()
    with torch.no_grad():
        stats.params[4].add_(1.0)                             # (a warm pass over OTHER weights than the shadow holds)
    stats.warm()
    assert torch.equal(stats._buf, buf) and torch.equal(stats._shadow, shadow)
    other = monitor.ParamStats(_tensors(dev), capacity=4)
    other.prepare()
    other.load_state_dict(stats.state_dict())
    assert torch.equal(other._buf, buf) and other.blame() == (1, "2")
    _compare(other.read(), stats.read())


def test_refusals(dev):
    from mcquic_amd import monitor
    good = torch.zeros(4, device=dev)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        monitor.ParamStats([good, torch.zeros(4)])
    with pytest.raises(TypeError, match="must be torch.float32"):
        monitor.ParamStats([good, torch.zeros(4, device=dev, dtype=torch.float64)])
    with pytest.raises(ValueError, match="capacity >= 1 and every >= 1"):
        monitor.ParamStats([good], capacity=0)
    with pytest.raises(ValueError, match="capacity >= 1 and every >= 1"):
        monitor.ParamStats([good], every=0)
    with pytest.raises(ValueError, match="nothing to watch"):
        monitor.ParamStats([torch.zeros(0, device=dev)])
    stats = monitor.ParamStats([good])
    with pytest.raises(TypeError, match="`skip` must be one int32"):
        stats.after(skip=torch.zeros(1, device=dev))
