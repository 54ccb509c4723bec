"""GPU: GroupNorm (csrc/norm.hip, the `denseNorm=True` path), kernel by kernel, against float64 references written from the
definition (tests/_leaf_refs.py: group_norm64, group_norm_bwd64; tests/test_leaf_ops_reference.py ties them to
torch.nn.functional.group_norm).

The launcher has three routes: one workgroup per run (planes below 256 pixels), the chunked kernels (planes from 256 pixels on,
cut into chunks of 8192 floats) and -- with more than 65535 planes -- the one-workgroup kernels again on planes the chunked
kernels would take.  Every route runs here at the shapes where its index arithmetic can go wrong (runs of two elements, counts
that are no whole quads, unaligned runs, one / several channels per group, a plane of exactly 256, 8191, 8192, 8193 pixels, a
tail chunk of one element, 65536 planes), in every input regime of R.GN_REGIMES: the backward formulas cancel in proportion to
|mean| / sigma of a run, which a conv bias in front of a one-channel-per-group norm makes large.

Bars: for every asserted quantity, e_hip = the kernel against float64 and e_f32 = the DEFINITION (centred, not the kernel's
rearrangement) in float32 on the CPU against float64, both in the scales of R.group_norm_scales64 (a sum that cancels is measured
against the sum of its terms' magnitudes, never against itself); e_hip <= max(4 e_f32, 1.2e-7), the bar of
test_gpu_soft_assign_leaf.py.  Both figures of every case go to the run's record (tests/_record.py); the committed copy is
profiles/r09_group_norm_leaf_errors.json.

Not tested: runs beyond 2^24 elements (gn_merge_stats counts in float32, exact only below that)."""
import functools

import pytest
import torch

import _leaf_refs as R
from _record import record

pytestmark = pytest.mark.gpu

FLOOR = 1.2e-7                                   # one float32 spacing relative to the scale
EPS = 1e-5

ONE_WG = [(2, 6, 1, 1, 3), (1, 4, 3, 5, 2), (3, 8, 5, 51, 2), (2, 32, 15, 17, 32), (2, 8, 8, 8, 1)]
BOUNDARY = [(2, 4, 16, 16, 2), (2, 4, 1, 257, 2)]
CHUNKED = [(2, 4, 1, 8191, g) for g in (4, 2, 1)] + [(2, 4, 64, 128, g) for g in (4, 2, 1)] + \
          [(2, 4, 1, 8193, g) for g in (4, 2, 1)] + [(3, 2, 1, 16385, g) for g in (2, 1)]        # cg in {1, 2, C} (C = 2: {1, C})
MANY_PLANES = (1024, 64, 16, 16, 32)             # N * C = 65536 planes of 256 pixels, two channels per group
ROUTE_SHAPES = {"one_wg": (3, 8, 5, 51, 2), "chunked": (2, 4, 1, 8193, 2), "many_planes": MANY_PLANES}


def _cases():
    """(shape + groups, regime): every shape in `plain` and `bias_dominated`, every regime on one shape of each route, and the run
    that opens with its outlier on more chunked shapes (a 256-pixel plane, one channel per group, three chunks per plane)."""
    out = [(s, r) for s in ONE_WG + BOUNDARY + CHUNKED for r in ("plain", "bias_dominated")]
    out += [(s, "outlier_first") for s in ((2, 4, 16, 16, 2), (2, 4, 1, 8193, 4), (3, 2, 1, 16385, 2), (3, 2, 1, 16385, 1))]
    for s in ROUTE_SHAPES.values():
        out += [(s, r) for r in R.GN_REGIMES if (s, r) not in out]
    return out


def _id(v):
    return "x".join(str(i) for i in v) if isinstance(v, tuple) else str(v)


def _bar(key, e_hip, e_f32):
    bar = max(4.0 * e_f32, FLOOR)
    record(key, e_hip=e_hip, e_f32=e_f32, bar=bar)
    print(f"{key}: e_hip {e_hip:.3e}  e_f32 {e_f32:.3e}  bar {bar:.3e}")
    return None if e_hip <= bar else f"{key}: kernel {e_hip:.3e} > max(4 x {e_f32:.3e}, {FLOOR:.1e})"


NAMES = ("y", "silu", "mean", "rstd", "dx", "dgamma", "dbeta")


def _slices(n, elems_per_image):
    step = max(1, (1 << 21) // elems_per_image)                          # at most 2 M elements of float64 autograd at a time
    return [slice(i, min(i + step, n)) for i in range(0, n, step)]


def _errs(got, x, dy, gamma, beta, groups, eps):
    """{name: (error of `got`, error of the float32 definition)} against float64, image slice by image slice (the parameter
    gradients and their scales are sums over the batch: accumulated in float64).  `got`: name -> CPU tensor, names may be absent."""
    n, c, h, w = x.shape
    worst = {k: [0.0, 0.0] for k in NAMES}
    acc = {k: torch.zeros(c, dtype=torch.float64) for k in ("dgamma", "dbeta", "s_dgamma", "s_dbeta", "f_dgamma", "f_dbeta")}
    for sl in _slices(n, c * h * w):
        xs, ds = x[sl], dy[sl]
        y64, mean64, rstd64, silu64 = R.group_norm64(xs, gamma, beta, groups, eps)
        dx64, dg64, db64 = R.group_norm_bwd64(xs, ds, gamma, groups, eps)
        sc = R.group_norm_scales64(xs, ds, gamma, beta, groups, eps)
        yf, meanf, rstdf, siluf = R.group_norm_f32(xs, gamma, beta, groups, eps)
        dxf, dgf, dbf = R.group_norm_bwd_f32(xs, ds, gamma, groups, eps)
        want = dict(y=(y64, sc["y"], yf), silu=(silu64, sc["y"], siluf), mean=(mean64, sc["mean"], meanf), rstd=(rstd64, sc["rstd"], rstdf),
                    dx=(dx64, sc["dx"], dxf))
        for k, (w64, s64, f) in want.items():
            worst[k][1] = max(worst[k][1], R.scaled_err(f, w64, s64.expand_as(w64)))
            if k in got:
                g = got[k].reshape((n,) + tuple(w64.shape[1:]))[sl]
                worst[k][0] = max(worst[k][0], R.scaled_err(g, w64, s64.expand_as(w64)))
        for k, v in (("dgamma", dg64), ("dbeta", db64), ("s_dgamma", sc["dgamma"]), ("s_dbeta", sc["dbeta"]), ("f_dgamma", dgf), ("f_dbeta", dbf)):
            acc[k] += v.double()
    for k in ("dgamma", "dbeta"):
        worst[k][1] = R.scaled_err(acc["f_" + k].float(), acc[k], acc["s_" + k])
        if k in got:
            worst[k][0] = R.scaled_err(got[k], acc[k], acc["s_" + k])
    return {k: tuple(v) for k, v in worst.items() if k in got}


def _run(dev, x, dy, gamma, beta, groups, eps=EPS, dual_silu=True, want_stats=True, want_params=True):
    """Forward and (with statistics) backward once; name -> CPU tensor.  Inputs must come back untouched."""
    from mcquic_amd import ops
    on = lambda t: None if t is None else t.to(dev)
    xd, dyd, gd, bd = on(x), on(dy), on(gamma), on(beta)
    res = ops.group_norm(xd, gd, bd, groups, eps, dual_silu=dual_silu, want_stats=want_stats)
    y, mean, rstd = res if want_stats else (res, None, None)
    got = dict(y=y.cpu())
    if dual_silu:
        got["silu"] = ops.silu_twin(y).cpu()
    if want_stats:
        got["mean"], got["rstd"] = mean.cpu(), rstd.cpu()
        dx, dw, db = ops.group_norm_bwd(xd, dyd, gd, mean, rstd, groups, want_params=want_params)
        got["dx"] = dx.cpu()
        if want_params:
            got["dgamma"], got["dbeta"] = dw.cpu(), db.cpu()
        else:
            assert dw is None and db is None
    assert torch.equal(xd.cpu(), x) and torch.equal(dyd.cpu(), dy), "an input was written to"
    assert gamma is None or torch.equal(gd.cpu(), gamma)
    assert beta is None or torch.equal(bd.cpu(), beta)
    assert y.shape == x.shape and (not want_stats or (mean.shape == (x.shape[0] * groups,) and got["dx"].shape == x.shape))
    return got


def _hold(key, got, x, dy, gamma, beta, groups, eps=EPS):
    failures = []
    for name, (e_hip, e_f32) in _errs(got, x, dy, gamma, beta, groups, eps).items():
        failures.append(_bar(f"{key}.{name}", e_hip, e_f32))
    failures = [f for f in failures if f]
    assert not failures, "\n".join(failures)


@functools.lru_cache(maxsize=2)
def _case(sg, regime, constant_run=False):
    return R.gn_case(sg[:4], sg[4], regime, 9000 + sum(sg) + R.GN_REGIMES.index(regime), constant_run=constant_run)


@pytest.mark.parametrize("sg,regime", _cases(), ids=_id)
def test_group_norm_against_float64(dev, sg, regime):
    """y, its SiLU twin, mean, rstd, dx, dgamma and dbeta of every shape in the `plain` and `bias_dominated` regimes and of one shape
    per route in all nine, each at the bar; `outlier_first` (the 1e3 element opens a run) also on the chunked shapes with one
    channel per group and with a run of several chunks.  Measured figures: profiles/r09_group_norm_leaf_errors.json."""
    x, dy, gamma, beta = _case(sg, regime)
    _hold(f"group_norm[{_id(sg)},{regime}]", _run(dev, x, dy, gamma, beta, sg[4]), x, dy, gamma, beta, sg[4])


@pytest.mark.parametrize("route", sorted(ROUTE_SHAPES))
def test_group_norm_constant_run(dev, route):
    """The last run of the last image is 2.5 throughout: variance 0, rstd = eps^-1/2 = 316, xhat = 0, y = beta exactly and
    dx = rstd (gamma dy - mean(gamma dy)).  All outputs finite, every quantity at the bar -- y and its twin too: the forward
    stores (x - mean) scale + beta, which is beta here, where x scale + (beta - scale mean) would round at the size of 790 gamma."""
    sg = ROUTE_SHAPES[route]
    x, dy, gamma, beta = _case(sg, "plain", True)
    assert float(x.reshape(sg[0], sg[4], -1)[-1, -1].std()) == 0.0
    got = _run(dev, x, dy, gamma, beta, sg[4])
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    _hold(f"group_norm_constant_run[{route}]", got, x, dy, gamma, beta, sg[4])


@pytest.mark.parametrize("affine", ["no_gamma", "no_beta", "neither"])
@pytest.mark.parametrize("route", sorted(ROUTE_SHAPES))
def test_group_norm_without_parameters(dev, route, affine):
    """gamma=None / beta=None mean 1 / 0 (the parameter gradients are still returned)."""
    sg = ROUTE_SHAPES[route]
    x, dy, gamma, beta = _case(sg, "biased")
    gamma, beta = (None if affine != "no_beta" else gamma), (None if affine != "no_gamma" else beta)
    _hold(f"group_norm_{affine}[{route}]", _run(dev, x, dy, gamma, beta, sg[4]), x, dy, gamma, beta, sg[4])


@pytest.mark.parametrize("eps", [1e-3, 0.0])
@pytest.mark.parametrize("route", sorted(ROUTE_SHAPES))
def test_group_norm_eps(dev, route, eps):
    """eps = 1e-3 and 0 (1e-5 is every other test's) on the `quiet` regime, whose variance 1e-6 lies below both non-zero values:
    eps decides the result there.  No run is constant."""
    sg = ROUTE_SHAPES[route]
    x, dy, gamma, beta = _case(sg, "quiet")
    _hold(f"group_norm_eps{eps:g}[{route}]", _run(dev, x, dy, gamma, beta, sg[4], eps=eps), x, dy, gamma, beta, sg[4], eps=eps)


@pytest.mark.parametrize("route", sorted(ROUTE_SHAPES))
def test_group_norm_options_and_determinism(dev, route):
    """Without the twin and without statistics y keeps its bits and no twin is attached; with the twin but without statistics
    (a twin pointer next to null statistics pointers) y and the twin keep theirs; without parameter gradients dx keeps its bits
    and none is returned; a repeated call gives the same bits, forward and backward."""
    from mcquic_amd import ops
    sg = ROUTE_SHAPES[route]
    x, dy, gamma, beta = _case(sg, "biased")
    full = _run(dev, x, dy, gamma, beta, sg[4])
    again = _run(dev, x, dy, gamma, beta, sg[4])
    assert sorted(full) == sorted(NAMES)
    for k in NAMES:
        assert torch.equal(full[k], again[k]), f"{k}: a second call gave other bits"
    bare = _run(dev, x, dy, gamma, beta, sg[4], dual_silu=False, want_stats=False)
    assert sorted(bare) == ["y"] and torch.equal(bare["y"], full["y"])
    twin_only = _run(dev, x, dy, gamma, beta, sg[4], dual_silu=True, want_stats=False)
    assert sorted(twin_only) == ["silu", "y"] and torch.equal(twin_only["y"], full["y"]) and torch.equal(twin_only["silu"], full["silu"])
    y = ops.group_norm(x.to(dev), gamma.to(dev), beta.to(dev), sg[4], EPS)
    assert ops.silu_twin(y) is None
    no_params = _run(dev, x, dy, gamma, beta, sg[4], dual_silu=False, want_params=False)
    assert "dgamma" not in no_params and "dbeta" not in no_params
    for k in ("y", "mean", "rstd", "dx"):
        assert torch.equal(no_params[k], full[k]), f"{k} changed with the options"
