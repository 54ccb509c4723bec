"""The device CDF tables (csrc/vq_cdf.hip: mcq_pmf_to_quantized_cdf_dev) against the library's host function `pmfToQuantizedCDF`, row for
row and bit for bit: these tables must decode streams written with the host's.  The rows are those of tests/_cdf_ref.py (pinned to the
host function without a GPU by tests/test_cdf_ref.py): k = 2, k = 3 with a zero, k = 65 and 1000 (no multiple of the wave), all mass on
one symbol, ties among donors, both range directions in one row, a donor used up by an earlier steal, k = 8192 with more than half the
symbols at zero, exact .5 products.  The host's fourth error, no donor left, cannot arise at k <= 8192 (`_cdf_ref.bad_cases`)."""
import functools

import numpy as np
import pytest
import torch

import _cdf_ref as C

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _host(name):
    from mcquic_amd.modules.entropyCoder import pmfToQuantizedCDF
    return np.asarray(pmfToQuantizedCDF(C.cases()[name], 16), dtype=np.uint32)


def _levels(names):
    """The named rows grouped by length: one [m, k] level per k, the largest k first."""
    rows = C.cases()
    by_k = {}
    for nm in names:
        by_k.setdefault(len(rows[nm]), []).append(nm)
    ks = sorted(by_k, reverse=True)
    return [by_k[k] for k in ks], [np.stack([rows[nm] for nm in by_k[k]]) for k in ks]


def _check(tables, status, groups):
    st = status.cpu().numpy()
    assert st.dtype == np.int32 and st.shape == (sum(len(g) for g in groups),)
    row = 0
    for table, names in zip(tables, groups):
        assert table.dtype == torch.uint32 and table.is_cuda
        got = table.cpu().numpy()
        for g, nm in enumerate(names):
            want = _host(nm)
            assert st[row] == 0, (nm, st[row])
            assert got[g].shape == want.shape and np.array_equal(got[g], want), (nm, np.flatnonzero(got[g] != want)[:8])
            row += 1


def test_every_case_in_one_launch_equals_the_host_function(dev):
    """All rows of `_cdf_ref.cases()`: a level per row length (eleven levels of different k, m from 1 to 3) in ONE launch."""
    from mcquic_amd import ops
    groups, levels = _levels(sorted(C.cases()))
    assert len(levels) >= 3 and {len(g) for g in groups} >= {1, 3}
    tables, status = ops.pmf_to_quantized_cdf_dev([torch.from_numpy(a).to(dev) for a in levels])
    _check(tables, status, groups)


@pytest.mark.parametrize("names", [("k65",), ("k65", "k65_dead", "k65"), ("k8192_more_than_half_zero", "k8192_uniform", "k8192_plain"),
                                   ("k2", "k2_one_empty"), ("k3_one_zero",), ("k1000_dead", "k1000")])
def test_one_level_alone(dev, names):
    """m = 1, 2 and 3 at one k: the rows of a level do not see each other."""
    from mcquic_amd import ops
    groups, levels = [list(names)], [np.stack([C.cases()[nm] for nm in names])]
    tables, status = ops.pmf_to_quantized_cdf_dev([torch.from_numpy(levels[0]).to(dev)])
    _check(tables, status, groups)


def test_three_levels_of_the_coder_shape(dev):
    """m = 2, k = [8192, 2048, 512] (the qp = 2 shape): frequency rows as a trained model leaves them, half of level 0 dead."""
    from mcquic_amd import ops
    from mcquic_amd.modules.entropyCoder import pmfToQuantizedCDF
    g = np.random.default_rng(5)
    levels = []
    for k in (8192, 2048, 512):
        f = g.random((2, k)) ** 6 + 1e-9
        f[0, g.random(k) < 0.5] = 0.0
        levels.append((f / f.sum(-1, keepdims=True)).astype(np.float32))
    tables, status = ops.pmf_to_quantized_cdf_dev([torch.from_numpy(a).to(dev) for a in levels])
    assert not status.cpu().numpy().any()
    for a, t in zip(levels, tables):
        for row, got in zip(a, t.cpu().numpy()):
            assert np.array_equal(got, np.asarray(pmfToQuantizedCDF(row, 16), np.uint32))


def test_status_words_beside_valid_rows(dev):
    """A NaN row, an infinite one, a negative one and an all-zero one between valid rows: their status words say so, and the valid rows'
    tables are right.  Nothing is read by the host inside the call; the caller's buffers are written in place."""
    from mcquic_amd import ops
    bad = C.bad_cases(65)
    order = ["k65", "nan", "k65_dead", "negative", "all_zero", "inf", "k65"]
    rows = C.cases()
    level = np.stack([rows[nm] if nm in rows else bad[nm][0] for nm in order])
    other = np.stack([rows["k1000"], rows["k1000_dead"]])
    out = [torch.full((len(order), 66), 7, dtype=torch.int32, device=dev).view(torch.uint32), torch.empty((2, 1001), dtype=torch.uint32, device=dev)]
    status = torch.full((len(order) + 2,), -1, dtype=torch.int32, device=dev)
    tables, st = ops.pmf_to_quantized_cdf_dev([torch.from_numpy(level).to(dev), torch.from_numpy(other).to(dev)], out=out, status=status)
    assert tables[0] is out[0] and tables[1] is out[1] and st is status
    want = [0 if nm in rows else bad[nm][1] for nm in order] + [0, 0]
    assert st.cpu().tolist() == want
    assert want.count(0) == 5 and set(want) == {C.OK, C.BAD_ELEMENT, C.ZERO_TOTAL}
    got = tables[0].cpu().numpy()
    for g, nm in enumerate(order):
        if nm in rows:
            assert np.array_equal(got[g], _host(nm)), nm
    assert np.array_equal(tables[1].cpu().numpy(), np.stack([_host("k1000"), _host("k1000_dead")]))
    for nm, (row, code) in bad.items():
        assert C.quantized_cdf(row)[1] == code


def test_normalize_against_the_numpy_rule(dev):
    """normalize=True: raw frequency rows (an EMA's: they do not sum to one) divided by the row sum in double, rounded once to float32;
    the tables are the host function's for those quotients."""
    from mcquic_amd import ops
    from mcquic_amd.modules.entropyCoder import pmfToQuantizedCDF
    g = np.random.default_rng(9)
    raws = []
    for k, m in ((8192, 2), (1000, 3), (65, 1), (2, 2)):
        f = (g.random((m, k)) ** 5 * g.uniform(0.3, 40.0, (m, 1))).astype(np.float32)
        f[0, g.random(k) < 0.4] = 0.0
        f[0, 0] = 0.25
        raws.append(f)
    tables, status = ops.pmf_to_quantized_cdf_dev([torch.from_numpy(a).to(dev) for a in raws], normalize=True)
    assert not status.cpu().numpy().any()
    for raw, t in zip(raws, tables):
        p = C.normalise(raw)
        for row, got in zip(p, t.cpu().numpy()):
            assert np.array_equal(got, np.asarray(pmfToQuantizedCDF(row, 16), np.uint32))
    zero = torch.zeros((1, 8), device=dev)
    assert ops.pmf_to_quantized_cdf_dev([zero], normalize=True)[1].item() == ops.CDF_ZERO_TOTAL     # (tested before the division)
    mixed = torch.zeros((3, 65), device=dev)
    mixed[0] = torch.from_numpy(raws[2][0]).to(dev)
    mixed[2] = mixed[0] * 3.0
    tables, status = ops.pmf_to_quantized_cdf_dev([mixed], normalize=True)
    assert status.cpu().tolist() == [0, ops.CDF_ZERO_TOTAL, 0]
    want = np.asarray(pmfToQuantizedCDF(C.normalise(raws[2])[0], 16), np.uint32)
    assert np.array_equal(tables[0].cpu().numpy()[0], want)


def test_limits_are_python_errors(dev):
    from mcquic_amd import ops
    kmax = ops.cdf_max_k()
    assert kmax == 8192
    with pytest.raises(ValueError):
        ops.pmf_to_quantized_cdf_dev([torch.ones((1, kmax + 1), device=dev)])
    with pytest.raises(RuntimeError):
        ops.pmf_to_quantized_cdf_dev([torch.ones((1, 8))])                              # (no CPU path)
    with pytest.raises(ValueError):
        ops.pmf_to_quantized_cdf_dev([torch.ones((1, 8), device=dev)], status=torch.zeros(2, dtype=torch.int32, device=dev))


def test_coder_tables_equal_cdfs_and_follow_their_staleness(dev):
    """EntropyCoder.deviceCDFs() equals `CDFs` entry for entry, is cached, and is rebuilt when `CDFs` would be: after an EMA update and
    after a write to `_freqEMA`.  VariousMCoder: per-level m."""
    from mcquic_amd.modules import entropyCoder as E
    coder = E.EntropyCoder(2, [512, 64, 16]).to(dev)
    g = torch.Generator().manual_seed(3)

    def same(c):
        tables = c.deviceCDFs()                                                        # (device first; the other order: the test below)
        for want, got in zip(c.CDFs, tables):
            assert got.dtype == torch.uint32 and got.cpu().numpy().tolist() == want
        assert not c.deviceCDFStatus().cpu().numpy().any()
    same(coder)
    first = coder.deviceCDFs()
    assert all(a is b for a, b in zip(first, coder.deviceCDFs()))                      # cached
    with torch.no_grad():
        for f in coder._freqEMA:
            f.copy_((torch.rand(f.shape, generator=g) ** 4 + 1e-6).to(dev))
    same(coder)                                                                        # (a write to `_freqEMA`: stale, device side asked first)
    coder([torch.randint(0, k, (2, 2, 4, 4), generator=g).to(dev) for k in (512, 64, 16)])
    coder.deviceCDFs()
    same(coder)                                                                        # (an EMA update)
    various = E.VariousMCoder([1, 3, 2], [512, 64, 16]).to(dev)
    with torch.no_grad():
        for f in various._freqEMA:
            f.copy_((torch.rand(f.shape, generator=g) ** 4 + 1e-6).to(dev))
    various.resetFreqAndCDF()
    same(various)
    assert [tuple(t.shape) for t in various.deviceCDFs()] == [(1, 513), (3, 65), (2, 17)]


def test_device_tables_see_a_write_the_host_tables_saw_first(dev):
    """The order host first, then device: a write to `_freqEMA` without `resetFreqAndCDF`, then `CDFs` (which consumes the coder's
    staleness key), then `deviceCDFs()` -- the device tables keep the stamp they were built under and must still be rebuilt.  The same
    through `NormalizedFreq` and `compress`, for both `normalize` settings, and the other way round."""
    from mcquic_amd.modules import entropyCoder as E
    ks = [512, 64, 16]
    coder = E.EntropyCoder(2, ks).to(dev)
    g = torch.Generator().manual_seed(11)

    def write():
        with torch.no_grad():
            for f in coder._freqEMA:
                f.copy_((torch.rand(f.shape, generator=g) ** 4 + 1e-6).to(dev))

    def device_equals_host(host):
        for want, got in zip(host, coder.deviceCDFs()):
            assert got.cpu().numpy().tolist() == want
        for f, got in zip(coder._freqEMA, coder.deviceCDFs(normalize=True)):
            raw = f.detach().cpu().numpy()
            for row, table in zip(C.normalise(raw), got.cpu().numpy()):
                assert np.array_equal(table, C.quantized_cdf(row)[0])
    write()
    coder.deviceCDFs(), coder.deviceCDFs(normalize=True)               # cached under the first contents
    old = [t.clone() for t in coder.deviceCDFs()]
    write()
    host = coder.CDFs                                                  # the host side sees the write first
    device_equals_host(host)
    assert any(not np.array_equal(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(old, coder.deviceCDFs()))
    write()
    coder.NormalizedFreq
    device_equals_host(coder.CDFs)
    write()
    codes = [torch.randint(0, k, (1, 2, 4, 4), generator=g).to(dev) for k in ks]
    binaries, _ = coder.compress(codes)
    device_equals_host(coder.CDFs)
    write()
    tables = [t.clone() for t in coder.deviceCDFs()]                   # the device side first: the host tables must follow as well
    assert [t.cpu().numpy().tolist() for t in tables] == [c for c in coder.CDFs]
