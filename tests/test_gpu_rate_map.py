"""Rate control per image and per region on the device: lambda as an operand of the assignment kernel (mcq_vq_assign_rate_map_f32), the
bits section and the level maps (csrc/vq_rate_map.hip) against the references of tests/_rate_map_ref.py, then `rd_map` and the
per-image target-rate search of `Compressor` on the smallest model of tests/test_gpu_rate_encode.py at 2 x 128 x 128.

Bars.  lambda = 0 anywhere: `ops.vq_assign`'s code, bit for bit.  Bits section: within ONE float32 ulp of fl32(16 - log2 width) evaluated
with float64's log2 (the device's log2 may differ in its last place before the one rounding), powers of two exact.  Assignment: the
float64 argmin, a differing position excused only inside (d + 4) 2^-23 (|x|^2 + |c|^2 + 2 |x.c| + lambda_v bits), at most 1 % of the
positions of a (k, d) case (tests/test_rate_map_ref.py shows the float32 sequence staying under that on these seeds).  Addressing, level
maps, the search's trace: exact."""
import numpy as np
import pytest
import torch

import _rate_map_ref as MR
import _rate_ref as RR
from oracle import mcquic_ref as R

pytestmark = pytest.mark.gpu

SHAPE = (8, 2, [32, 16, 8])


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


_CASES = {}


def _case(dev, m, k, d, h, w):
    """One seeded case on the device, made once: (x, codebook, cdf as NumPy; x, plain pack, bits section, plain codes on the device)."""
    key = (str(dev), m, k, d, h, w)
    if key not in _CASES:
        from mcquic_amd import ops
        x, cb, cdf = RR.make_case(m, k, d, h, w)
        pack = ops.PackedCodebook(_t(cb, dev))
        xd = _t(x, dev)
        _CASES[key] = (x, cb, cdf, xd, pack, ops.pack_bits(_t(cdf, dev)), ops.vq_assign(xd, pack))
    return _CASES[key]


# ---- the leaf kernels -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", RR.PACK_KS)
@pytest.mark.parametrize("m", RR.PACK_MS)
def test_bits_section(dev, m, k):
    from mcquic_amd import ops
    _, _, cdf = RR.make_case(m, k, 3, 1, 1)
    cdf = cdf.copy()
    if k >= 128:                                                     # power-of-two widths among the others, and one empty slot
        w = np.diff(cdf.astype(np.int64), axis=-1)
        w[:, 3], w[:, 4], w[:, 5] = 1, 64, 0
        for gi in range(m):
            w[gi, np.argmax(w[gi])] += 65536 - w[gi].sum()
        assert (w >= 0).all() and (w.sum(-1) == 65536).all()
        cdf = np.concatenate([np.zeros((m, 1), np.int64), np.cumsum(w, -1)], -1).astype(np.uint32)
    got = ops.pack_bits(_t(cdf, dev)).cpu().numpy()
    g, word, kind = RR.norm_section_layout(m, k)
    assert got.shape == (len(kind),) and got.dtype == np.float32
    assert (got[kind != 0] == 0).all() and not np.signbit(got[kind != 0]).any()
    want = MR.bits_f32(cdf)[g[kind == 0], word[kind == 0]]
    have = got[kind == 0]
    assert np.array_equal(np.isinf(have), np.isinf(want))
    fin = np.isfinite(want)
    ulps = np.abs(have[fin].astype(np.float64) - want[fin].astype(np.float64)) / np.spacing(np.maximum(np.abs(want[fin]), np.float32(1e-30))).astype(np.float64)
    print(f"m{m} k{k}: worst {ulps.max():.2f} ulp, {int((ulps > 0).sum())} of {ulps.size} off")
    assert ulps.max() <= 1.0
    width = np.diff(cdf.astype(np.int64), axis=-1)[g[kind == 0], word[kind == 0]]
    pow2 = (width > 0) & ((width & (width - 1)) == 0)
    assert np.array_equal(have[pow2], want[pow2])
    if k >= 128:
        assert np.isinf(have[word[kind == 0] == 5]).all() and (have[word[kind == 0] == 3] == 16).all() and (have[word[kind == 0] == 4] == 10).all()


@pytest.mark.parametrize("d", RR.PACK_DS)
@pytest.mark.parametrize("k", RR.PACK_KS)
def test_zero_map_is_the_plain_assignment_and_lambdas_are_audited(dev, k, d):
    from mcquic_amd import ops
    positions = differ = 0
    for m in RR.PACK_MS:
        for (h, w) in MR.MAPS:
            x, cb, cdf, xd, pack, bits, plain = _case(dev, m, k, d, h, w)
            for zero in (torch.zeros(2, device=dev), torch.zeros((2, h, w), device=dev)):
                assert torch.equal(ops.vq_assign_rate_map(xd, pack, bits, zero), plain)
            b64 = RR.penalty_table(cdf)
            for lam in (MR.map_lambdas(2, h, w, k + d), np.asarray([0.25, 3.0], dtype=np.float32)):
                got = ops.vq_assign_rate_map(xd, pack, bits, _t(lam, dev)).cpu().numpy()
                assert got.shape == (2, m, h, w) and got.dtype == np.int64
                dn, unexcused = MR.audit(x, cb, b64, lam, got)
                assert unexcused == 0, f"m{m} {h}x{w}: {unexcused} codes differ from float64 beyond the rounding bound"
                positions += got.size
                differ += dn
                if h * w > 1:
                    assert not np.array_equal(got, plain.cpu().numpy())
    print(f"k{k} d{d}: {differ} of {positions} positions excused")
    assert differ <= RR.EXCUSED_CAP * positions


def test_the_lds_staged_instance(dev):
    from mcquic_amd import ops
    x, cb, cdf, xd, pack, bits, plain = _case(dev, 1, 512, 256, 5, 7)
    assert torch.equal(ops.vq_assign_rate_map(xd, pack, bits, torch.zeros((2, 5, 7), device=dev)), plain)
    lam = MR.map_lambdas(2, 5, 7, 99)
    got = ops.vq_assign_rate_map(xd, pack, bits, _t(lam, dev)).cpu().numpy()
    dn, unexcused = MR.audit(x, cb, RR.penalty_table(cdf), lam, got)
    print(f"k512 d256: {dn} of {got.size} positions excused")
    assert unexcused == 0 and dn <= RR.EXCUSED_CAP * got.size and not np.array_equal(got, plain.cpu().numpy())


@pytest.mark.parametrize("m, k, d, symbol", [(2, 5, 1, 3), (2, 129, 3, 128), (1, 512, 64, 200)])
def test_addressing_is_exact(dev, m, k, d, symbol):
    """A dominant symbol and a map that is 0 but for 1e30 at ONE cell: that position returns the symbol, every other the plain code."""
    from mcquic_amd import ops
    h, w = 9, 33
    x, cb, _, xd, pack, _, plain = _case(dev, m, k, d, h, w)
    bits = ops.pack_bits(_t(RR.dominant_table(m, k, symbol), dev))
    for (i, y, xx) in ((0, 0, 0), (0, 0, 32), (0, 8, 31), (1, 4, 16), (1, 8, 32)):       # corners, block seams, the last image
        lam = torch.zeros((2, h, w), device=dev)
        lam[i, y, xx] = 1e30
        want = plain.clone()
        want[i, :, y, xx] = symbol
        assert torch.equal(ops.vq_assign_rate_map(xd, pack, bits, lam), want), (i, y, xx)
        # the same map as a view of a larger tensor (strides that are not the grid's), and with explicit strides
        big = torch.full((2, h + 3, 2 * w + 5), 7e30, device=dev)
        view = big[:, 1:h + 1, 2:2 * w + 2:2]
        view.copy_(lam)
        assert not view.is_contiguous() and torch.equal(ops.vq_assign_rate_map(xd, pack, bits, view), want)
        assert torch.equal(ops.vq_assign_rate_map(xd, pack, bits, lam.flatten(), strides=(h * w, w, 1)), want)
    want = plain.clone()
    want[1] = symbol
    assert torch.equal(ops.vq_assign_rate_map(xd, pack, bits, _t(np.asarray([0.0, 1e30], dtype=np.float32), dev)), want)
    with pytest.raises(ValueError):
        ops.vq_assign_rate_map(xd, pack, bits, torch.zeros((2, h, w), device=dev).flatten(), strides=(h * w, w, 2))
    with pytest.raises(ValueError):
        ops.vq_assign_rate_map(xd, pack, bits, torch.zeros((2, h, w - 1), device=dev))


def test_an_empty_slot_never_wins(dev):
    from mcquic_amd import ops
    for (m, k, d) in ((1, 5, 3), (2, 512, 64)):
        x, cb, cdf, xd, pack, _, plain = _case(dev, m, k, d, 5, 7)
        slot = int(torch.bincount(plain[:, 0].flatten()).argmax())   # group 0's most used code loses its slot
        cdf = cdf.copy()
        cdf[0, slot + 1] = cdf[0, slot]
        bits = ops.pack_bits(_t(cdf, dev))
        for lam in (0.0, 0.5):
            got = ops.vq_assign_rate_map(xd, pack, bits, torch.full((2,), lam, device=dev))
            assert not bool((got[:, 0] == slot).any()) and bool((got >= 0).all()) and bool((got < k).all())
            if lam == 0.0:
                assert torch.equal(got[:, 0][plain[:, 0] != slot], plain[:, 0][plain[:, 0] != slot])


def test_level_maps(dev):
    from mcquic_amd import ops
    rng = np.random.default_rng(5)
    for shape, scales in (((3, 5, 7), (1.0, 0.5, 0.1)), ((2, 9, 33), (1.0, 2.0, 0.0, 0.3)), ((2, 1, 1), (1.0, 1.0)), ((3,), (1.0, 0.1, 0.7))):
        a = rng.uniform(0, 4, size=shape).astype(np.float32)
        for bad in (False, True):
            if bad:
                a.reshape(shape[0], -1)[0, -1] = np.nan
                a.reshape(shape[0], -1)[-1, 0] = -1.0
                if len(shape) == 3 and shape[1] > 1:
                    a[-1, 1, 1] = np.inf
            want, werr = MR.level_maps(a, scales)
            got, err = ops.rate_map_levels(_t(a, dev), scales)
            assert err.cpu().numpy().tolist() == werr.tolist() and bool(werr.any()) == bad
            for g, wv in zip(got, want):
                assert g.dtype == torch.float32 and tuple(g.shape) == wv.shape
                assert np.array_equal(g.cpu().numpy().view(np.int32), wv.view(np.int32))
            # the scales from the device, and a strided map
            got2, _ = ops.rate_map_levels(_t(a, dev), [1.0] * len(scales), scales_dev=_t(np.asarray(scales, dtype=np.float32), dev))
            assert _same(got, got2)
            if len(shape) == 3:
                big = torch.zeros((shape[0], shape[1] + 1, 2 * shape[2]), device=dev)
                big[:, :-1, ::2] = _t(a, dev)
                assert _same(ops.rate_map_levels(big[:, :-1, ::2], scales)[0], got)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------------
def _tables(seed: int):
    rng = np.random.default_rng([77, seed])
    return [torch.from_numpy(rng.dirichlet(np.ones(k), size=SHAPE[1]).astype(np.float32)) for k in SHAPE[2]]


def _model(dev, tables_seed: int = 0, seed: int = 11):
    from mcquic_amd import Compressor
    sd = R.make_state_dict(*SHAPE, seed=seed)
    for lv, t in enumerate(_tables(tables_seed)):
        sd[f"_quantizer._entropyCoder._freqEMA.{lv}"] = t
    model = Compressor(*SHAPE).eval()
    model.load_state_dict(sd, strict=True)
    return model.to(dev)


@pytest.fixture(scope="module")
def shared(dev):
    model, x = _model(dev), R.make_images(2, 128, 128, seed=21).to(dev)
    return model, x, model.encode(x)


def _half_map(dev):
    mp = torch.zeros((2, 8, 8), device=dev)
    mp[:, :, 4:] = 0.5
    return mp


def test_zero_and_per_image_maps(shared, dev):
    model, x, plain = shared
    assert _same(model.encode(x, rd_map=torch.zeros(2, device=dev)), plain)
    assert _same(model.encode(x, rd_map=torch.zeros((2, 8, 8), device=dev), rd_lambda=[1.0, 0.5, 2.0]), plain)
    assert int(model.rateMapError().sum()) == 0
    got = model.encode(x, rd_map=torch.tensor([0.0, 0.5], device=dev))
    assert all(torch.equal(g[0], p[0]) for g, p in zip(got, plain))
    bits, bits0 = model.codeBits(got).sum(-1), model.codeBits(plain).sum(-1)
    assert float(bits[0]) == float(bits0[0]) and float(bits[1]) < float(bits0[1])
    # the scale multiplies the map: scale 0 on every level is the plain cascade, a bad value counts as 0 and is reported
    assert _same(model.encode(x, rd_map=torch.tensor([3.0, 0.5], device=dev), rd_lambda=0.0), plain)
    assert _same(model.encode(x, rd_map=torch.tensor([float("nan"), -1.0], device=dev)), plain)
    assert model.rateMapError().tolist() == [1, 1]


def test_half_zero_grid_map(shared, dev):
    model, x, plain = shared
    got = model.encode(x, rd_map=_half_map(dev))
    assert torch.equal(got[0][..., :4], plain[0][..., :4]) and not torch.equal(got[0][..., 4:], plain[0][..., 4:])
    assert float(model.codeBits(got)[:, 0].sum()) < float(model.codeBits(plain)[:, 0].sum())
    for bad in (torch.zeros((2, 8, 7), device=dev), torch.zeros(2), torch.zeros(2, device=dev, dtype=torch.float64)):
        with pytest.raises(ValueError, match="rd_map"):
            model.encode(x, rd_map=bad)


@pytest.mark.parametrize("coder", ["host", "device"])
def test_streams_round_trip(shared, dev, coder):
    model, x, plain = shared
    for mp, scale in ((_half_map(dev), None), (torch.tensor([0.1, 0.6], device=dev), [1.0, 0.5, 0.0])):
        codes = model.encode(x, rd_map=mp, rd_lambda=scale)
        got, binaries, headers = model.compress(x, coder=coder, rd_map=mp, rd_lambda=scale)
        assert _same(got, codes) and not _same(codes, plain)
        assert torch.equal(model.decompress(binaries, headers, coder=coder), model.decode(codes))


def test_one_capture_serves_every_map_and_scale(dev):
    model, x = _model(dev), R.make_images(2, 128, 128, seed=22).to(dev)
    maps = [_half_map(dev), _half_map(dev).flip(-1) * 3, torch.rand((2, 8, 8), device=dev)]
    runs = [(mp, sc) for mp in maps for sc in (None, [0.5, 1.0, 2.0])] + [(torch.tensor([0.0, 0.5], device=dev), None), (torch.tensor([1.0, 0.1], device=dev), 0.3)]
    eager = [model.encode(x, rd_map=mp, rd_lambda=sc) for mp, sc in runs]
    plain = model.encode(x)
    assert not _same(eager[0], eager[1]) and not _same(eager[0], eager[2])
    model.enableGraphs(True)
    counts = []
    for (mp, sc), want in list(zip(runs, eager)) * 2:
        assert _same(model.encode(x, rd_map=mp, rd_lambda=sc), want)
        counts.append(len(model._graphs))
    assert counts[0] == 1 and counts[5] == 1 and counts[6] == 2 and counts[-1] == 2       # one per map form, whatever the values
    assert _same(model.encode(x), plain) and len(model._graphs) == 3
    # new tables (a new stamp, no weight change): noticed, the capture is taken again under them
    before = model.encode(x, rd_map=maps[0])
    key = [k for k in model._graphs if k[-1] == "rd_map" and len(k[1][1]) == 3][0]
    with torch.no_grad():
        for p, t in zip(model._quantizer._entropyCoder._freqEMA, _tables(1)):
            p.copy_(t.to(dev))
    after = model.encode(x, rd_map=maps[0])
    assert _same(after, _model(dev, tables_seed=1).encode(x, rd_map=maps[0])) and not torch.equal(after[0], before[0])
    model._quantizer._entropyCoder.resetFreqAndCDF()
    old = model._graphs[key]
    again = model.encode(x, rd_map=maps[0])
    assert model._graphs[key] is not old
    assert _same(again, model.enableGraphs(False).encode(x, rd_map=maps[0]))       # (whatever the reset left in the tables)


def test_every_capture_owns_its_error_word(dev):
    """A capture with n = 2, then a call with n = 1 (which must not take the word away from under the graph), then the n = 2 graph
    again: each replay writes the word of its own call, and `rateMapError()` is the last call's, replays included."""
    model, x = _model(dev), R.make_images(2, 128, 128, seed=33).to(dev)
    clean, dirty = torch.tensor([0.25, 0.5], device=dev), torch.tensor([0.25, float("nan")], device=dev)
    want = model.encode(x, rd_map=clean)
    # (1) a caller's own capture
    static_map = clean.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        model.encode(x, rd_map=static_map)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = model.encode(x, rd_map=static_map)
    word = model.rateMapError()                                      # the captured call's: the graph's own
    assert model.encode(x[:1], rd_map=torch.tensor([-1.0], device=dev)) is not None
    other = model.rateMapError()
    assert other.tolist() == [1] and other.data_ptr() != word.data_ptr()
    junk = [torch.full((64,), 7, dtype=torch.int32, device=dev) for _ in range(64)]       # what a freed word's memory would be reused for
    static_map.copy_(dirty)
    graph.replay()
    assert word.tolist() == [0, 1] and other.tolist() == [1] and all(bool((j == 7).all()) for j in junk)
    static_map.copy_(clean)
    graph.replay()
    assert word.tolist() == [0, 0] and _same(out, want)
    # (2) the model's own captures, two batch sizes alive at once
    model.enableGraphs(True)
    assert _same(model.encode(x, rd_map=clean), want) and model.rateMapError().tolist() == [0, 0]
    model.encode(x[:1], rd_map=torch.tensor([float("inf")], device=dev))
    assert model.rateMapError().tolist() == [1]
    model.encode(x, rd_map=dirty)
    assert model.rateMapError().tolist() == [0, 1]
    model.encode(x[:1], rd_map=torch.tensor([0.5], device=dev))
    assert model.rateMapError().tolist() == [0] and all(bool((j == 7).all()) for j in junk)
    assert _same(model.encode(x, rd_map=clean), want) and model.rateMapError().tolist() == [0, 0] and len(model._graphs) == 2


def test_inside_a_callers_capture(dev):
    model, x = _model(dev), R.make_images(2, 128, 128, seed=29).to(dev)
    maps = [_half_map(dev), torch.rand((2, 8, 8), device=dev)]
    want = [model.encode(x, rd_map=mp) for mp in maps]              # (also the warm call: the bits sections exist)
    static_x, static_map = x.clone(), torch.zeros((2, 8, 8), device=dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        model.encode(static_x, rd_map=static_map)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = model.encode(static_x, rd_map=static_map)
    for mp, w in zip(maps, want):
        static_map.copy_(mp)
        graph.replay()
        assert _same(out, w)
    # sections that are not current are refused before anything is launched (the capture is only pretended here)
    model._quantizer._entropyCoder.resetFreqAndCDF()
    import unittest.mock as mock
    with mock.patch.object(torch.cuda, "is_current_stream_capturing", lambda: True):
        with pytest.raises(RuntimeError, match="outside the capture"):
            model._quantizer.rateBitsPacks()


def _replay_checks(model, x, plain, target, out, lambda_max=64.0):
    codes, lam, bpp, tl, tb = out
    n, trials = x.shape[0], tl.shape[0]
    assert lam.dtype == torch.float32 and bpp.dtype == torch.float64 and tuple(tl.shape) == tuple(tb.shape) == (trials, n)
    assert _same(codes, model.encode(x, rd_map=lam))
    b = model.codeBits(codes)
    assert torch.equal(bpp, ((b[:, 0] + b[:, 1]) + b[:, 2]) / float(128 * 128))
    plain_bpp = model.codeBits(plain).sum(-1) / float(128 * 128)
    tgt = target.tolist() if torch.is_tensor(target) else [float(target)] * n
    for i in range(n):
        li, bi = float(lam[i]), float(bpp[i])
        if float(plain_bpp[i]) <= tgt[i]:
            assert li == 0.0 and all(torch.equal(c[i], p[i]) for c, p in zip(codes, plain))
        assert bi <= tgt[i] or li == lambda_max
        rows = [t for t in range(trials) if float(tl[t, i]) == li]
        assert rows and all(float(tb[t, i]) == bi for t in rows)    # equal inputs give equal codes and bits
        lams, answer = MR.replay(tb[:, i].tolist(), tgt[i], lambda_max)
        assert lams == tl[:, i].tolist() and answer == li


def test_encode_to_rate_per_image(shared, dev):
    model, x, plain = shared
    bpp0 = model.codeBits(plain).sum(-1) / float(128 * 128)
    # image 0 already meets its target, image 1 must come down: two targets, two lambdas
    target = torch.stack([bpp0[0] * 1.01, bpp0[1] * 0.8])
    out = model.encode_to_rate(x, target, per_image=True, trace=True)
    print("targets", target.tolist(), "lambda", out[1].tolist(), "bpp", out[2].tolist())
    assert out[3].shape[0] == 14 and float(out[1][0]) == 0.0 and 0.0 < float(out[1][1]) < 64.0
    _replay_checks(model, x, plain, target, out)
    # one float for all, as float32 targets too; without the trace three values come back
    low = float(bpp0.min()) * 0.7
    out = model.encode_to_rate(x, low, per_image=True, trace=True, iters=6)
    assert out[3].shape[0] == 8 and bool((out[1] > 0).all())
    _replay_checks(model, x, plain, low, out)
    assert len(model.encode_to_rate(x, target.float(), per_image=True, iters=2)) == 3
    # unreachable: no exception, the images end at lambda_max and show their bpp
    out = model.encode_to_rate(x, 1e-6, per_image=True, trace=True, iters=3, lambda_max=8.0)
    assert out[1].tolist() == [8.0, 8.0] and bool((out[2] > 1e-6).all())
    _replay_checks(model, x, plain, 1e-6, out, lambda_max=8.0)


def test_the_whole_search_captures(dev):
    """No host read anywhere: a synchronising read would fail the capture."""
    model, x = _model(dev), R.make_images(2, 128, 128, seed=31).to(dev)
    plain = model.encode(x)
    target = (model.codeBits(plain).sum(-1) / float(128 * 128) * torch.tensor([0.85, 0.7], device=dev, dtype=torch.float64))
    want = model.encode_to_rate(x, target, per_image=True, trace=True, iters=5)
    static_x, static_t = x.clone(), target.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        model.encode_to_rate(static_x, static_t, per_image=True, trace=True, iters=5)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = model.encode_to_rate(static_x, static_t, per_image=True, trace=True, iters=5)
    graph.replay()
    assert _same(out[0], want[0]) and all(torch.equal(a, b) for a, b in zip(out[1:], want[1:]))
    static_t.copy_(target.flip(0))                                   # other targets through the same graph
    graph.replay()
    want = model.encode_to_rate(x, target.flip(0), per_image=True, trace=True, iters=5)
    assert _same(out[0], want[0]) and all(torch.equal(a, b) for a, b in zip(out[1:], want[1:]))


def test_neon_refuses_the_new_keywords(dev):
    import mcquic_amd
    model = mcquic_amd.Neon(32, 256, [8, 4, 2, 2]).eval().to(dev)
    x = torch.zeros((1, 3, 128, 128), device=dev)
    with pytest.raises(NotImplementedError):
        model.encode(x, rd_map=torch.zeros(1, device=dev))
    with pytest.raises(NotImplementedError):
        model.compress(x, rd_map=torch.zeros(1, device=dev))
    with pytest.raises(NotImplementedError):
        model.encode_to_rate(x, 0.1, per_image=True)
