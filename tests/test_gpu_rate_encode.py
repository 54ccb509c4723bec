"""Rate-constrained encoding on the device: the penalised pack (mcq_vq_pack_codebook_rate_f32) and `vq_assign` on it against the float64
references of tests/_rate_ref.py, then the `rd_lambda` knob and the target-rate search of `Compressor` on the smallest model of
tests/test_gpu_model.py at 2 x 128 x 128.

Bars.  Pack: lambda = 0 is the plain pack bit for bit; else every finite norm is within ONE float32 ulp of the documented sequence
fl32(c2 + fl32(lambda fl32(16 - log2 width))) evaluated with float64's log2 (`_rate_ref.norms_f32`: the device's log2 may differ from
the host's in its last place before the one rounding to float32, nothing else may differ).  Assignment: the float64 argmin, a
differing position excused only inside (d + 4) 2^-23 (|x|^2 + |c|^2 + 2 |x.c| + lambda bits), at most 1 % of the positions of a
(k, d) case (tests/test_rate_ref.py shows float32 arithmetic staying under that on these seeds)."""
import numpy as np
import pytest
import torch

import _rate_ref as RR
from oracle import mcquic_ref as R

pytestmark = pytest.mark.gpu

SHAPE = (8, 2, [32, 16, 8])


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---- the pack ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", RR.PACK_DS)
@pytest.mark.parametrize("k", RR.PACK_KS)
@pytest.mark.parametrize("m", RR.PACK_MS)
def test_pack_sections(dev, m, k, d):
    from mcquic_amd import ops
    _, cb, cdf = RR.make_case(m, k, d, 1, 1)
    plain = ops.PackedCodebook(_t(cb, dev))
    zero = ops.pack_codebook_rate(_t(cb, dev), _t(cdf, dev), 0.0)
    assert (zero.m, zero.k, zero.d) == (m, k, d) and torch.equal(zero.codebook, plain.codebook)
    assert _bits_equal(zero.packed, plain.packed), "lambda = 0 must be the plain pack bit for bit"
    g, word, kind = RR.norm_section_layout(m, k)
    nn_ = len(kind)
    plain_norms = plain.packed[-nn_:].cpu().numpy()
    assert np.array_equal(plain_norms[kind == 0], RR.c2_f32(cb)[g[kind == 0], word[kind == 0]])
    for lam in RR.LAMBDAS:
        got = ops.pack_codebook_rate(_t(cb, dev), _t(cdf, dev), lam).packed
        assert got.numel() == plain.packed.numel()
        assert _bits_equal(got[:-nn_], plain.packed[:-nn_]), "the codeword section is vq_pack_kernel's"
        norms = got[-nn_:].cpu().numpy()
        assert np.array_equal(np.isinf(norms), np.isinf(plain_norms)) and (norms[kind == 1] == np.inf).all()
        assert np.array_equal(norms == 0, plain_norms == 0) and not np.signbit(norms[kind == 2]).any() and (norms[kind == 2] == 0).all()
        want = RR.norms_f32(cb, cdf, lam)[g[kind == 0], word[kind == 0]]
        have = norms[kind == 0]
        ulps = np.abs(have.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want)).astype(np.float64)
        print(f"m{m} k{k} d{d} lambda {lam}: worst {ulps.max():.2f} ulp, {int((ulps > 0).sum())} of {ulps.size} entries off")
        assert np.isfinite(have).all() and ulps.max() <= 1.0
        assert (have > plain_norms[kind == 0]).all()                # every valid slot costs something: width <= 65536 - (k - 1)


def test_pack_writes_inf_for_an_empty_slot_and_refuses_bad_arguments(dev):
    from mcquic_amd import ops
    _, cb, cdf = RR.make_case(1, 5, 3, 1, 1)
    cdf = cdf.copy()
    cdf[0, 3] = cdf[0, 2]                                           # slot 2 is empty (no valid table has one)
    g, word, kind = RR.norm_section_layout(1, 5)
    for lam in (0.0, 0.25):
        norms = ops.pack_codebook_rate(_t(cb, dev), _t(cdf, dev), lam).packed[-len(kind):].cpu().numpy()
        assert np.isinf(norms[(kind == 0) & (word == 2)]).all() and np.isfinite(norms[(kind == 0) & (word != 2)]).all()
    for lam in (-1.0, float("nan"), float("inf"), 1e39):           # 1e39: a finite double, inf as the float32 the kernel takes
        with pytest.raises(ValueError):
            ops.pack_codebook_rate(_t(cb, dev), _t(cdf, dev), lam)
    with pytest.raises(ValueError):
        ops.pack_codebook_rate(_t(cb, dev), _t(cdf[:, :-1], dev), 0.5)
    with pytest.raises(TypeError):
        ops.pack_codebook_rate(_t(cb, dev), _t(cdf.astype(np.int64), dev), 0.5)


# ---- the assignment ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", RR.PACK_DS)
@pytest.mark.parametrize("k", RR.PACK_KS)
def test_assign_on_the_penalised_pack(dev, k, d):
    from mcquic_amd import ops
    positions = differ = 0
    for m in RR.PACK_MS:
        for (h, w) in RR.MAPS:
            x, cb, cdf = RR.make_case(m, k, d, h, w)
            bits = RR.penalty_table(cdf)
            for lam in RR.LAMBDAS:
                pack = ops.pack_codebook_rate(_t(cb, dev), _t(cdf, dev), lam)
                got = ops.vq_assign(_t(x, dev), pack).cpu().numpy()
                assert got.shape == (2, m, h, w) and got.dtype == np.int64
                dn, unexcused = RR.audit(x, cb, bits, lam, got)
                assert unexcused == 0, f"m{m} {h}x{w} lambda {lam}: {unexcused} codes differ from float64 beyond the rounding bound"
                positions += got.size
                differ += dn
                # the penalty is at work: these codes are not the plain ones
                if h * w > 1:
                    assert not np.array_equal(got, RR.penalised_argmin(x, cb, bits, 0.0))
    print(f"k{k} d{d}: {differ} of {positions} positions excused")
    assert differ <= RR.EXCUSED_CAP * positions


@pytest.mark.parametrize("m, k, d, symbol", [(2, 5, 1, 3), (2, 129, 3, 128), (1, 512, 64, 200)])
def test_a_dominant_symbol_takes_every_code(dev, m, k, d, symbol):
    from mcquic_amd import ops
    x, cb, _ = RR.make_case(m, k, d, 5, 7)
    cdf = RR.dominant_table(m, k, symbol)
    pack = ops.pack_codebook_rate(_t(cb, dev), _t(cdf, dev), 1e30)
    got = ops.vq_assign(_t(x, dev), pack)
    assert bool((got == symbol).all())
    with pytest.raises(ValueError):
        ops.pack_codebook_rate(_t(cb, dev), _t(cdf, dev), float("inf"))


# ---- the model -------------------------------------------------------------------------------------------------------------------------------
def _tables(seed: int):
    """Non-uniform frequency EMAs (the synthetic state dict's are uniform: every penalty equal, lambda without effect)."""
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
    """One model and batch for the tests that change neither."""
    return _model(dev), R.make_images(2, 128, 128, seed=21).to(dev)


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


def test_lambda_zero_is_encode(shared):
    model, x = shared
    plain = model.encode(x)
    assert _same(model.encode(x, rd_lambda=0.0), plain) and _same(model.encode(x, rd_lambda=[0.0, 0.0, 0.0]), plain)
    assert _same(model.compress(x, rd_lambda=0.0)[0], plain)


def test_level0_bits_fall_with_lambda(shared):
    """Level 0 sees the same input at every lambda, so its bits under argmin (dist + lambda bits) cannot rise with lambda."""
    model, x = shared
    bits = [float(model.codeBits(model.encode(x, rd_lambda=lam))[:, 0].sum()) for lam in (0.0, 0.05, 0.5)]
    print("level-0 bits at lambda 0, 0.05, 0.5:", bits)
    assert bits[0] >= bits[1] >= bits[2] and bits[2] < bits[0]


def test_per_level_lambdas(shared):
    """A lambda on the last level only leaves the levels above it alone."""
    model, x = shared
    plain, last = model.encode(x), model.encode(x, rd_lambda=[0.0, 0.0, 0.5])
    assert _same(last[:2], plain[:2]) and not torch.equal(last[2], plain[2])


@pytest.mark.parametrize("coder", ["host", "device"])
@pytest.mark.parametrize("lam", [0.05, [0.5, 0.25, 0.0]])
def test_streams_round_trip(shared, coder, lam):
    model, x = shared
    codes = model.encode(x, rd_lambda=lam)
    got_codes, binaries, headers = model.compress(x, coder=coder, rd_lambda=lam)
    assert _same(got_codes, codes)
    assert torch.equal(model.decompress(binaries, headers, coder=coder), model.decode(codes))
    assert not _same(codes, model.encode(x))


def test_graph_replays_never_cross_lambdas(dev):
    model, x = _model(dev), R.make_images(2, 128, 128, seed=22).to(dev)
    a, b = 0.05, 0.5
    eager = {lam: model.encode(x) if lam is None else model.encode(x, rd_lambda=lam) for lam in (a, None, b)}
    assert not _same(eager[a], eager[None]) and not _same(eager[a], eager[b])
    model.enableGraphs(True)
    for lam in (a, None, b, a, None, b):
        got = model.encode(x) if lam is None else model.encode(x, rd_lambda=lam)
        assert _same(got, eager[lam]), f"replay at lambda {lam}"
    assert len(model._graphs) == 3
    x2 = R.make_images(2, 128, 128, seed=23).to(dev)                 # new data through the captures
    want = model.enableGraphs(False).encode(x2, rd_lambda=b)
    assert _same(model.enableGraphs(True).encode(x2, rd_lambda=b), want)


def test_captures_own_their_packs(dev):
    """A captured penalised encode must never replay on packs that the per-level cache has dropped: between two graphed encodes at
    one lambda the cache is walked through more lambdas than it keeps (eagerly, by `encode_to_rate`, and under graphs), and the
    tables' stamp is bumped (`resetFreqAndCDF`, which the weight fingerprint cannot see).  Every result equals the eager one, and a
    capture and its packs are the same objects for as long as the capture is kept."""
    import gc
    from mcquic_amd.modules.quantizer import _RatePackCache
    model, x = _model(dev), R.make_images(2, 128, 128, seed=27).to(dev)
    lams = [0.5, 0.02, 0.04, 0.08, 0.16, 0.32, 0.64]
    assert len(lams) > _RatePackCache.KEEP + 1
    eager = {lam: model.encode(x, rd_lambda=lam) for lam in lams}
    plain = model.encode(x)
    model.enableGraphs(True)
    a = lams[0]
    key = lambda lam: [k for k in model._graphs if len(k) == 4 and k[3] == model._quantizer.rateLambdas(lam)]      # noqa: E731
    assert _same(model.encode(x, rd_lambda=a), eager[a])
    first = model._graphs[key(a)[0]]
    packs = first.owns
    assert packs is not None and len(packs) == 3
    ptrs = [p.packed.data_ptr() for p in packs]
    # (1) the cache forgets a's packs: other lambdas through the quantizer itself (no capture involved), then the search
    with torch.no_grad():
        y = model._encode_latent(x)
        for lam in lams[1:]:
            model._quantizer.encode(y, rd_lambda=lam)
    model.encode_to_rate(x, 0.8 * float(model.codeBits(plain).sum()) / (2 * 128 * 128))
    cached = [p for c in model._quantizer.__dict__["_rateCaches"] for p in c._packs.values()]
    assert not any(p is q for p in cached for q in packs), "the cache was meant to have dropped them"
    gc.collect()
    junk = [torch.full((1 << 16,), float("nan"), device=dev) for _ in range(8)]       # what a freed pack's memory would be reused for
    assert _same(model.encode(x, rd_lambda=a), eager[a])
    assert model._graphs[key(a)[0]] is first and [p.packed.data_ptr() for p in first.owns] == ptrs
    del junk
    # (2) ... and under graphs: every lambda twice round, each equal to its eager codes; the captures stay bounded
    for lam in lams + lams:
        assert _same(model.encode(x, rd_lambda=lam), eager[lam]), f"replay at lambda {lam}"
        assert _same(model.encode(x), plain)
    owned = [g for g in model._graphs.values() if g.owns is not None]
    assert len(owned) <= model.RATE_CAPTURES and len(model._graphs) == len(owned) + 1
    # (3) the tables' stamp moves without a weight change: the stale capture is dropped, not replayed
    before = model._graphs[key(lams[-1])[0]]
    model._quantizer._entropyCoder.resetFreqAndCDF()
    assert _same(model.encode(x, rd_lambda=lams[-1]), eager[lams[-1]])
    assert model._graphs[key(lams[-1])[0]] is not before


def test_rate_captures_are_bounded(dev):
    model, x = _model(dev), R.make_images(2, 128, 128, seed=28).to(dev)
    model.enableGraphs(True)
    model.encode(x)
    for i in range(model.RATE_CAPTURES + 3):
        model.encode(x, rd_lambda=0.01 * (i + 1))
    owned = [k for k, g in model._graphs.items() if g.owns is not None]
    assert len(owned) == model.RATE_CAPTURES and len(model._graphs) == model.RATE_CAPTURES + 1
    # the most recent ones stayed
    assert owned[-1][3] == model._quantizer.rateLambdas(0.01 * (model.RATE_CAPTURES + 3))


def test_inside_a_callers_capture(dev, monkeypatch):
    """Cached and current packs are handed out while a stream is capturing (nothing is built or read there); anything else is a
    RuntimeError that says what to do."""
    model, x = _model(dev), R.make_images(2, 128, 128, seed=29).to(dev)
    want = model.encode(x, rd_lambda=0.25)
    packs = model._quantizer.ratePacks(model._quantizer.rateLambdas(0.25))             # the caller keeps them with its graph
    static = x.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        model.encode(static, rd_lambda=0.25)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = model.encode(static, rd_lambda=0.25)
    static.copy_(x)
    graph.replay()
    assert _same(out, want) and len(packs) == 3
    # not cached / stale: refused before anything is launched (the capture itself is only pretended here)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(RuntimeError, match="outside the capture"):
        model._quantizer.ratePacks(model._quantizer.rateLambdas(0.75))
    assert all(a is b for a, b in zip(model._quantizer.ratePacks(model._quantizer.rateLambdas(0.25)), packs))
    model._quantizer._entropyCoder.resetFreqAndCDF()
    with pytest.raises(RuntimeError, match="outside the capture"):
        model._quantizer.ratePacks(model._quantizer.rateLambdas(0.25))


@pytest.mark.parametrize("graphs", [False, True])
def test_new_tables_are_followed(dev, graphs):
    model, x = _model(dev, tables_seed=0), R.make_images(2, 128, 128, seed=24).to(dev)
    model.enableGraphs(graphs)
    before = model.encode(x, rd_lambda=0.5)
    with torch.no_grad():
        for p, t in zip(model._quantizer._entropyCoder._freqEMA, _tables(1)):
            p.copy_(t.to(dev))
    after = model.encode(x, rd_lambda=0.5)
    fresh = _model(dev, tables_seed=1).encode(x, rd_lambda=0.5)
    assert _same(after, fresh) and not torch.equal(after[0], before[0])


def test_packs_are_built_only_when_lambda_or_tables_change(dev):
    from mcquic_amd import ops
    model, x = _model(dev), R.make_images(2, 128, 128, seed=25).to(dev)
    lib = ops._lib.load()
    real, calls = lib.mcq_vq_pack_codebook_rate_f32, [0]

    def counting(*a):
        calls[0] += 1
        return real(*a)
    lib.mcq_vq_pack_codebook_rate_f32 = counting
    try:
        model.encode(x)
        assert calls[0] == 0
        model.encode(x, rd_lambda=0.5); model.encode(x, rd_lambda=0.5); model.compress(x, rd_lambda=0.5)
        assert calls[0] == 3
        model.encode(x, rd_lambda=0.25); model.encode(x, rd_lambda=0.5)
        assert calls[0] == 6
        model._quantizer._entropyCoder.resetFreqAndCDF()
        model.encode(x, rd_lambda=0.5)
        assert calls[0] == 9
    finally:
        lib.mcq_vq_pack_codebook_rate_f32 = real


def test_a_bad_table_row_raises_what_compress_raises(dev):
    model, x = _model(dev), R.make_images(2, 128, 128, seed=26).to(dev)
    with torch.no_grad():
        model._quantizer._entropyCoder._freqEMA[1][1, 3] = float("nan")
    with pytest.raises(ValueError) as e1:
        model.compress(x)
    with pytest.raises(ValueError) as e2:
        model.encode(x, rd_lambda=0.5)
    assert str(e1.value) == str(e2.value)


def test_encode_to_rate(shared):
    model, x = shared
    pixels = x.shape[0] * x.shape[-2] * x.shape[-1]
    plain = model.encode(x)
    bpp0 = float(model.codeBits(plain).sum()) / pixels
    # a target above the plain rate: lambda 0, the plain codes
    codes, lam, bpp = model.encode_to_rate(x, bpp0 * 1.01)
    assert lam == 0.0 and bpp == bpp0 and _same(codes, plain)
    # a target below it
    target = 0.8 * bpp0
    codes, lam, bpp = model.encode_to_rate(x, target)
    print(f"plain {bpp0:.5f} bpp; target {target:.5f}: lambda {lam:.6g}, {bpp:.5f} bpp")
    assert 0.0 < lam <= 64.0 and bpp <= target
    assert bpp == float(model.codeBits(codes).sum()) / pixels
    assert _same(codes, model.encode(x, rd_lambda=lam))
    # twelve trials land close under the target, not just anywhere below it
    assert bpp >= 0.9 * target
    # no lambda up to lambda_max reaches this
    with pytest.raises(ValueError, match="bpp"):
        model.encode_to_rate(x, 1e-6)
    with pytest.raises(ValueError, match="bpp"):
        model.encode_to_rate(x, target, lambda_max=lam / 1024)


def test_rate_sweep_rows(shared):
    from mcquic_amd import validate
    model, x = shared
    lams = [0.0, 0.05, 0.5]
    for bits in ("estimated", "exact"):
        rows = validate.rate_sweep(model, x, lams, bits=bits, msssim=False)
        assert tuple(rows.shape) == (3, 4) and rows.dtype == torch.float64
        assert rows[:, 3].tolist() == lams and torch.isnan(rows[:, 1]).all() and torch.isfinite(rows[:, [0, 2]]).all()
        base = validate.validate(model, x, msssim=False, gather=False, bits=bits).mean(0)
        assert torch.equal(rows[0, [0, 2]], base[[0, 2]])
        if bits == "estimated":                                     # the bpp column is codeBits of that lambda's codes
            for row, lam in zip(rows, lams):
                want = (model.codeBits(model.encode(x, rd_lambda=lam)).sum(-1) / float(128 * 128)).mean()
                assert float(row[2]) == float(want)


def test_neon_has_no_rate_knob(dev):
    import mcquic_amd
    model = mcquic_amd.Neon(32, 256, [8, 4, 2, 2]).eval().to(dev)
    x = torch.zeros((1, 3, 128, 128), device=dev)
    with pytest.raises(NotImplementedError):
        model.encode(x, rd_lambda=0.5)
    with pytest.raises(NotImplementedError):
        model.compress(x, rd_lambda=0.5)
    with pytest.raises(NotImplementedError):
        model.encode_to_rate(x, 0.1)
