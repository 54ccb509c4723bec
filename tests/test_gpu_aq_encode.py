"""Adaptive quantisation through the public interface: `aq` on `encode`, `compress`, `encode_to_rate` (both forms), `validate.rate_sweep`
and the command line, on the smallest model of tests/test_gpu_rate_map.py at 2 x 128 x 128 (and one padded size).  Everything here is
exact: `aq` is the `rd_map` path with a map the device made, so the codes are those of that map, bit for bit."""
import numpy as np
import pytest
import torch

from oracle import mcquic_ref as R

pytestmark = pytest.mark.gpu

SHAPE = (8, 2, [32, 16, 8])
PIXELS = float(128 * 128)


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(s, t) for s, t in zip(a, b))


def _model(dev, seed: int = 11):
    from mcquic_amd import Compressor
    sd = R.make_state_dict(*SHAPE, seed=seed)
    rng = np.random.default_rng([77, 0])
    for lv, k in enumerate(SHAPE[2]):
        sd[f"_quantizer._entropyCoder._freqEMA.{lv}"] = torch.from_numpy(rng.dirichlet(np.ones(k), size=SHAPE[1]).astype(np.float32))
    model = Compressor(*SHAPE).eval()
    model.load_state_dict(sd, strict=True)
    return model.to(dev)


def _images(dev, n, h, w, seed):
    """Images whose right half is nearly flat: the activity map has something to say."""
    x = R.make_images(n, h, w, seed=seed)
    x[..., w // 2:] = x[..., w // 2:] * 0.02 + 0.1
    return x.to(dev).contiguous()


@pytest.fixture(scope="module")
def shared(dev):
    model, x = _model(dev), _images(dev, 2, 128, 128, seed=21)
    return model, x, model.encode(x)


def test_aq_is_the_rd_map_path_with_the_map_the_device_made(shared, dev):
    model, x, plain = shared
    for images in (x, _images(dev, 2, 130, 200, seed=23)):
        w = model.activityWeights(images, 0.5)
        n, h0, w0 = model._rateGrid(images)
        assert tuple(w.shape) == (n, h0, w0) and w.dtype == torch.float32 and float(w.min()) < 0.9 and float(w.max()) > 1.1
        assert model.activityError().tolist() == [0] * n
        for lam in (None, 0.3, [0.5, 0.2, 0.1]):
            got = model.encode(images, rd_lambda=lam, aq=0.5)
            assert _same(got, model.encode(images, rd_lambda=lam, rd_map=w))
            assert not _same(got, model.encode(images, rd_lambda=1.0 if lam is None else lam))
        assert _same(model.encode(images, rd_lambda=0.3, aq=0.0), model.encode(images, rd_lambda=0.3, rd_map=torch.ones_like(w)))
        assert _same(model.encode(images, rd_lambda=0.3, aq=(1.0, 0.5)), model.encode(images, rd_lambda=0.3, rd_map=model.activityWeights(images, (1.0, 0.5))))
        assert 1.4 < float(model.activityWeights(images, (1.0, 0.5)).max()) < 1.4143          # clipped at 2^0.5
        for r in (torch.tensor([0.5, 2.0], device=dev), torch.rand((n, h0, w0), device=dev) * 2):
            want = model.encode(images, rd_lambda=0.3, rd_map=w * (r[:, None, None] if r.dim() == 1 else r))
            assert _same(model.encode(images, rd_lambda=0.3, aq=0.5, rd_map=r), want)
        assert int(model.rateMapError().sum()) == 0
    # aq = None is the code path without it
    assert _same(model.encode(x, aq=None), plain)
    # a bad value of the caller's map is still reported by the map's error word
    model.encode(x, aq=0.5, rd_map=torch.tensor([1.0, float("nan")], device=dev))
    assert model.rateMapError().tolist() == [0, 1]
    # a non-finite pixel: reported, and the encode itself is the rd_map path's
    bad = x.clone()
    bad[1, 0, 5, 5] = float("nan")
    model.activityWeights(bad, 0.5)
    assert model.activityError().tolist() == [0, 1]


def test_bad_aq_values_raise_before_any_launch(shared, dev):
    model, x, _ = shared
    for bad in (-0.5, float("nan"), float("inf"), (1.0, 0.0), (1.0, -1.0), (1.0, float("nan"))):
        for call in (lambda: model.encode(x, aq=bad), lambda: model.compress(x, aq=bad), lambda: model.activityWeights(x, bad),
                     lambda: model.encode_to_rate(x, 0.1, aq=bad), lambda: model.encode_to_rate(x, 0.1, per_image=True, aq=bad)):
            with pytest.raises(ValueError, match="aq"):
                call()


def test_under_enable_graphs_the_codes_are_the_eager_ones(dev):
    model = _model(dev)
    xs = [_images(dev, 2, 128, 128, seed=s) for s in (31, 32)]
    runs = [(x, lam, aq) for x in xs for lam in (0.3, [0.5, 0.2, 0.1]) for aq in (0.5, (1.0, 1.0))]
    eager = [model.encode(x, rd_lambda=lam, aq=aq) for x, lam, aq in runs]
    assert not _same(eager[0], eager[1])
    model.enableGraphs(True)
    for (x, lam, aq), want in list(zip(runs, eager)) * 2:
        assert _same(model.encode(x, rd_lambda=lam, aq=aq), want)
    assert len(model._graphs) == 1                                   # the rd_map capture of this shape serves them all


@pytest.mark.parametrize("coder", ["host", "device"])
def test_streams_round_trip(shared, dev, coder):
    model, x, plain = shared
    codes = model.encode(x, rd_lambda=0.3, aq=0.5)
    got, binaries, headers = model.compress(x, coder=coder, rd_lambda=0.3, aq=0.5)
    assert _same(got, codes) and not _same(codes, plain)
    assert torch.equal(model.decompress(binaries, headers, coder=coder), model.decode(codes))


def test_encode_to_rate_per_image(shared, dev):
    from mcquic_amd import ops
    model, x, plain = shared
    bpp0 = model.codeBits(plain).sum(-1) / PIXELS
    target = torch.stack([bpp0[0] * 1.01, bpp0[1] * 0.8])
    base = model.encode_to_rate(x, target, per_image=True)
    codes, lam, bpp, tl, tb = model.encode_to_rate(x, target, per_image=True, aq=0.5, trace=True)
    print("targets", target.tolist(), "plain search", base[2].tolist(), "aq search", bpp.tolist(), "lambda", lam.tolist())
    assert lam.dtype == torch.float32 and bpp.dtype == torch.float64 and tuple(tl.shape) == tuple(tb.shape) == (14, 2)
    reached = base[2] <= target
    assert bool(reached[0]) and bool((bpp[reached] <= target[reached]).all())
    assert float(lam[0]) == 0.0 and float(lam[1]) > 0.0
    a, mask, _ = ops.activity_cells(x)
    assert _same(codes, model.encode(x, rd_map=ops.activity_weights(a, mask, 0.5, 2.0, lam=lam)))
    b = model.codeBits(codes)
    assert torch.equal(bpp, ((b[:, 0] + b[:, 1]) + b[:, 2]) / PIXELS)
    # the caller's own map under the search, with and without aq
    roi = torch.rand((2, 8, 8), device=dev) + 0.5
    for aq, strength in ((0.5, 0.5), (None, 0.0)):
        codes, lam, bpp = model.encode_to_rate(x, target, per_image=True, aq=aq, rd_map=roi)
        assert bool(((bpp <= target) | (lam == 64.0)).all())
        assert _same(codes, model.encode(x, rd_map=ops.activity_weights(a, mask, strength, 2.0, roi=roi, lam=lam)))


def test_the_whole_per_image_search_captures(dev):
    """No host read anywhere: a synchronising read would fail the capture."""
    model, x = _model(dev), _images(dev, 2, 128, 128, seed=41)
    plain = model.encode(x)
    target = model.codeBits(plain).sum(-1) / PIXELS * torch.tensor([0.85, 0.7], device=dev, dtype=torch.float64)
    want = model.encode_to_rate(x, target, per_image=True, trace=True, iters=4, aq=0.5)
    static_x, static_t = x.clone(), target.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        model.encode_to_rate(static_x, static_t, per_image=True, trace=True, iters=4, aq=0.5)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = model.encode_to_rate(static_x, static_t, per_image=True, trace=True, iters=4, aq=0.5)
    graph.replay()
    assert _same(out[0], want[0]) and all(torch.equal(a, b) for a, b in zip(out[1:], want[1:]))
    other = _images(dev, 2, 128, 128, seed=42)
    static_x.copy_(other)
    static_t.copy_(target.flip(0))
    graph.replay()
    want = model.encode_to_rate(other, target.flip(0), per_image=True, trace=True, iters=4, aq=0.5)
    assert _same(out[0], want[0]) and all(torch.equal(a, b) for a, b in zip(out[1:], want[1:]))


def test_encode_to_rate_batch_form(shared, dev):
    model, x, plain = shared
    bpp0 = float(model.codeBits(plain).sum()) / (2 * PIXELS)
    for aq, roi in ((0.5, None), ((1.0, 1.0), torch.tensor([1.0, 0.5], device=dev)), (None, torch.rand((2, 8, 8), device=dev) + 0.5)):
        codes, lam, bpp = model.encode_to_rate(x, bpp0 * 0.8, iters=6, aq=aq, rd_map=roi)
        assert isinstance(lam, float) and lam > 0.0 and bpp <= bpp0 * 0.8
        assert _same(codes, model.encode(x, rd_lambda=lam, aq=aq, rd_map=roi))
        assert bpp == float(model.codeBits(codes).sum()) / (2 * PIXELS)
    # a target the plain codes meet: lambda 0, the plain codes
    codes, lam, bpp = model.encode_to_rate(x, bpp0 * 1.01, aq=0.5)
    assert lam == 0.0 and _same(codes, plain) and _same(codes, model.encode(x, rd_lambda=0.0, aq=0.5))


def test_rate_sweep_takes_aq(shared, dev):
    from mcquic_amd import validate
    model, x, _ = shared
    rows = validate.rate_sweep(model, x, [0.0, 0.3], msssim=False, aq=0.5)
    off = validate.rate_sweep(model, x, [0.0, 0.3], msssim=False)
    assert tuple(rows.shape) == (2, 4) and rows[:, 3].tolist() == [0.0, 0.3]
    assert torch.equal(rows[0, [0, 2]], off[0, [0, 2]])             # lambda 0: the map scales nothing
    want = model.codeBits(model.encode(x, rd_lambda=0.3, aq=0.5)).sum(-1) / PIXELS
    assert float(rows[1, 2]) == float(want.mean()) and float(rows[1, 2]) != float(off[1, 2])


def test_neon_refuses_aq(dev):
    import mcquic_amd
    model = mcquic_amd.Neon(32, 256, [8, 4, 2, 2]).eval().to(dev)
    x = torch.zeros((1, 3, 128, 128), device=dev)
    for call in (lambda: model.encode(x, aq=0.5), lambda: model.compress(x, aq=0.5), lambda: model.activityWeights(x, 0.5),
                 lambda: model.encode_to_rate(x, 0.1, aq=0.5), lambda: model.encode_to_rate(x, 0.1, per_image=True, aq=0.5)):
        with pytest.raises(NotImplementedError):
            call()


def test_cli_rate_knobs(dev, tmp_path, capsys):
    """`--aq 0.5 --rd-lambda 0.1` writes a `.mcq` that restores; `--target-bpp` prints a bpp at or below the target."""
    import re
    from PIL import Image
    from mcquic_amd.demo import main
    from mcquic_amd.utils import File
    rng = np.random.default_rng(0)
    img = (rng.random((150, 200, 3)) * 255).astype(np.uint8)
    img[:, 100:] = 128 + (img[:, 100:] >> 6)                         # a nearly flat half
    src = tmp_path / "sample.png"
    Image.fromarray(img).save(src)
    mcq = tmp_path / "sample.mcq"
    assert main(["-q", "--aq", "0.5", "--rd-lambda", "0.1", str(src), str(mcq)]) == 0
    doc = File.deserialize(mcq.read_bytes())
    assert doc.FileHeader.ImageSize.height == 150 and doc.FileHeader.ImageSize.width == 200 and len(doc.Content) == 3
    out = tmp_path / "a.png"
    assert main(["-q", str(mcq), str(out)]) == 0
    assert np.asarray(Image.open(out)).shape == (150, 200, 3)
    capsys.readouterr()
    assert main(["--target-bpp", "0.5", "--aq", "0.5", "--aq-clip", "1", str(src), str(tmp_path / "t.mcq")]) == 0
    said = capsys.readouterr().out
    m = re.search(r"target 0\.5000 bpp: lambda (\S+), (\S+) bpp", said)
    assert m is not None, said
    assert 0.0 < float(m.group(2)) <= 0.5
    assert File.deserialize((tmp_path / "t.mcq").read_bytes()).FileHeader.ImageSize.width == 200
