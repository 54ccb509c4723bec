"""GPU: mcquic_amd.kmeans (lloyd_step, fit_codebooks) and UMGMQuantizer.quantizerInputs on top of the k-means kernels."""
import numpy as np
import pytest
import torch

import _kmeans_ref as R

pytestmark = pytest.mark.gpu


def _bits(t):
    return t.view({torch.float64: torch.int64, torch.float32: torch.int32}.get(t.dtype, t.dtype))


def _images(seed, n=2, side=64, count=2):
    gen = torch.Generator().manual_seed(seed)
    return [torch.rand((n, 3, side, side), generator=gen) * 2 - 1 for _ in range(count)]


def _model(dev, channel, k, seed=7):
    from mcquic_amd import Compressor
    torch.manual_seed(seed)
    return Compressor(channel, 2, k).eval().to(dev)


def _twin(model, dev, channel, k):
    """A second model with the same weights (its own parameters and caches)."""
    other = _model(dev, channel, k, seed=8)
    other.load_state_dict(model.state_dict())
    return other


def test_lloyd_step_on_separated_blobs(dev):
    """m = 2, d = 16, k = 8: eight blobs per group (points at centre +- 1e-3, centres >= 1 apart), codeword c starts at blob c's
    centre + 0.05 per coordinate (0.2 away, every other centre >= 1 away): assignments are unambiguous, so two steps must land
    every codeword within 1 ulp of its blob's float64 mean, leave none empty, and the second step's inertia is the within-cluster
    sum of squares (against the codewords the step started from) to the leaf bound 1e-12 sum_v (|x_v|^2 + |c_old|^2)."""
    from torch import nn
    from mcquic_amd import kmeans
    from mcquic_amd.modules.quantizer import _CodebookCache, _multiCodebookQuantization
    m, d, k, N, h, w = 2, 16, 8, 4, 4, 6
    V = N * h * w
    rs = np.random.RandomState(5)
    centres = rs.normal(size=(m, k, d)) * 3.0
    gaps = np.linalg.norm(centres[:, :, None] - centres[:, None], axis=-1) + 10.0 * np.eye(k)
    assert gaps.min() >= 1.0
    labels = np.stack([rs.permutation(np.repeat(np.arange(k), V // k)) for _ in range(m)])            # [m, V]
    pts = (centres[np.arange(m)[:, None], labels] + rs.uniform(-1e-3, 1e-3, size=(m, V, d))).astype(np.float32)
    x = torch.from_numpy(pts.reshape(m, N, h * w, d).transpose(1, 0, 3, 2).reshape(N, m * d, h, w).copy()).to(dev)
    assert np.array_equal(R.vectors(x.cpu().numpy(), m), pts.astype(np.float64))
    quant = _multiCodebookQuantization(nn.Parameter(torch.from_numpy((centres + 0.05).astype(np.float32)).to(dev)), _CodebookCache())
    means = np.stack([[pts[g][labels[g] == c].astype(np.float64).mean(0) for c in range(k)] for g in range(m)])
    for step in range(2):
        before = quant._codebook.detach().cpu().numpy().astype(np.float64)
        inertia, empty = kmeans.lloyd_step(quant, x)
        got = quant._codebook.detach().cpu().numpy()
        want = means.astype(np.float32)
        assert (np.abs(got.astype(np.float64) - want) <= np.maximum(np.spacing(np.abs(want)), np.spacing(np.abs(got)))).all()
        assert empty.tolist() == [0, 0]
    wcss = ((pts.astype(np.float64) - before[np.arange(m)[:, None], labels]) ** 2).sum((1, 2))
    scale = (pts.astype(np.float64) ** 2).sum((1, 2)) + (before[np.arange(m)[:, None], labels] ** 2).sum((1, 2))
    err = np.abs(inertia.cpu().numpy() - wcss)
    print("inertia", inertia.tolist(), "wcss", wcss.tolist(), "error / bound", (err / (1e-12 * scale)).tolist())
    assert (err <= 1e-12 * scale).all()


def test_fit_is_the_by_hand_sequence(dev):
    """fit_codebooks(iters=1, levels=[0], init="current", reseed_empty=False) = quantizerInputs -> vq_assign -> accumulate (both
    batches) -> update on a copy of the model, bit for bit; the other levels stay as they were."""
    from mcquic_amd import kmeans, ops
    k = [64, 32, 16]
    model = _model(dev, 32, k)
    twin = _twin(model, dev, 32, k)
    batches = [b.to(dev) for b in _images(11)]
    start = [c.detach().clone() for c in model.Codebooks]
    report = kmeans.fit_codebooks(model, batches, iters=1, levels=[0], init="current", reseed_empty=False)
    with torch.no_grad():
        cb = twin.Codebooks[0].detach().clone()
        acc = ops.KMeansAcc(*cb.shape, dev)
        packed = ops.PackedCodebook(cb)
        for b in batches:
            qin = twin._quantizer.quantizerInputs(twin._encode_latent(b))[0]
            ops.vq_kmeans_accumulate(qin, ops.vq_assign(qin, packed), acc)
        inertia, empty = ops.vq_kmeans_update(cb, acc)
    assert not torch.equal(model.Codebooks[0].detach(), start[0])
    assert torch.equal(_bits(model.Codebooks[0].detach()), _bits(cb))
    assert torch.equal(_bits(report[0].inertia), _bits(inertia[None])) and torch.equal(report[0].empty, empty[None])
    assert report[1] is None and report[2] is None
    for lv in (1, 2):
        assert torch.equal(_bits(model.Codebooks[lv].detach()), _bits(start[lv]))


@pytest.fixture(scope="module")
def fits(dev):
    """Three full fits (iters = 4) of the same weights on the same two batches: seed 0 twice, seed 1 once."""
    from mcquic_amd import kmeans
    k = [64, 32, 16]
    first = _model(dev, 32, k)
    batches = [b.to(dev) for b in _images(12)]
    out = []
    for seed in (0, 0, 1):
        model = _twin(first, dev, 32, k)
        out.append((model, kmeans.fit_codebooks(model, batches, iters=4, seed=seed)))
    return batches, out


def test_full_fit_is_deterministic_and_seeded(fits):
    _, ((a, ra), (b, rb), (c, _)) = fits
    for lv in range(3):
        assert torch.equal(_bits(a.Codebooks[lv].detach()), _bits(b.Codebooks[lv].detach()))
        assert torch.equal(_bits(ra[lv].inertia), _bits(rb[lv].inertia)) and torch.equal(ra[lv].empty, rb[lv].empty)
    assert not torch.equal(a.Codebooks[0].detach(), c.Codebooks[0].detach())


def test_full_fit_lowers_inertia_and_empties(fits):
    _, ((_, report), _, _) = fits
    for lv, r in enumerate(report):
        assert r.inertia.shape == (4, 2) and r.empty.shape == (4, 2) and r.inertia.dtype == torch.float64
        print("level", lv, "inertia", r.inertia.tolist(), "empty", r.empty.tolist())
        assert (r.inertia[-1] < r.inertia[0]).all()
        assert (r.empty[-1] <= r.empty[0]).all()


def test_encode_and_decode_see_the_fitted_codebooks(fits):
    from mcquic_amd import ops
    batches, ((model, _), _, _) = fits
    x = batches[0]
    codes = model.encode(x)
    with torch.no_grad():
        inputs = model._quantizer.quantizerInputs(model._encode_latent(x))
    for lv, (code, qin, k) in enumerate(zip(codes, inputs, [64, 32, 16])):
        assert int(code.min()) >= 0 and int(code.max()) < k
        assert torch.equal(code, ops.vq_assign(qin, ops.PackedCodebook(model.Codebooks[lv])))
    assert torch.isfinite(model.decode(codes)).all()


def test_neon_is_out_of_scope(dev):
    from mcquic_amd import Neon, kmeans
    with pytest.raises(NotImplementedError):
        kmeans.fit_codebooks(Neon(32, 256, [8, 4, 2, 2]), [torch.zeros(1, 3, 64, 64, device=dev)])


def test_fit_with_four_dimensional_codewords(dev):
    """Compressor(8, 2, [32, 16, 8]): d = 4."""
    from mcquic_amd import kmeans
    k = [32, 16, 8]
    first = _model(dev, 8, k)
    batches = [b.to(dev) for b in _images(13)]
    runs = []
    for _ in range(2):
        model = _twin(first, dev, 8, k)
        runs.append((model, kmeans.fit_codebooks(model, batches, iters=2, seed=3)))
    (a, ra), (b, rb) = runs
    for lv in range(3):
        assert a.Codebooks[lv].shape[-1] == 4
        assert torch.isfinite(a.Codebooks[lv]).all()
        assert torch.equal(_bits(a.Codebooks[lv].detach()), _bits(b.Codebooks[lv].detach()))
        assert torch.equal(_bits(ra[lv].inertia), _bits(rb[lv].inertia)) and torch.equal(ra[lv].empty, rb[lv].empty)
