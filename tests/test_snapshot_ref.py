"""CPU: the references of tests/_snapshot_ref.py against the real things, so that the GPU tests of csrc/step_snapshot.hip lean on helpers that
were themselves checked: the histogram restatement against np.histogram (counts and edges bit for bit), the code image against the
reference's own expression evaluated by torch, the float64 transform against torch's float32 ops."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _snapshot_ref as R

CASES = R.histogram_cases(4096)


@pytest.mark.parametrize("name", list(CASES))
def test_histogram_helper_is_np_histogram(name):
    v, bins = CASES[name]
    counts, edges, stats = R.histogram(v, bins)
    want_counts, want_edges = np.histogram(v.astype(np.float64), bins)
    assert edges.dtype == want_edges.dtype == np.float64 and counts.dtype == np.int64
    assert edges.tobytes() == want_edges.tobytes(), name
    assert counts.tolist() == want_counts.tolist(), name
    assert stats == (v.size, 0) and int(counts.sum()) == v.size


def test_histogram_helper_on_the_transformed_slab_and_without_the_non_finite():
    for x in R.logit_cases().values():
        v = torch.from_numpy(x).neg().clamp(R.EPS).log10().numpy()
        counts, edges, _ = R.histogram(v, 64)
        want_counts, want_edges = np.histogram(v.astype(np.float64), 64)
        assert edges.tobytes() == want_edges.tobytes() and counts.tolist() == want_counts.tolist()
    x = R.sprinkled()
    counts, edges, stats = R.histogram(x, 64)
    kept = x[np.isfinite(x)]
    want_counts, want_edges = np.histogram(kept.astype(np.float64), 64)
    assert edges.tobytes() == want_edges.tobytes() and counts.tolist() == want_counts.tolist()
    assert stats == (kept.size, 40) and x.size - kept.size == 40
    with pytest.raises(ValueError, match="not finite"):          # what numpy does with them, and the kernels do not
        np.histogram(x, 64)
    counts, edges, stats = R.histogram(np.array([np.nan, np.inf], np.float32), 4)      # nothing finite: numpy's empty range (0, 1)
    assert edges.tolist() == np.histogram(np.array([], np.float64), 4)[1].tolist() and counts.tolist() == [0] * 4 and stats == (0, 2)


def test_the_float64_form_is_the_statement_for_widened_values():
    """Why float64: numpy >= 2 keeps a float32 array's edges in float32; the same values widened give float64 edges, and the float32
    edges are those rounded only where linspace's own arithmetic allows (the outer edges are exact in both)."""
    v, bins = CASES["n=100003"]
    e32, e64 = np.histogram(v, bins)[1], np.histogram(v.astype(np.float64), bins)[1]
    assert e64.dtype == np.float64
    assert float(e32[0]) == e64[0] == float(v.min()) and float(e32[-1]) == e64[-1] == float(v.max())
    assert np.allclose(e32.astype(np.float64), e64, rtol=1e-5, atol=0)


def test_linspace_helper():
    for first, last, bins in ((0.0, 1.0, 7), (-3.75, -2.75, 64), (1e-30, 3e-30, 4096), (-1e30, 1e30, 3), (0.0, 5e-324, 2), (0.25, 64.0, 1)):
        assert R.linspace(first, last, bins).tobytes() == np.linspace(np.float64(first), np.float64(last), bins + 1).tobytes()


def test_log_distance_reference_against_torch():
    """The float64 transform rounded to float32 is within 1 ulp of torch's float32 `(-x).clamp(eps).log10()` away from log10's zero (next
    to v = 1 the float32 ops differ by more in ulps of a tiny result: the GPU test measures that), and the clamp acts where it should."""
    for x in R.logit_cases().values():
        got = torch.from_numpy(x).neg().clamp(R.EPS).log10().numpy().reshape(-1)
        want = R.log_distance64(x).reshape(-1)
        big = np.abs(want) > 1e-3
        assert np.isfinite(want).all()
        assert R.ulp_distance(got[big], want[big]) <= 2.0
        clamped = (-x.reshape(-1)) < np.float32(R.EPS)
        assert clamped.sum() > 0 and (got[clamped] == np.float32(np.log10(np.float64(np.float32(R.EPS))))).all()
    assert np.isnan(R.log_distance64(np.array([np.nan], np.float32))[0]) and R.log_distance64(np.array([-np.inf], np.float32))[0] == np.inf


@pytest.mark.parametrize("shape,top", [((1, 1, 1, 1), 5), ((2, 2, 3, 5), 100), ((3, 2, 16, 16), 8191)])
def test_code_image_helper_is_the_reference_expression(shape, top):
    g = torch.Generator().manual_seed(3)
    codes = torch.randint(0, top + 1, shape, generator=g)
    codes.view(-1)[-1] = top
    if shape[1] > 1:
        codes[:, 0].clamp_(max=top // 2)                       # the maximum lives in group 1
    want = F.interpolate(R.detransform((codes.float() / codes.max() - 0.5) * 2)[:, :1], scale_factor=4, mode="nearest")
    assert want.dtype == torch.uint8 and torch.equal(R.code_image(codes), want)
    assert torch.equal(R.code_image(codes, keep=1), want[:1])
    if shape[1] > 1:
        group0 = F.interpolate(R.detransform((codes.float() / codes[:, :1].max() - 0.5) * 2)[:, :1], scale_factor=4, mode="nearest")
        assert not torch.equal(group0, want), "a group-0 maximum must be told apart by this case"
    assert int(R.code_image(torch.zeros(shape, dtype=torch.int64)).max()) == 0


def test_normalized_freq_helper_against_torch():
    g = np.random.default_rng(5)
    freqs = [g.uniform(0, 1, (2, 64)).astype(np.float32), g.uniform(0, 1, (3, 37)).astype(np.float32)]
    freqs[0][1, :5] = 0.0
    freqs[1][0, 3] = 1e-9
    rows, usage = R.normalized_freq(freqs)
    want = [torch.from_numpy(f) / torch.from_numpy(f).sum(-1, keepdim=True) for f in freqs]
    for r, w in zip(rows, want):
        # torch's float32 row sum is within a few ulp of the exact one, and so is every quotient
        assert np.allclose(r, w[0].numpy(), rtol=8 * 2.0 ** -24, atol=0)
    assert usage == torch.cat([(w > 1e-6).flatten() for w in want]).float().mean().item()
