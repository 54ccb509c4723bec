"""mcq_histogram_f32 / mcq_log_distance_f32 (csrc/step_snapshot.hip) alone.

Identity transform: counts and edges BIT-EQUAL to np.histogram of the same values widened to float64 (tests/_snapshot_ref.py restates it and
tests/test_snapshot_ref.py pins that restatement; both are asserted here), on the wave seam, one workgroup's chunk +- 1, several
workgroups plus a tail, values on bin edges, all-equal values, 1 / 64 / 4096 bins, tiny and huge scales, an unaligned slab (the scalar-load
path), and inf / NaN sprinkled in.  The transform is pinned element by element against float64, and the fused histogram against
np.histogram of the unfused kernel's own output, so that the composition holds without a tolerance on bin counts.

Bar of the transform: twice the worst distance measured on an MI355X over exactly the cases of `_snapshot_ref.logit_cases()` (docs/experiments.md
section 23), in float32 spacings at the float64 value; log10f is not correctly rounded on the device or on the host."""
import numpy as np
import pytest
import torch

import _snapshot_ref as R
from _record import record

pytestmark = pytest.mark.gpu
MEASURED_ULP = 1.639        # worst |log_distance - float64| in float32 spacings, measured (section 23: 1.068 on [2, 2, 8], 1.639 on
#                             [4, 4, 512]); the test holds 2 x this
CASES = R.histogram_cases(4096)


def _run(x, bins, transform=0):
    from mcquic_amd import ops
    counts, edges, stats = ops.histogram(x, bins, transform, R.EPS)
    return counts.cpu().numpy(), edges.cpu().numpy(), tuple(stats.cpu().tolist())


def _equal(got, v, bins, where):
    counts, edges, stats = got
    want_counts, want_edges, want_stats = R.histogram(v, bins)
    assert edges.dtype == np.float64 and counts.dtype == np.int64
    assert edges.tobytes() == want_edges.tobytes(), (where, edges[:4], want_edges[:4])
    assert counts.tolist() == want_counts.tolist(), where
    assert stats == want_stats, (where, stats, want_stats)


def test_chunk_is_what_the_cases_were_built_for():
    from mcquic_amd import _lib
    assert _lib.load().mcq_histogram_chunk() == 4096


@pytest.mark.parametrize("name", list(CASES))
def test_identity_is_np_histogram(dev, name):
    v, bins = CASES[name]
    got = _run(torch.from_numpy(v).to(dev), bins)
    _equal(got, v, bins, name)
    want_counts, want_edges = np.histogram(v.astype(np.float64), bins)        # and the real thing, not only its restatement
    assert got[1].tobytes() == want_edges.tobytes() and got[0].tolist() == want_counts.tolist()
    if name == "integers 0..64":
        assert got[0].tolist() == [1] * 63 + [2], "every value on an edge; the maximum in the closed last bin"
    if name == "n=1":
        assert got[1][0] == 0.25 and got[1][-1] == 1.25 and got[0].sum() == 1


def test_unaligned_slab_takes_the_scalar_path(dev):
    """A slab that starts 4 bytes into its allocation: no float4 loads, the same histogram."""
    v, bins = CASES["bins=64"]
    base = torch.zeros(v.size + 1, dtype=torch.float32, device=dev)
    base[1:] = torch.from_numpy(v).to(dev)
    x = base[1:]
    assert x.data_ptr() % 16 == 4
    _equal(_run(x, bins), v, bins, "unaligned")


def test_non_finite_values_are_counted_and_left_out(dev):
    x = R.sprinkled()
    got = _run(torch.from_numpy(x).to(dev), 64)
    _equal(got, x, 64, "sprinkled")
    kept = x[np.isfinite(x)]
    want_counts, want_edges = np.histogram(kept.astype(np.float64), 64)
    assert got[1].tobytes() == want_edges.tobytes() and got[0].tolist() == want_counts.tolist()
    assert got[2] == (kept.size, 40)
    nothing = _run(torch.tensor([float("nan"), float("inf")], device=dev), 4)
    assert nothing[0].tolist() == [0] * 4 and nothing[1].tolist() == [0.0, 0.25, 0.5, 0.75, 1.0] and nothing[2] == (0, 2)


def test_two_calls_give_equal_bits(dev):
    v, bins = CASES["n=100003"]
    x = torch.from_numpy(v).to(dev)
    a, b = _run(x, bins), _run(x, bins)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]
    a, b = _run(x, bins, 1), _run(x, bins, 1)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


def test_transform_element_by_element(dev):
    from mcquic_amd import ops
    worst = 0.0
    for name, x in R.logit_cases().items():
        got = ops.log_distance(torch.from_numpy(x).to(dev), R.EPS).cpu().numpy()
        want = R.log_distance64(x)
        assert got.shape == x.shape and np.isfinite(got).all()
        err = R.ulp_distance(got, want)
        print(f"log_distance {name}: worst {err:.3f} float32 spacings")
        worst = max(worst, err)
        clamped = (-x) < np.float32(R.EPS)
        assert clamped.sum() > 0 and (got[clamped] == got[clamped][0]).all() and abs(float(got[clamped][0]) + 6.0) < 1e-6
    record("step_snapshot/log_distance_ulp", value=worst, bar=2 * MEASURED_ULP)
    print(f"log_distance worst over the cases: {worst:.3f} (bar {2 * MEASURED_ULP})")
    assert worst <= 2 * MEASURED_ULP
    odd = ops.log_distance(torch.tensor([float("nan"), float("-inf"), float("inf")], device=dev), R.EPS).cpu().numpy()
    assert np.isnan(odd[0]) and odd[1] == np.inf and abs(float(odd[2]) + 6.0) < 1e-6      # clamp hands a NaN through, as torch's does


@pytest.mark.parametrize("name", list(R.logit_cases()))
def test_fused_equals_np_histogram_of_the_unfused_output(dev, name):
    from mcquic_amd import ops
    x = torch.from_numpy(R.logit_cases()[name]).to(dev)
    v = ops.log_distance(x, R.EPS).cpu().numpy().reshape(-1)
    got = _run(x, 64, 1)
    want_counts, want_edges = np.histogram(v.astype(np.float64), 64)
    assert got[1].tobytes() == want_edges.tobytes() and got[0].tolist() == want_counts.tolist() and got[2] == (v.size, 0)


def test_fused_on_a_slab_of_several_workgroups(dev):
    """[12, 12, 257] = 37008 values, nine chunks and a tail, some NaN logits: fused == np.histogram of the unfused output's finite part."""
    from mcquic_amd import ops
    g = np.random.default_rng(3)
    x = -(10.0 ** g.uniform(-8, 3, (12, 12, 257))).astype(np.float32)
    x[g.uniform(size=x.shape) < 0.1] *= -1
    x[3, 4, 5] = np.nan
    xd = torch.from_numpy(x).to(dev)
    v = ops.log_distance(xd, R.EPS).cpu().numpy().reshape(-1)
    _equal(_run(xd, 64, 1), v, 64, "fused slab")


def test_refusals(dev):
    from mcquic_amd import ops
    x = torch.zeros(8, device=dev)
    for bins in (0, 4097):
        with pytest.raises(ValueError):
            ops.histogram(x, bins)
    with pytest.raises(ValueError):
        ops.histogram(x, 64, transform=2)
    with pytest.raises(ValueError):
        ops.histogram(x[:0], 64)
    with pytest.raises(TypeError):
        ops.histogram(x.double(), 64)
