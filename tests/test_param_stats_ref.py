"""CPU: tests/_param_stats_ref.py, the float64 reference the GPU tests of monitor.ParamStats compare against, on cases worked out by
hand -- and the host-side surface of the feature that needs no device (the class exists, its entry points are typed, sizes)."""
import math

import numpy as np
import pytest

import _param_stats_ref as R

NAN, INF = float("nan"), float("inf")


def test_one_element():
    assert R.columns([-3.0], [4.0], [-1.0]).tolist() == [3.0, 4.0, 4.0, 0.0, 2.0]
    assert R.columns([0.0], [0.0], [0.0]).tolist() == [0.0, 0.0, 0.0, 0.0, 0.0]
    assert R.columns([2.0], None, [2.0]).tolist() == [2.0, 0.0, 0.0, 0.0, 0.0]           # no gradient: zeros


def test_all_nan_gradient():
    got = R.columns([3.0, 4.0, 0.0], [NAN, NAN, NAN], [3.0, 4.0, 0.0])
    assert got.tolist() == [5.0, 0.0, 0.0, 3.0, 0.0]


def test_infinities_mixed_with_finite_values():
    got = R.columns([1.0, 2.0, 2.0, 4.0, 0.0], [INF, 3.0, -INF, -4.0, NAN], [0.0, 0.0, 0.0, 0.0, 0.0])
    assert got.tolist() == [5.0, 5.0, 4.0, 3.0, 5.0]                                     # norm and maximum over {3, -4} only


def test_update_column_rules():
    assert math.isnan(R.columns([1.0], [1.0], [0.0], updates=False)[4])
    assert R.columns([1.0], [1.0], None, updates=True)[4] == 0.0                         # a row that does not read the shadow
    assert R.columns([], [], [])[:4].tolist() == [0.0, 0.0, 0.0, 0.0] and R.columns([], [], [])[4] == 0.0


def test_sums_are_float64():
    """Squares that overflow or flush in float32 do neither here."""
    big, small = np.full(4, 1e30, dtype=np.float32), np.full(4, 1e-30, dtype=np.float32)
    assert R.columns(big, small, big)[0] == pytest.approx(2e30, rel=1e-7) and R.columns(big, small, big)[1] == pytest.approx(2e-30, rel=1e-7)


def test_recording_rule():
    assert R.is_recorded(0, 1, False) == (True, True) and R.is_recorded(5, 1, False) == (True, True)
    assert R.is_recorded(4, 2, False) == (True, True) and R.is_recorded(5, 2, False) == (False, False)
    assert R.is_recorded(5, 2, True) == (True, False)                                    # forced by the skip flag: recorded, not sampled
    assert R.is_recorded(6, 2, True) == (True, True)
    assert [c for c in range(250) if R.is_recorded(c, 100, c == 137)[0]] == [0, 100, 137, 200]


def test_ring_wrap_dropped_and_blame():
    """every=2, capacity=3, seven calls, the one at count 3 skipped: rows at 0, 2, 3 (forced), 4, 6."""
    rec = R.Recorder(tensors=2, capacity=3, every=2)
    w0 = [np.array([1.0]), np.array([2.0, 0.0])]
    for c in range(7):
        w1 = [w + 1.0 for w in w0]
        g = [np.array([float(c)]), np.array([NAN if c in (3, 4) else 1.0, 0.0])]
        assert rec.after(w1, g, w0, skip=c == 3) == (c % 2 == 0 or c == 3, c % 2 == 0)
        if c == 2:
            first = rec.read()
            assert first["steps"].tolist() == [0, 2] and first["dropped"] == 0 and first["count"] == 3
            assert first["grad_norm"][:, 0].tolist() == [0.0, 2.0] and first["first_bad_step"] == -1
    assert (rec.count, rec.rows) == (7, 5)
    out = rec.read()
    assert out["steps"].tolist() == [3, 4, 6] and out["dropped"] == 0                    # rows 0 and 2 were read before they were overwritten
    assert out["update_norm"][:, 0].tolist() == [0.0, 1.0, 1.0]                          # the forced row does not read the shadow
    assert out["grad_nonfinite"][:, 1].tolist() == [1.0, 1.0, 0.0]
    assert (out["first_bad_step"], out["first_bad_tensor"]) == (3, 1)                    # set by the first such row, kept by the second
    assert rec.read()["steps"].tolist() == []
    late = R.Recorder(tensors=2, capacity=3, every=2)
    for c in range(7):
        late.after(w0, [np.array([INF]), np.array([INF, 0.0])], w0, skip=c == 3)
    out = late.read()
    assert out["steps"].tolist() == [3, 4, 6] and out["dropped"] == 2                    # never read: rows 0 and 2 are gone
    assert (out["first_bad_step"], out["first_bad_tensor"]) == (0, 0)                    # two tensors at once: the lower index


def test_one_ulp_bar():
    x = np.float32(1.0)
    up, up2 = np.nextafter(x, np.float32(2)), np.nextafter(np.nextafter(x, np.float32(2)), np.float32(2))
    assert R.within_one_ulp([x, up, NAN, 0.0], [1.0, 1.0, NAN, 0.0]).all()
    assert not R.within_one_ulp([up2], [1.0]).any() and not R.within_one_ulp([NAN], [1.0]).any() and not R.within_one_ulp([1.0], [NAN]).any()


def test_param_stats_host_side():
    """The feature's surface that needs no device: the class, the typed entry points, the sizes, the refusals in front of any launch."""
    import torch
    from mcquic_amd import _lib, monitor
    lib = _lib.load()
    assert lib.mcq_param_stats_columns() == len(R.COLUMNS) == len(monitor.STAT_COLUMNS) and tuple(monitor.STAT_COLUMNS) == R.COLUMNS
    assert lib.mcq_param_stats_workspace_bytes(0, 3) == 0 and lib.mcq_param_stats_workspace_bytes(3, 0) == 0
    assert lib.mcq_param_stats_workspace_bytes(7, 3) >= 7 * 5 * 8 and lib.mcq_param_stats_workspace_bytes(7, 3) % 8 == 0
    assert lib.mcq_param_stats_before_f32(None, 1, None, None, None, 1, None, 1, None) == _lib.MCQ_EINVAL
    assert lib.mcq_param_stats_after_f32(None, 1, None, None, None, 1, None, 1, 1, 1, None, None, None) == _lib.MCQ_EINVAL
    assert lib.mcq_param_stats_finish_f32(None, None, 1, 1, None, 1, None, None, None, None) == _lib.MCQ_EINVAL
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        monitor.ParamStats([torch.zeros(4)])
