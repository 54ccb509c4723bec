"""CPU: the references of tests/_rate_map_ref.py on themselves (the float32 sequence of the per-vector-lambda assignment against the
float64 argmin on the seeds tests/test_gpu_rate_map.py runs, the level maps on hand-worked cases, the per-image search rule on
synthetic curves), the host-side checks of `rd_map` on a CPU model, and the new entry points' refusals without a device."""
import numpy as np
import pytest
import torch

import _rate_map_ref as MR
import _rate_ref as RR


@pytest.mark.parametrize("k", RR.PACK_KS)
@pytest.mark.parametrize("d", RR.PACK_DS)
def test_float32_sequence_stays_under_the_excuse_cap(k, d):
    positions = differ = 0
    for m in RR.PACK_MS:
        for (h, w) in MR.MAPS[:2]:                                   # (9 x 33 adds positions, not paths: the GPU test runs it)
            x, cb, cdf = RR.make_case(m, k, d, h, w)
            bits = RR.penalty_table(cdf)
            for lam in (MR.map_lambdas(2, h, w, k + d), np.asarray([0.25, 3.0], dtype=np.float32)):
                got = MR.emulate_assign_f32(x, cb, cdf, lam)
                dn, unexcused = MR.audit(x, cb, bits, lam, got)
                assert unexcused == 0
                positions += got.size
                differ += dn
    assert differ <= RR.EXCUSED_CAP * positions, (k, d, differ, positions)


def test_zero_lambda_is_the_plain_sequence_and_an_empty_slot_never_wins():
    x, cb, cdf = RR.make_case(2, 129, 3, 5, 7)
    zero = np.zeros((2, 5, 7), dtype=np.float32)
    assert np.array_equal(MR.emulate_assign_f32(x, cb, cdf, zero), RR.emulate_assign_f32(x, cb, RR.c2_f32(cb)))
    assert np.array_equal(MR.argmin_map(x, cb, RR.penalty_table(cdf), zero), RR.penalised_argmin(x, cb, RR.penalty_table(cdf), 0.0))
    plain = RR.flat_of(RR.emulate_assign_f32(x, cb, RR.c2_f32(cb)))
    slot = int(np.bincount(plain[0]).argmax())                       # the most used code of group 0 loses its slot
    cdf = cdf.copy()
    cdf[0, slot + 1:] = np.maximum(cdf[0, slot + 1:], cdf[0, slot]); cdf[0, slot + 1] = cdf[0, slot]
    assert np.isinf(MR.bits_f32(cdf)[0, slot])
    for lam in (zero, zero + np.float32(0.5)):
        assert not (RR.flat_of(MR.emulate_assign_f32(x, cb, cdf, lam))[0] == slot).any()
        assert not (RR.flat_of(MR.argmin_map(x, cb, RR.penalty_table(cdf), lam))[0] == slot).any()


def test_level_maps_by_hand():
    a = np.arange(35, dtype=np.float32).reshape(1, 5, 7)
    (l0, l1, l2), err = MR.level_maps(a, (1.0, 2.0, 0.5))
    assert err.tolist() == [0] and np.array_equal(l0, a) and l1.shape == (1, 3, 4) and l2.shape == (1, 2, 2)
    # 5 x 7 -> 3 x 4: full cells, the one-column right edge, the one-row bottom edge, the single corner cell
    assert l1[0, 0, 0] == 2.0 * (0 + 1 + 7 + 8) / 4 and l1[0, 0, 3] == 2.0 * (6 + 13) / 2
    assert l1[0, 2, 0] == 2.0 * (28 + 29) / 2 and l1[0, 2, 3] == 2.0 * 34
    # 3 x 4 -> 2 x 2 on the UNSCALED level 1
    u1 = l1[0] / 2.0
    assert l2[0, 0, 0] == 0.5 * (u1[0, 0] + u1[0, 1] + u1[1, 0] + u1[1, 1]) / 4 and l2[0, 1, 1] == 0.5 * (u1[2, 2] + u1[2, 3]) / 2
    # bad values count as 0 and mark their image
    b = np.ones((3, 5, 7), dtype=np.float32)
    b[0, 4, 6], b[2, 0, 0], b[2, 1, 1] = np.nan, -1.0, np.inf
    levels, err = MR.level_maps(b, (1.0, 1.0, 1.0))
    assert err.tolist() == [1, 0, 1] and levels[0][0, 4, 6] == 0 and levels[0][2, 0, 0] == 0 and levels[1][2, 0, 0] == 0.5
    assert levels[1][0, 2, 3] == 0 and (levels[2][1] == 1).all()
    # the per-image form just scales
    levels, err = MR.level_maps(np.asarray([0.5, -2.0, 3.0], dtype=np.float32), (1.0, 0.1, 0.0))
    assert err.tolist() == [0, 1, 0] and [l.shape for l in levels] == [(3,)] * 3
    assert np.array_equal(levels[1], (np.float32(0.1) * np.asarray([0.5, 0, 3.0], dtype=np.float32)).astype(np.float32)) and (levels[2] == 0).all()


def test_search_rule_on_monotone_curves():
    curve = lambda lam: 2.0 / (1.0 + 4.0 * lam)                      # noqa: E731
    # the plain codes meet the target
    lam, trace = MR.search(curve, 2.5, 64.0, 12)
    assert lam == 0.0 and len(trace) == 14 and all(t == (0.0, 2.0) for t in trace)
    # unreachable: ends at lambda_max and shows its bpp
    lam, trace = MR.search(curve, 1e-6, 64.0, 12)
    assert lam == 64.0 and trace[1][0] == 64.0 and trace[-1] == (64.0, curve(64.0))
    # in between: sixteenths first, then geometric means; the answer meets the target and is the smallest met lambda visited
    lam, trace = MR.search(curve, 1.0, 64.0, 12)
    # (the curve meets 1.0 exactly at 0.25: 4 and 0.25 meet, 0.25 / 16 misses and becomes the lower end, then geometric means)
    assert [t[0] for t in trace[:6]] == [0.0, 64.0, 4.0, 0.25, 0.015625, float(np.float32(np.sqrt(0.015625 * 0.25)))]
    met = [t[0] for t in trace if t[1] <= 1.0]
    assert curve(lam) <= 1.0 and lam == min(met) == 0.25
    assert all(0.015625 < t[0] < 0.25 for t in trace[5:] if t[0] != lam)
    assert MR.replay([t[1] for t in trace], 1.0, 64.0) == ([t[0] for t in trace], lam)
    # iters = 0: two trials, the answer is lambda_max when it meets
    assert MR.search(curve, 1.0, 64.0, 0)[0] == 64.0
    # a frozen bracket ends the search early and the image rides along
    lam, trace = MR.search(lambda l: 0.0 if l >= 1e-30 else 1.0, 0.5, 1e-30, 40)
    assert lam == trace[-1][0] and trace[-1][0] == trace[-2][0]


def test_rd_map_is_checked_on_the_host_before_anything_runs():
    from mcquic_amd import Compressor
    model = Compressor(8, 2, [32, 16, 8]).eval()
    x = torch.zeros((2, 3, 128, 128))
    assert model._rateGrid(x) == (2, 8, 8) and model._rateGrid(torch.zeros((1, 3, 100, 300))) == (1, 8, 24)
    bad_maps = [torch.zeros(2, dtype=torch.float64), torch.zeros(3), torch.zeros(2, 8), torch.zeros(2, 8, 9), torch.zeros(2, 1, 8, 8),
                [0.0, 0.0], 0.5, torch.zeros(2, device="meta")]
    for bad in bad_maps:
        for call in (lambda m: model.encode(x, rd_map=m), lambda m: model.compress(x, rd_map=m),
                     lambda m: model.compress(x, coder="device", rd_map=m)):
            with pytest.raises(ValueError, match="rd_map"):
                call(bad)
    good = torch.zeros(2)
    for bad in (-1.0, float("nan"), [0.5, 0.5], torch.ones(3)):       # the scale is `rateLambdas`'
        with pytest.raises(ValueError, match="rd_lambda"):
            model.encode(x, rd_lambda=bad, rd_map=good)
        with pytest.raises(ValueError, match="rd_lambda"):
            model.compress(x, rd_lambda=bad, rd_map=good)
    with pytest.raises(ValueError, match="rd_map"):
        model._quantizer.encode(torch.zeros((2, 8, 16, 16)), rd_map=torch.zeros(2, 8, 7))
    for kw in (dict(target_bpp=-1.0), dict(target_bpp=float("nan")), dict(target_bpp=0.1, lambda_max=float("inf")),
               dict(target_bpp=0.1, lambda_max=0.0), dict(target_bpp=0.1, iters=-1), dict(target_bpp=torch.ones(3)),
               dict(target_bpp=torch.ones(2, dtype=torch.int64))):
        with pytest.raises(ValueError):
            model.encode_to_rate(x, per_image=True, **kw)


def test_quantizers_without_tables_refuse_the_new_keywords():
    from mcquic_amd import Neon
    model = Neon(32, 256, [8, 4, 2, 2]).eval()
    x = torch.zeros((1, 3, 128, 128))
    with pytest.raises(NotImplementedError):
        model.encode(x, rd_map=torch.zeros(1))
    with pytest.raises(NotImplementedError):
        model.compress(x, rd_map=torch.zeros(1))
    with pytest.raises(NotImplementedError):
        model.encode_to_rate(x, 0.1, per_image=True)


def test_entry_points_refuse_bad_arguments_without_a_device():
    from ctypes import c_float, c_int32, c_void_p
    from mcquic_amd import _lib
    lib, E, P = _lib.load(), _lib.MCQ_EINVAL, 0x1000                 # P is never dereferenced: every call below is refused first
    assert lib.mcq_packed_bits_floats(2, 129) == 2 * 3 * 256 and lib.mcq_packed_bits_floats(0, 5) == 0
    assert lib.mcq_vq_pack_bits_f32(None, 1, 5, P, None) == E and lib.mcq_vq_pack_bits_f32(P, 1, 5, None, None) == E
    assert lib.mcq_vq_pack_bits_f32(P, 0, 5, P, None) == E and lib.mcq_vq_pack_bits_f32(P, 1, -1, P, None) == E
    f = lib.mcq_vq_assign_rate_map_f32
    ok = [P, P, P, P, 1, 0, 0, P, 2, 1, 3, 5, 7, 5, None, None]
    for i in (0, 1, 2, 3, 7):
        assert f(*[None if j == i else a for j, a in enumerate(ok)]) == E
    for i in (4, 5, 6):
        assert f(*[-1 if j == i else a for j, a in enumerate(ok)]) == E
    for i in range(8, 14):
        assert f(*[0 if j == i else a for j, a in enumerate(ok)]) == E
    f = lib.mcq_rate_map_levels_f32
    sc, outs = (c_float * 3)(1.0, 1.0, 1.0), (c_void_p * 3)(P, P, P)
    ok = [P, 2, 5, 7, 35, 7, 1, sc, None, 3, outs, P, None]
    for i in (0, 7, 10, 11):
        assert f(*[None if j == i else a for j, a in enumerate(ok)]) == E
    for i, v in ((1, 0), (2, -1), (2, 0), (3, 0), (4, -1), (5, -1), (6, -1), (9, 0), (9, 33)):
        assert f(*[v if j == i else a for j, a in enumerate(ok)]) == E
    assert f(*[(c_float * 3)(1.0, -1.0, 1.0) if j == 7 else a for j, a in enumerate(ok)]) == E
    assert f(*[(c_void_p * 3)(P, None, P) if j == 10 else a for j, a in enumerate(ok)]) == E
    f = lib.mcq_rate_search_step
    ok = [P, P, P, P, P, None, None, 2, 3, 16384.0, 64.0, 0, 14, None]
    for i in range(5):
        assert f(*[None if j == i else a for j, a in enumerate(ok)]) == E
    for i, v in ((7, 0), (8, 0), (9, 0.0), (10, 0.0), (10, float("inf")), (10, float("nan")), (11, -1), (11, 15), (12, 1)):
        assert f(*[v if j == i else a for j, a in enumerate(ok)]) == E
    V, I, L, F, D = c_void_p, c_int32, _lib.SYMBOLS["mcq_vq_assign_rate_map_f32"][1][4], c_float, _lib.SYMBOLS["mcq_rate_search_step"][1][9]
    assert _lib.SYMBOLS["mcq_vq_assign_rate_map_f32"] == (I, [V, V, V, V, L, L, L, V, I, I, I, I, I, I, V, V])
    assert _lib.SYMBOLS["mcq_rate_map_levels_f32"] == (I, [V, I, I, I, L, L, L, V, V, I, V, V, V])
    assert _lib.SYMBOLS["mcq_rate_search_step"] == (I, [V, V, V, V, V, V, V, I, I, D, F, I, I, V])
    assert _lib.MCQ_ABI_VERSION == 18
