"""CPU: the float64 references of the rate-constrained assignment (tests/_rate_ref.py) tested on themselves, the float32 emulation's
mismatch count on the seeds tests/test_gpu_rate_encode.py runs, and the validation of `rd_lambda` (before any device work)."""
import math

import numpy as np
import pytest
import torch

import _rate_ref as RR


def test_lambda_zero_is_the_plain_argmin():
    for (m, k, d) in ((1, 5, 1), (2, 129, 3), (2, 512, 64)):
        x, cb, cdf = RR.make_case(m, k, d, 5, 7)
        bits = RR.penalty_table(cdf)
        v = RR._vectors(x.astype(np.float64), m)
        plain = np.argmin(((v[:, :, None, :] - cb.astype(np.float64)[:, None, :, :]) ** 2).sum(-1), -1)
        assert np.array_equal(RR.penalised_argmin(x, cb, bits, 0.0), RR.codes_of(plain, 2, 5, 7))
        # ... and a real penalty moves codes toward the cheap symbols: fewer bits in total, never more
        heavy = RR.flat_of(RR.penalised_argmin(x, cb, bits, 3.0))
        assert np.take_along_axis(bits, heavy, 1).sum() < np.take_along_axis(bits, plain, 1).sum()


def test_first_index_on_ties():
    cb = np.zeros((1, 4, 2), dtype=np.float32)                     # four identical codewords
    x = np.ones((1, 2, 1, 1), dtype=np.float32)
    bits = np.array([[3.0, 2.0, 2.0, 5.0]])
    assert RR.penalised_argmin(x, cb, bits, 0.0).item() == 0
    assert RR.penalised_argmin(x, cb, bits, 1.0).item() == 1       # 1 and 2 tie: the first


def test_power_of_two_widths_give_exact_penalties():
    widths = np.array([[1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768 + 1]], dtype=np.int64)
    widths[0, -1] = 65536 - widths[0, :-1].sum()                   # = 32769: the one width that is no power of two
    cdf = np.zeros((1, 17), dtype=np.int64)
    cdf[:, 1:] = np.cumsum(widths, -1)
    bits = RR.penalty_table(cdf.astype(np.uint32))
    assert np.array_equal(bits[0, :15], np.arange(16, 1, -1, dtype=np.float64))
    assert bits[0, 15] == 16.0 - math.log2(32769)
    one = np.array([[0, 65536]], dtype=np.uint32)                  # k = 1: the whole range, 0 bits
    assert RR.penalty_table(one)[0, 0] == 0.0
    assert np.isinf(RR.penalty_table(np.array([[0, 7, 7, 65536]], dtype=np.uint32))[0, 1])
    # the float32 norm sequence on exact penalties: c2 + lam * bits with a single rounding each, exactly representable here
    cb = np.full((1, 16, 3), 0.5, dtype=np.float32)
    got = RR.norms_f32(cb, cdf.astype(np.uint32), 0.25)
    assert np.array_equal(got[0, :15], (0.75 + 0.25 * np.arange(16, 1, -1)).astype(np.float32))
    assert np.array_equal(RR.norms_f32(cb, cdf.astype(np.uint32), 0.0), RR.c2_f32(cb))


def test_tables_of_the_cases_are_valid_and_distinct():
    for k in RR.PACK_KS:
        _, _, cdf = RR.make_case(2, k, 3, 1, 1)
        w = np.diff(cdf.astype(np.int64), axis=-1)
        assert cdf.dtype == np.uint32 and (cdf[:, 0] == 0).all() and (cdf[:, -1] == 65536).all() and (w >= 1).all()
        assert all(len(np.unique(row)) > min(k, 64) // 2 for row in w)
    dom = RR.dominant_table(2, 129, 7)
    w = np.diff(dom.astype(np.int64), axis=-1)
    assert (w.sum(-1) == 65536).all() and (np.delete(w, 7, 1) == 1).all()


def test_norm_section_layout_counts():
    for m in RR.PACK_MS:
        for k in RR.PACK_KS:
            g, word, kind = RR.norm_section_layout(m, k)
            ntile = (k + 127) // 128
            assert len(kind) == m * (ntile + 1) * 256
            assert (kind == 0).sum() == m * k and (kind == 2).sum() == len(kind) // 2
            for gi in range(m):
                assert sorted(word[(kind == 0) & (g == gi)]) == list(range(k))


@pytest.mark.parametrize("k", RR.PACK_KS)
@pytest.mark.parametrize("d", RR.PACK_DS)
def test_float32_emulation_stays_under_the_excuse_cap(k, d):
    """The seeds of the GPU assignment test: float32 arithmetic in the kernel's sequence differs from the float64 argmin in at most
    1 % of the positions, and only inside the rounding bound."""
    for m in RR.PACK_MS:
        for (h, w) in RR.MAPS:
            x, cb, cdf = RR.make_case(m, k, d, h, w)
            bits = RR.penalty_table(cdf)
            for lam in RR.LAMBDAS:
                got = RR.emulate_assign_f32(x, cb, RR.norms_f32(cb, cdf, lam))
                differ, unexcused = RR.audit(x, cb, bits, lam, got)
                assert unexcused == 0
                assert differ <= RR.EXCUSED_CAP * got.size, (m, k, d, h, w, lam, differ, got.size)


def test_audit_refuses_a_wrong_code():
    x, cb, cdf = RR.make_case(1, 129, 3, 5, 7)
    bits = RR.penalty_table(cdf)
    want = RR.penalised_argmin(x, cb, bits, 3.0)
    assert RR.audit(x, cb, bits, 3.0, want) == (0, 0)
    wrong = want.copy()
    wrong[0, 0, 0, 0] = (wrong[0, 0, 0, 0] + 64) % 129
    wrong[1, 0, 4, 6] = 129                                        # out of range: never excused
    assert RR.audit(x, cb, bits, 3.0, wrong) == (2, 2)


# ---- rd_lambda is checked on the host, before anything touches a device ---------------------------------------------------------------
def test_rate_lambdas_spreads_and_checks():
    from mcquic_amd.modules.quantizer import rateLambdas
    assert rateLambdas(0.5, 3) == (0.5, 0.5, 0.5) and rateLambdas(0, 2) == (0.0, 0.0)
    assert rateLambdas([0.0, 1, 2.5], 3) == (0.0, 1.0, 2.5)
    # the kernel takes a float32: that rounding is what comes back (and what the caches key on)
    assert rateLambdas((1e30,), 1) == (float(np.float32(1e30)),) and rateLambdas(0.1, 1) == (float(np.float32(0.1)),)
    assert rateLambdas(1e-50, 2) == (0.0, 0.0) and rateLambdas(3.0e38, 1) == (float(np.float32(3.0e38)),)
    assert rateLambdas(torch.tensor(0.25), 2) == (0.25, 0.25)
    for bad in (-1.0, float("nan"), float("inf"), -0.5, 1e39, [0.1, 3.5e38, 0.2], [0.1, 0.2], [0.1, 0.2, 0.3, 0.4], [0.1, -0.2, 0.3], [0.1, float("nan"), 0.3],
                "much", [0.1, None, 0.2], torch.ones(3)):
        with pytest.raises(ValueError):
            rateLambdas(bad, 3)


def test_model_entry_points_refuse_a_bad_rd_lambda_on_the_host():
    """A model on the CPU: every entry point raises ValueError for the lambda before it reaches a kernel (which would refuse the CPU
    tensors with a RuntimeError instead)."""
    from mcquic_amd import Compressor, validate
    model = Compressor(8, 2, [32, 16, 8]).eval()
    x = torch.zeros((1, 3, 128, 128))
    for bad in (-1.0, float("nan"), 1e39, [0.5, 0.5], [0.5, 0.5, 0.5, 0.5]):
        with pytest.raises(ValueError, match="rd_lambda"):
            model.encode(x, rd_lambda=bad)
        with pytest.raises(ValueError, match="rd_lambda"):
            model.compress(x, rd_lambda=bad)
        with pytest.raises(ValueError, match="rd_lambda"):
            model.compress(x, coder="device", rd_lambda=bad)
        with pytest.raises(ValueError, match="rd_lambda"):
            model._quantizer.encode(x, rd_lambda=bad)
        with pytest.raises(ValueError, match="rd_lambda"):
            validate.rate_sweep(model, x, [0.0, bad])
    with pytest.raises(ValueError, match="bits"):
        validate.rate_sweep(model, x, [0.0], bits="coded")
    with pytest.raises(ValueError):
        model.encode_to_rate(x, target_bpp=-1.0)
    with pytest.raises(ValueError):
        model.encode_to_rate(x, target_bpp=0.1, lambda_max=float("inf"))


def test_quantizers_without_tables_refuse():
    from mcquic_amd import Neon
    model = Neon(32, 256, [8, 4, 2, 2]).eval()
    x = torch.zeros((1, 3, 128, 128))
    with pytest.raises(NotImplementedError):
        model.encode(x, rd_lambda=0.5)
    with pytest.raises(NotImplementedError):
        model.compress(x, rd_lambda=0.5)
    with pytest.raises(NotImplementedError):
        model.encode_to_rate(x, 0.1)


def test_pack_entry_refuses_bad_arguments_without_a_device():
    """mcq_vq_pack_codebook_rate_f32 returns MCQ_EINVAL before any launch: NULL pointers, sizes, lambda < 0 / NaN / inf."""
    from mcquic_amd import _lib
    lib = _lib.load()
    f = lib.mcq_vq_pack_codebook_rate_f32
    P = 0x1000                                                     # never dereferenced: every call below is refused first
    assert f(None, P, 0.5, 1, 5, 3, P, None) == _lib.MCQ_EINVAL
    assert f(P, None, 0.5, 1, 5, 3, P, None) == _lib.MCQ_EINVAL
    assert f(P, P, 0.5, 1, 5, 3, None, None) == _lib.MCQ_EINVAL
    for m, k, d in ((0, 5, 3), (1, 0, 3), (1, 5, 0), (-1, 5, 3)):
        assert f(P, P, 0.5, m, k, d, P, None) == _lib.MCQ_EINVAL
    for lam in (-1.0, -1e-30, float("nan"), float("inf"), -float("inf")):
        assert f(P, P, lam, 1, 5, 3, P, None) == _lib.MCQ_EINVAL
    from ctypes import c_float, c_int32, c_void_p
    assert _lib.SYMBOLS["mcq_vq_pack_codebook_rate_f32"] == (c_int32, [c_void_p, c_void_p, c_float, c_int32, c_int32, c_int32, c_void_p, c_void_p])
