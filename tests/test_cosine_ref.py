"""CPU: the float64 reference of the codebook cosine regulariser (tests/_cosine_ref.py) against torch autograd of the literal
formula, a hand case with exact-zero and negative cosines and the fixture of the real reference's BasicRate (F18); loss.BasicRate,
Rate / Distortion and step_loss(rate=...) on CPU tensors; the new entry points' argument checks."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _cosine_ref as R
from mcquic_amd import loss as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F18 = np.load(os.path.join(ROOT, "tests", "golden", "f18_basic_rate.npz"))
CASES = [tuple(int(v) for v in row) for row in F18["cases"]]
GAMMA = float(F18["gamma"][0])

# e0, e1, (-1, 0, 1, 0), (1, 1, 0, 0): cos(0,1) = 0 exactly, cos(0,2) < 0, cos(0,3) = cos(1,3) = 1/sqrt 2, cos(1,2) = 0, cos(2,3) < 0
FOUR = torch.tensor([[[1.0, 0, 0, 0], [0, 1.0, 0, 0], [-1.0, 0, 1.0, 0], [1.0, 1.0, 0, 0]]])


def _autograd64(cb):
    c = cb.double().clone().requires_grad_()
    loss = R.torch_formula(c)
    loss.backward()
    return float(loss.detach()), c.grad


@pytest.mark.parametrize("k,d", [(7, 3), (33, 16), (130, 64)])
def test_reference_matches_autograd_of_the_formula(k, d):
    cb = R.make_codebook(2, k, d, 3)
    loss, grad = _autograd64(cb)
    ref = R.cosine_ref(cb, chunk=32)                            # (several chunks, the last one ragged)
    assert abs(ref.loss - loss) <= 1e-13 * abs(loss)
    assert float((ref.grad - grad).abs().max()) <= 1e-13 * float(grad.abs().max())


def test_exact_zero_passes_gradient_and_negative_does_not():
    loss, grad = _autograd64(FOUR)
    ref = R.cosine_ref(FOUR)
    r = 1 / np.sqrt(2.0)
    assert abs(ref.loss - 2 * r) < 1e-15 and abs(loss - 2 * r) < 1e-15
    assert float((ref.grad - grad).abs().max()) < 1e-15
    # row 0 (e0): pair (0, 1), cos 0, passes c_1 / s = e1; pair (0, 2), cos -1/sqrt 2, passes nothing; pair (0, 3) passes
    # c_3 / sqrt 2 - (1/sqrt 2) e0
    f64 = dict(dtype=torch.float64)
    want0 = torch.tensor([0.0, 1.0, 0, 0], **f64) + torch.tensor([r, r, 0, 0], **f64) - r * torch.tensor([1.0, 0, 0, 0], **f64)
    assert float((ref.grad[0, 0] - want0).abs().max()) < 1e-15
    assert ref.grad[0, 0, 2] == 0                               # nothing of c_2 = (-1, 0, 1, 0) arrives: its cosine is negative
    # the two exact zeros are inside every tau: they are the ambiguous pairs
    assert sorted(map(tuple, ref.pairs[0].tolist())) == [(0, 1), (1, 2)]


def test_tau_and_the_small_shapes_have_no_ambiguous_pair():
    assert R.tau(64) == 2 * 68 * 2.0 ** -24
    for m, k, d, seed, _ in CASES[:7]:
        ref = R.cosine_ref(R.make_codebook(m, k, d, seed), want_grad=False)
        assert ref.n_ambiguous == 0 and ref.ambiguous_rows == 0.0, (m, k, d, seed)


@pytest.mark.parametrize("i", range(9))
def test_reference_matches_the_real_basic_rate(i):
    m, k, d, seed, _ = CASES[i]
    ref = R.cosine_ref(R.make_codebook(m, k, d, seed))
    loss64 = float(F18[f"loss64_{i}"][0])
    assert abs(GAMMA * ref.loss - loss64) <= 1e-13 * max(abs(loss64), 1e-300)
    rows = torch.from_numpy(F18[f"rows64_{i}"])
    got = GAMMA * ref.grad[0, :rows.shape[0]]
    assert float((got - rows).abs().max()) <= 1e-13 * max(float(rows.abs().max()), 1e-300)


@pytest.mark.parametrize("i", [1, 2, 5, 8])
def test_basic_rate_on_cpu_tensors(i):
    m, k, d, seed, _ = CASES[i]
    cb = R.make_codebook(m, k, d, seed).requires_grad_()
    half = R.make_codebook(m, k, d, seed)[:, : max(2, k // 2)].clone().requires_grad_()       # a second level: the sum over levels
    rate = L.BasicRate(GAMMA)
    loss = rate(None, [cb])
    loss.backward()
    # float32 on the CPU is the reference's own formula: its recorded value within a few ulp (the BLAS under it may differ)
    assert abs(float(loss.detach()) - float(F18[f"loss32_{i}"][0])) <= 4 * 2.0 ** -23 * abs(float(F18[f"loss64_{i}"][0]))
    rows = torch.from_numpy(F18[f"rows64_{i}"]).float()
    assert float((cb.grad[0, :rows.shape[0]] - rows).abs().max()) <= 1e-5 * float(rows.abs().max())
    both = L.BasicRate(GAMMA)(None, [cb.detach(), half]).detach()
    want = GAMMA * (R.cosine_ref(cb).loss + R.cosine_ref(half).loss)
    assert abs(float(both) - want) <= 1e-6 * want
    c64 = cb.detach().double().requires_grad_()
    l64 = rate(None, [c64])
    l64 = l64.detach()
    assert l64.dtype == torch.float64 and abs(float(l64) - float(F18[f"loss64_{i}"][0])) <= 1e-13 * abs(float(l64))


def test_gamma_zero_is_a_plain_zero():
    cb = R.make_codebook(1, 5, 3, 0).requires_grad_()
    zero_row = torch.zeros(1, 4, 3, requires_grad=True)         # the reference would return NaN here: the documented shortcut
    out = L.BasicRate()(None, [cb, zero_row])
    assert out.dim() == 0 and float(out) == 0.0 and not out.requires_grad
    assert L.BasicRate(0.0)(None, []).dim() == 0
    assert torch.isnan(L.BasicRate(1.0)(None, [zero_row]))      # with a weight the zero codeword shows


def test_rate_and_distortion_formatters():
    rate = L.Rate(L.Decibel(2.0))
    dist = L.Distortion(L.Decibel(1.0))
    x = torch.tensor(0.01)
    assert torch.allclose(rate.formatRate(x), -10 * (x / 4).log10())
    assert torch.allclose(dist.formatDistortion(x), -10 * x.log10())
    b = L.BasicRate(0.5)
    assert isinstance(b, L.Rate) and b.formatRate(x) is x        # nn.Identity
    for name in ("BasicRate", "Rate", "Distortion", "MsSSIM", "PSNR", "step_loss"):
        assert name in L.__all__


def test_step_loss_rate_needs_the_model_and_marks_its_loss_fn():
    with pytest.raises(ValueError, match="model"):
        L.step_loss(rate=L.BasicRate(0.1))
    assert not hasattr(L.step_loss(), "single_segment")

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.cb = torch.nn.Parameter(R.make_codebook(2, 9, 4, 0))

        @property
        def Codebooks(self):
            return [self.cb]

    model = Model()
    fn = L.step_loss(L.PSNR(), rate=L.BasicRate(0.5), model=model)
    assert fn.single_segment is True
    xh, x = torch.rand(1, 3, 8, 8, requires_grad=True), torch.rand(1, 3, 8, 8)
    out = fn((xh, None, None, None), x)
    plain = L.step_loss(L.PSNR())((xh, None, None, None), x)
    want = float(plain.detach()) + 0.5 * R.cosine_ref(model.cb).loss
    assert abs(float(out.detach()) - want) <= 1e-6 * want
    out.backward()
    assert float((model.cb.grad.double() - 0.5 * R.cosine_ref(model.cb).grad).abs().max()) <= 1e-5


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from mcquic_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "mcquic_hip.h")).read()
    assert int(re.search(r"#define\s+MCQ_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.ABI_VERSION >= 13
    for name in ("mcq_codebook_cos_workspace", "mcq_codebook_cos_f32", "mcq_codebook_cos_bwd_f32"):
        assert name in _lib.SYMBOLS and re.search(r"\b%s\s*\(" % name, header)
    E = _lib.MCQ_EINVAL
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)                                   # never dereferenced: every call below is refused
    for bad in [(0, 4, 4), (1, 0, 4), (1, 4, 0), (1, 4, 257), (-1, 4, 4)]:
        assert lib.mcq_codebook_cos_workspace(*bad) == 0
        assert lib.mcq_codebook_cos_f32(p, p, p, *bad, None) == E
        assert lib.mcq_codebook_cos_bwd_f32(p, p, 1.0, p, p, *bad, None) == E
    for i in range(3):
        assert lib.mcq_codebook_cos_f32(*[None if j == i else p for j in range(3)], 1, 4, 4, None) == E
    for i in range(4):
        a = [None if j == i else p for j in range(4)]
        assert lib.mcq_codebook_cos_bwd_f32(a[0], a[1], 1.0, a[2], a[3], 1, 4, 4, None) == E
    # O(m k): per-workgroup double partials and two floats per codeword
    assert lib.mcq_codebook_cos_workspace(2, 8192, 64) == 2 * 256 * 8 + 2 * 2 * 8192 * 4
    assert lib.mcq_codebook_cos_workspace(1, 1, 256) == 8 + 8
    with pytest.raises(RuntimeError, match="HIP device"):
        from mcquic_amd import ops
        ops.codebook_cosine(torch.zeros(1, 4, 4))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.codebook_cosine_bwd(torch.zeros(1, 4, 4), torch.ones(()), 1.0)
