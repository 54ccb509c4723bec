"""validate(..., bits="estimated"): the PSNR and MS-SSIM columns equal those of bits="coded" bit for bit (the coder is lossless: both
paths restore from the same codes), and the bpp column is lower by no more than `levels` times the interval of
tests/test_gpu_code_bits_vs_coder.py per image, over the pixel count."""
import pytest
import torch

from test_gpu_code_bits_vs_coder import small_model, stream_minus_estimate_interval

pytestmark = pytest.mark.gpu


def _compare(dev, n, h, w, msssim):
    from mcquic_amd import validate as V
    model = small_model(dev)
    x = (torch.rand((n, 3, h, w), generator=torch.Generator().manual_seed(h)) * 2 - 1).to(dev)
    coded = V.validate(model, x, msssim=msssim, gather=False)
    est = V.validate(model, x, msssim=msssim, gather=False, bits="estimated")
    assert coded.dtype == est.dtype == torch.float64 and tuple(est.shape) == (n, 3)
    assert torch.equal(coded[:, 0], est[:, 0])
    if msssim:
        assert torch.equal(coded[:, 1], est[:, 1])
    else:
        assert bool(torch.isnan(coded[:, 1]).all()) and bool(torch.isnan(est[:, 1]).all())
    codes = model.encode(x)
    low = sum(stream_minus_estimate_interval(c[0].numel())[0] for c in codes)
    high = sum(stream_minus_estimate_interval(c[0].numel())[1] for c in codes)
    gap = ((coded[:, 2] - est[:, 2]) * (h * w)).cpu()
    print(f"{h}x{w}: coded bpp {coded[:, 2].tolist()}, estimated {est[:, 2].tolist()}, gap {gap.tolist()} bits in [{low:.3f}, {high:.3f}]")
    assert bool((gap >= low - 1e-9).all()) and bool((gap <= high + 1e-9).all())
    assert bool((est[:, 2] > 0).all())


def test_estimated_equals_coded_with_ms_ssim(dev):
    _compare(dev, 2, 176, 208, True)


def test_estimated_equals_coded_on_a_small_image(dev):
    _compare(dev, 3, 64, 48, False)


def test_the_mode_is_checked(dev):
    from mcquic_amd import validate as V
    with pytest.raises(ValueError):
        V.validate(small_model(dev), torch.zeros((1, 3, 64, 48), device=dev), bits="ideal")
