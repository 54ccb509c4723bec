"""mcq_code_image_u8 / mcq_code_image_first_u8 (csrc/step_snapshot.hip): bit-equal to `Validator.visualizeIntermediate` evaluated by torch on
the CPU (tests/_snapshot_ref.py::code_image, pinned to the reference's expression by tests/test_snapshot_ref.py)."""
import pytest
import torch
import torch.nn.functional as F

import _snapshot_ref as R

pytestmark = pytest.mark.gpu


def _codes(shape, top, seed=3):
    g = torch.Generator().manual_seed(seed)
    codes = torch.randint(0, top + 1, shape, generator=g)
    codes.view(-1)[-1] = top
    if shape[1] > 1:
        codes[:, 0].clamp_(max=top // 2)                       # the maximum lives in group 1: a group-0 maximum gives another image
    return codes


@pytest.mark.parametrize("shape,top", [((1, 1, 1, 1), 5), ((2, 2, 3, 5), 100), ((3, 2, 16, 16), 8191), ((5, 2, 7, 9), 511)])
def test_code_image_is_visualize_intermediate(dev, shape, top):
    from mcquic_amd import ops
    codes = _codes(shape, top)
    got = ops.code_image(codes.to(dev))
    want = R.code_image(codes)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (shape[0], 1, 4 * shape[2], 4 * shape[3])
    assert torch.equal(got.cpu(), want)
    assert torch.equal(want, F.interpolate(R.detransform((codes.float() / codes.max() - 0.5) * 2)[:, :1], scale_factor=4, mode="nearest"))
    if shape[1] > 1:
        assert int(codes[:, 0].max()) < int(codes.max())
        assert not torch.equal(got.cpu(), R.code_image(codes[:, :1]))
    if top == 8191:
        assert int(want.max()) >= 127 and int(want.min()) == 0


def test_first_images_only_and_buffers_given(dev):
    """`keep` images of the batch, scaled by the maximum of the WHOLE batch (it sits in the last image here), into buffers the caller owns."""
    from mcquic_amd import ops
    codes = _codes((4, 2, 3, 5), 1000)
    assert int(codes[:2].max()) < 1000
    out = torch.full((2 * 16 * 15 + 4,), 77, dtype=torch.uint8, device=dev)
    maxbuf = torch.zeros(1, dtype=torch.int64, device=dev)
    got = ops.code_image(codes.to(dev), keep=2, out=out[: 2 * 16 * 15], maxbuf=maxbuf)
    assert got.data_ptr() == out.data_ptr() and int(maxbuf) == 1000
    assert torch.equal(got.cpu().view(2, 1, 12, 20), R.code_image(codes, keep=2))
    assert out[2 * 16 * 15:].tolist() == [77] * 4, "nothing is written past the kept images"
    with pytest.raises(ValueError):
        ops.code_image(codes.to(dev), keep=5)
    with pytest.raises(ValueError):
        ops.code_image(codes.to(dev), keep=2, out=out[1: 1 + 2 * 16 * 15])       # not 4-byte aligned


def test_all_zero_codes_give_zero(dev):
    """0 / 0 in the reference (a NaN converted to uint8: unspecified); documented as 0 here."""
    from mcquic_amd import ops
    got = ops.code_image(torch.zeros((2, 2, 3, 5), dtype=torch.int64, device=dev))
    assert got.shape == (2, 1, 12, 20) and int(got.max()) == 0
