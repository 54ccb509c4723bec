"""CPU: the oracle against the REAL reference, through the reference's side recorded on these very seeds (tests/golden/
f16_reference_direct.npz, f16b_*, f16c_*, made by tests/golden/make_golden.py from the reference imported unmodified): state_dict
layouts and codes exactly; decoded tensors whole, bit-equal on the host they were recorded on and within the tolerances of the
other golden comparisons elsewhere (another host's CPU kernels sum float32 in another order: the same oracle's decode differs in
its last bits between an Intel and an AMD EPYC host); the validation handlers' results."""
import os

import numpy as np
import pytest
import torch

from oracle import mcquic_ref as R

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F16 = os.path.join(G, "f16_reference_direct.npz")


def _z():
    return np.load(F16)


def _tree(z, prefix):
    """The reference's state_dict as recorded: ordered names -> shapes."""
    return {str(k): tuple(int(d) for d in s if d >= 0) for k, s in zip(z[prefix + "_keys"], z[prefix + "_shapes"])}


def _close(t, want, name, tol=1e-6):
    """A float output against the whole recorded tensor: the same shape, every value within `tol` (0 on the host the vectors
    were recorded on; the float32 summation order of another host's CPU kernels moves the last bits)."""
    assert tuple(t.shape) == want.shape, name
    np.testing.assert_allclose(t.numpy(), want, rtol=0, atol=tol, err_msg=name)


def test_state_dict_layout_is_the_references():
    sd = R.make_state_dict(8, 2, [32, 16, 8], seed=3)
    ref = _tree(_z(), "compressor")
    assert set(sd) == set(ref) and len(ref) == 718
    for k in ref:
        assert tuple(sd[k].shape) == ref[k], k


def test_encode_decode_bit_equal_to_reference():
    z = _z()
    sd = R.make_state_dict(8, 2, [32, 16, 8], seed=3)
    x = R.make_images(2, 130, 250, seed=9)
    oc = R.encode(sd, x)
    assert len(oc) == 3
    for lv, b in enumerate(oc):
        assert torch.equal(torch.from_numpy(z[f"compressor_code{lv}"]), b)
    want = np.stack([np.load(os.path.join(G, f"f16b_compressor_decode_{i}.npz"))["dec"] for i in range(2)])
    _close(R.decode(sd, oc), want, "compressor_dec")


def test_hip_module_tree_matches_reference_keys():
    from mcquic_amd import Compressor
    ref = _tree(_z(), "compressor")
    mine = Compressor(8, 2, [32, 16, 8]).state_dict()
    assert list(mine.keys()) == list(ref.keys())
    for k in ref:
        assert tuple(mine[k].shape) == ref[k], k


def test_metrics_oracle_against_reference_handlers():
    """oracle/metrics_ref.py against the reference's MsSSIM / PSNR / IdealBPP handlers' results on the same seeds."""
    from oracle import metrics_ref as M
    z = _z()
    x, y = M.make_u8_pair(901, 2, 211, 180)
    want_db = torch.from_numpy(z["msssim_db"])
    assert torch.allclose(M.ms_ssim_db(M.ms_ssim(x, y)), want_db, atol=2e-3)
    assert torch.allclose(M.psnr_u8(x, y), torch.from_numpy(z["psnr"]), rtol=1e-14, atol=0)
    ks = list(M.CODE_BATCH_KS)
    hist = [torch.zeros(2, k) for k in ks]
    count = [torch.zeros(2) for _ in ks]
    for codes in M.make_code_batches(seed=5, batches=3):
        for lv, (c, k) in enumerate(zip(codes, ks)):
            for g in range(2):
                hist[lv][g] += torch.bincount(c[:, g].flatten(), minlength=k)
                count[lv][g] += c[:, g].numel()
    result = float(z["ideal_bpp"][0])
    assert abs(M.ideal_bpp(hist, count, 3 * 3 * 768 * 512) - result) <= 1e-6 * result


@pytest.mark.parametrize("dense", [False, True], ids=["plain", "denseNorm"])
def test_neon_oracle_bit_equal_to_reference(dense):
    """oracle/neon_ref.py against the reference's Neon / ResidualBackwardQuantizer: state_dict layout, encode,
    decode, residual_backward, residual_forward; with denseNorm=True (nn.GroupNorm(groups, C) in place of the ResidualBlocks'
    second activation, mcquic/nn/blocks.py:179-200; 32 groups need a width that is a multiple of 32)."""
    from oracle import neon_ref as N
    z = _z()
    tag = "denseNorm" if dense else "plain"
    ch, k, size = (32 if dense else 16), 64, [4, 2, 2]
    sd = N.make_state_dict(ch, k, size, seed=11, denseNorm=dense)
    ref = _tree(z, "neon_" + tag)
    assert set(sd) == set(ref)
    for key in ref:
        assert tuple(sd[key].shape) == ref[key], key
    x = R.make_images(2, 64, 64, seed=12)
    oc = N.encode(sd, x)
    assert len(oc) == 3
    assert all(torch.equal(torch.from_numpy(z[f"neon_{tag}_code{lv}"]), b) for lv, b in enumerate(oc))
    # (GroupNorm amplifies the host's float32 summation order: tests/test_neon.py's tolerances for the same oracle)
    tol = 5e-5 if dense else 1e-6
    out = np.load(os.path.join(G, "f16c_neon_outputs.npz"))
    _close(N.decode(sd, oc), out[f"neon_{tag}_dec"], f"neon_{tag}_dec", tol)
    _close(N.residual_backward(sd, oc[1], 2), out[f"neon_{tag}_rb"], f"neon_{tag}_rb", tol)
    _close(N.residual_forward(sd, oc[1], N.residual_forward(sd, oc[0], None, 0), 1), out[f"neon_{tag}_rf"], f"neon_{tag}_rf", tol)


def test_hip_neon_dense_norm_module_tree_matches_reference_keys():
    from mcquic_amd import Neon
    ref = _tree(_z(), "neon_tree_denseNorm")
    mine = Neon(32, 256, [8, 4, 2, 2], True).state_dict()
    assert list(mine) == list(ref)
    assert all(tuple(mine[k].shape) == ref[k] for k in ref)


def test_hip_neon_module_tree_matches_reference_keys():
    from mcquic_amd import Neon
    ref = _tree(_z(), "neon_tree_plain")
    mine = Neon(32, 256, [8, 4, 2, 2]).state_dict()
    assert list(mine.keys()) == list(ref.keys()) and len(ref) == 819
    for key in ref:
        assert tuple(mine[key].shape) == ref[key], key
