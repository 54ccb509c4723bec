"""CPU: the references of tests/_metrics_refs.py against the oracle (oracle/metrics_ref.py), torch and the library's host functions,
so that tests/test_gpu_metrics_leaf.py holds the kernels of mcquic_amd/csrc/metrics.hip to something that is itself held.

  maps64     against the oracle's float32 maps, per position: |m32 - m64| <= 48 u E + 8 u, u = 2^-24.  Each of the five blurred
             moments is 11 products and 10 sums a pass, two passes: 42 roundings, each at most u of a partial sum that the blur of the
             magnitudes bounds; the squares / the product of the means and the subtraction add three.  To first order the error of
             cs = (2 s12 + C2) / (s1 + s2 + C2) is then at most 45 u (2 B|xy| + 2 |mu1 mu2| + |cs| (B x^2 + mu1^2 + B y^2 + mu2^2)) / (s1 + s2 + C2)
             =: 45 u E; 48 leaves room for the second order, 8 u for the handful of operations after the moments (and the luminance factor
             of the SSIM map, whose terms do not cancel).  On the seeded image pairs E is about 1e2..1e3: the bar is some 1e-4 where a blur
             with a tap out of place is off by 1e-2 and more (test_maps64_bar_rejects_a_shifted_tap).
  halve64    equal to F.avg_pool2d(kernel 2, stride 2, padding = side % 2, count_include_pad=True) in float64 on integer-valued images
             (every sum exact).
  tile grid  equal to mcq_ssim_tiles and to the per-level sizes of mcq_ms_ssim_workspace_layout (host functions: no GPU).
  combine64  on the oracle's own float32 level means against oracle ms_ssim: five float32 pow (one spacing each), four products, the
             channel sum and one division, all of values in [0, 1]: 2^-20 absolute covers 16 half-spacings of 1."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _metrics_refs as R
from oracle import metrics_ref as M

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
U = 2.0 ** -24
SIDES = (11, 12, 13, 161, 162)


def _planes(t):
    return t.reshape(-1, t.shape[-2], t.shape[-1]).numpy()


def _bar(x, y):
    """48 u E + 8 u per map position (module docstring), from float64 moments."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    mu1, mu2 = R.blur64(x), R.blur64(y)
    bxx, byy, bxy = R.blur64(x * x), R.blur64(y * y), R.blur64(np.abs(x * y))
    den = (bxx - mu1 * mu1) + (byy - mu2 * mu2) + R.C2
    cs = R.maps64(x, y)[1]
    e = (2 * bxy + 2 * np.abs(mu1 * mu2) + np.abs(cs) * (bxx + mu1 * mu1 + byy + mu2 * mu2)) / den
    return 48 * U * e + 8 * U


def _oracle_maps(x, y):
    s, c = M.ssim_and_cs_maps(x.float(), y.float(), M.gauss_window())
    return _planes(s), _planes(c)


def test_window_and_weights_are_the_oracles():
    from mcquic_amd import _lib
    assert R.WIN64.tolist() == M.gauss_window().double().tolist()
    buf = (ctypes.c_float * 11)()
    _lib.load().mcq_ms_ssim_window(buf)
    assert [float(v) for v in buf] == R.WIN64.tolist()
    assert R.LEVEL_W64.tolist() == torch.tensor(M.MS_WEIGHTS).double().tolist()


@pytest.mark.parametrize("h,w", [(27, 129), (43, 247), (11, 11), (161, 175)])
def test_maps64_against_the_oracle(h, w):
    x, y = M.make_u8_pair(h * 1000 + w, 1, h, w)
    s64, c64 = R.maps64(_planes(x), _planes(y))
    s32, c32 = _oracle_maps(x, y)
    assert s64.shape == s32.shape == (3, h - 10, w - 10)
    bar = _bar(_planes(x), _planes(y))
    es, ec = np.abs(s32 - s64), np.abs(c32 - c64)
    print(f"{h}x{w}: worst |ssim32 - ssim64| {es.max():.3e}, |cs32 - cs64| {ec.max():.3e}, smallest bar {bar.min():.3e}, worst share {max((es / bar).max(), (ec / bar).max()):.3f}")
    assert (es <= bar).all() and (ec <= bar).all()
    # the oracle's means are the means of these maps
    ms, mc = M.ssim_and_cs(x.float(), y.float(), M.gauss_window())
    assert np.abs(ms.reshape(-1).numpy() - s64.mean(axis=(1, 2))).max() <= bar.max()
    assert np.abs(mc.reshape(-1).numpy() - c64.mean(axis=(1, 2))).max() <= bar.max()


def test_maps64_bar_rejects_a_shifted_tap():
    """The bar is no formality: the oracle's maps of y moved by one column miss it."""
    x, y = M.make_u8_pair(5, 1, 43, 247)
    s64, c64 = R.maps64(_planes(x), _planes(y))
    s32, c32 = _oracle_maps(x, torch.roll(y, 1, dims=-1))
    bar = _bar(_planes(x), _planes(y))
    assert (np.abs(c32 - c64) > bar).mean() > 0.9 and (np.abs(s32 - s64) > bar).mean() > 0.9


def test_maps64_of_identical_images_is_one():
    x, _ = M.make_u8_pair(9, 1, 30, 140)
    s, c = R.maps64(_planes(x), _planes(x))
    assert np.abs(s - 1).max() <= 1e-12 and np.abs(c - 1).max() <= 1e-12


@pytest.mark.parametrize("h", SIDES)
@pytest.mark.parametrize("w", SIDES)
def test_halve64_is_avg_pool2d(h, w):
    g = torch.Generator().manual_seed(h * 1000 + w)
    x = torch.randint(0, 256, (4, h, w), generator=g, dtype=torch.uint8)
    cur, ref, orc = x.numpy(), x.double(), x.float()
    for level in range(1, 5):
        hh, ww = ref.shape[-2:]
        ref = F.avg_pool2d(ref[None], kernel_size=2, stride=2, padding=(hh % 2, ww % 2), count_include_pad=True)[0]
        cur, orc = R.halve64(cur), M._halve(orc)
        assert cur.shape == tuple(ref.shape) == (4, (hh + 1) // 2, (ww + 1) // 2)
        assert np.array_equal(cur, ref.numpy()), f"level {level}"
        assert np.array_equal(cur, orc.double().numpy()), f"level {level}: the oracle's float32 pooling is not exact"
    assert np.array_equal(R.pyramid64(x.numpy())[4], cur)


def test_tile_grid_and_counts():
    assert (27 - 10, 129 - 10) in [(a, b) for a in R.SEAM_HOS for b in R.SEAM_WOS]      # the seam shape whose last tile is one position
    assert R.tile_grid(17, 119) == (2, 2) and R.tile_counts(17, 119).tolist() == [[16 * 118, 16], [118, 1]]      # H = 27, W = 129
    assert R.tile_grid(16, 118) == (1, 1) and R.tile_grid(1, 1) == (1, 1) and R.tile_grid(33, 237) == (3, 3)
    for ho, wo in ((1, 1), (15, 117), (33, 237), (151, 151), (758, 502)):
        assert R.tile_counts(ho, wo).sum() == ho * wo and R.tile_counts(ho, wo).min() >= 1
    m = np.arange(2 * 40 * 250, dtype=np.float64).reshape(2, 40, 250)
    s = R.tile_sums(m, (33, 237))
    assert s.shape == (2, 3, 3) and s.sum() == m[:, :33, :237].sum() and s[1, 2, 2] == m[1, 32, 236]
    assert R.tile_sums(m).shape == (2, 3, 3) and R.tile_sums(m)[0, 2, 2] == m[0, 32:, 236:].sum()


def test_tile_grid_is_the_librarys():
    """mcq_ssim_tiles and mcq_ms_ssim_workspace_layout (host arithmetic shared with the launcher) against the references' sizes."""
    from mcquic_amd import _lib, ops
    lib = _lib.load()
    for h in list(range(11, 60)) + [137, 138, 139, 161, 768, 2071]:
        for w in (11, 12, 127, 128, 129, 130, 245, 246, 247, 248, 512, 2071):
            assert ops.ssim_tiles(h, w) == R.tile_grid(h - 10, w - 10), (h, w)
    ty, tx = ctypes.c_int32(), ctypes.c_int32()
    assert lib.mcq_ssim_tiles(10, 200, ctypes.byref(ty), ctypes.byref(tx)) == _lib.MCQ_EINVAL
    assert lib.mcq_ssim_tiles(200, 10, ctypes.byref(ty), ctypes.byref(tx)) == _lib.MCQ_EINVAL
    assert lib.mcq_ssim_tiles(200, 200, None, None) == _lib.MCQ_EINVAL
    lay = (ctypes.c_int64 * _lib.MCQ_MS_SSIM_LAYOUT_WORDS)()
    assert lib.mcq_ms_ssim_workspace_layout(1, 3, 160, 161, lay) == _lib.MCQ_EINVAL
    assert lib.mcq_ms_ssim_workspace_layout(1, 3, 161, 161, None) == _lib.MCQ_EINVAL
    for n, c, h, w in ((1, 3, 161, 161), (2, 1, 175, 389), (1, 4, 322, 163), (1, 1, 161, 2071), (32, 3, 768, 512)):
        assert lib.mcq_ms_ssim_workspace_layout(n, c, h, w, lay) == 0
        planes, floats, hl, wl, max_tiles = n * c, 0, h, w, 0
        for l in range(5):
            t = R.tile_grid(hl - 10, wl - 10)
            want_off = (-1, -1) if l == 0 else (floats, floats + planes * hl * wl)
            assert tuple(lay[6 * l: 6 * l + 6]) == (hl, wl) + t + want_off, (n, c, h, w, l)
            floats += 0 if l == 0 else 2 * planes * hl * wl
            max_tiles = max(max_tiles, t[0] * t[1])
            hl, wl = (hl + 1) // 2, (wl + 1) // 2
        assert lay[30] == (4 * floats + 7) // 8 * 8 and lay[31] == lay[30] + planes * max_tiles * 16
        assert lay[32] == lay[31] + 5 * planes * 8 == lib.mcq_ms_ssim_workspace_bytes(n, c, h, w)
    # the stage entry points refuse before any launch
    p = ctypes.c_void_p(256)
    assert lib.mcq_ssim_level_u8(p, p, 1, 10, 11, p, None) == _lib.MCQ_EINVAL and lib.mcq_ssim_level_f32(p, p, 0, 11, 11, p, None) == _lib.MCQ_EINVAL
    assert lib.mcq_ssim_level_u8(p, p, 65536, 11, 11, p, None) == _lib.MCQ_ETOOLARGE and lib.mcq_ssim_level_f32(None, p, 1, 11, 11, p, None) == _lib.MCQ_EINVAL
    assert lib.mcq_ms_ssim_halve_u8(p, p, p, None, 1, 11, 11, None) == _lib.MCQ_EINVAL and lib.mcq_ms_ssim_halve_f32(p, p, p, p, 1, 0, 11, None) == _lib.MCQ_EINVAL
    assert lib.mcq_ms_ssim_combine_f32(p, 0, 3, p, None) == _lib.MCQ_EINVAL and lib.mcq_ms_ssim_combine_f32(None, 1, 3, p, None) == _lib.MCQ_EINVAL


def _oracle_level_table(x, y):
    """[5, N, C, 2] float32: the oracle's own per-level means along its own pyramid."""
    x, y, win, rows = x.float(), y.float(), M.gauss_window(), []
    for lv in range(5):
        s, c = M.ssim_and_cs(x, y, win)
        rows.append(torch.stack([s, c], dim=-1))
        if lv < 4:
            x, y = M._halve(x), M._halve(y)
    return torch.stack(rows).numpy()


def test_combine64_against_the_oracle_on_the_golden_cases():
    z = np.load(os.path.join(G, "f7_metrics.npz"))
    for i, (seed, n, h, w) in enumerate(z["cases"].tolist()):
        x, y = M.make_u8_pair(seed, n, h, w)
        got = R.combine64(_oracle_level_table(x, y))
        assert got.shape == (n,)
        np.testing.assert_allclose(got, M.ms_ssim(x, y).double().numpy(), rtol=0, atol=2.0 ** -20)
        np.testing.assert_allclose(got, z[f"msssim_{i}"], rtol=0, atol=5e-6)


def test_combine64_relu_zero_and_column_choice():
    t = np.full((5, 2, 2, 2), 0.5)
    t[:4, :, :, 0] = -7.0                 # the SSIM column of levels 0..3 and the CS column of the last are not read
    t[4, :, :, 1] = -7.0
    assert np.allclose(R.combine64(t), 0.5 ** R.LEVEL_W64.sum(), rtol=1e-15, atol=0)
    t[2, 1, 0, 1] = -0.25                 # a negative CS mean: that channel's product is 0, the mean halves
    assert R.combine64(t)[1] == 0.5 * R.combine64(t)[0]
    t[4, 1, 1, 0] = 0.0
    assert R.combine64(t)[1] == 0.0
