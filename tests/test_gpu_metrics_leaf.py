"""GPU: the kernels of the validation metric (mcquic_amd/csrc/metrics.hip) one stage at a time against tests/_metrics_refs.py (float64
from the definitions, held on the CPU by tests/test_metrics_refs.py), through the stage entry points, which launch by the code
mcq_ms_ssim_u8 launches by.  The final MS-SSIM value that tests/test_gpu_metrics.py compares is a poor witness: level 0 enters it as
relu(cs)^0.0448, so a whole seam column of a 768 x 512 image wrong by 0.01 moves it by 9e-7, under that file's 2e-6.

  level    ssim_level_kernel, per 16 x 118 map tile: S the kernel's float64 sum of a map over the tile, S64 = tile_sums(maps64) the
           truth, S32 = tile_sums of the oracle's float32 maps (the float32 restatement), n the tile's valid positions.
           (1) e = |S - S64| / n:  e_hip <= max(4 e_ref, 2^-23), e_ref the same distance of S32.  The float32 maps carry the
               cancellation E[x^2] - mu^2 (some 1e-5 on textured images, tests/test_metrics_refs.py), which is why the bar scales with
               the restatement's own error; 2^-23 is one float32 spacing of map values in [1, 2).
           (2) |S - S32| <= n 2^-23: the kernel's header claims the oracle's operations in the oracle's order, so every map value is
               the oracle's float32 and only the order of the float64 sums differs (n 2^-53 relative); one spacing per position is
               the most a different-but-correct rounding could give and far less than a tap out of place.
           Shapes: every (H - 10, W - 10) of {1, 15, 16, 17, 33} x {1, 117, 118, 119, 237} (one ragged row / column, exact multiples, a
           second and third tile; 27 x 129 has a last tile of ONE valid position), 1 and 3 planes, uint8 and float32 input.
           Impulses: x == y but for one pixel; every tile outside its 11 x 11 footprint must return exactly n for both sums.
  halve    exact: pooled values of level l are multiples of 4^-l below 256 (at most 8 + 8 bits), every sum of four is exact in float32,
           so the outputs equal halve64 bit for bit; guard words behind both outputs.
  finish   the level table of a full mcq_ms_ssim_u8 call: the float32 of (the level kernel's tile sums of the pooled images it left in
           the workspace, added in tile order) / count, bit for bit; and held to the means of maps64 by rule (1).
  combine  injected tables against combine64 by rule (1) with e_ref from the same formula in torch float32; relu'd products exactly 0.
  sqdiff   exact against int64 sums around the 16-byte vector path, the 16384-byte chunk and a misaligned base.

Measured on an MI355X (profiles/r16_metrics_leaf_errors.json, keys metrics_leaf[...]): level -- on all 50 seam shapes e_hip / e_ref is
1.0000 and |S - S32| is 0: the kernel's map values are the oracle's float32 bits (the float64 sums of like-sized float32 values are
exact in either order), the header's claim holds; the largest e_hip, 1.3e-4, is float32's own on the 0 / 255 checkerboard.  halve,
sqdiff, the finish restatement and the impulses' untouched tiles: exact.  Level table: e_hip 2.0e-7 .. 1.6e-5, at most 1.18 e_ref
where above the floor (its own float32 rounding).  combine: e_hip 0.9e-8 .. 6.4e-8 next to e_ref 0.6e-8 .. 6.4e-8.  No kernel needed a
change.  Three temporary wrong-value mutations of the kernels (a shifted tap in the last tile column, pooling that ignores the parity
of H, the CS column read on the last level) fail 60, 29 and 7 of the tests here; tests/test_gpu_metrics.py passes the last one whole."""
import ctypes

import numpy as np
import pytest
import torch

import _metrics_refs as R
from _record import record
from oracle import metrics_ref as M

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -23
GUARD = 4096                    # words behind (and in front of) an output
SENTINEL = 7.5
HOS, WOS = R.SEAM_HOS, R.SEAM_WOS       # 27 x 129 among them (tests/test_metrics_refs.py)


# ---- helpers ----------------------------------------------------------------------------------------------------------------------------
def _sync(what):
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:                       # a device fault: nothing more of this session may touch the GPU
        pytest.exit(f"{what}: {e}", returncode=3)


def _level(dev, x, y):
    """One mcq_ssim_level_* launch on x, y [P, H, W] (CPU uint8 or float32) into a NaN-filled buffer of exactly the tile grid's size
    between two guard bands -> float64 [P, tiles_y, tiles_x, 2] on the CPU."""
    from mcquic_amd import _lib, ops
    lib = _lib.load()
    p, h, w = x.shape
    ty, tx = ops.ssim_tiles(h, w)
    assert (ty, tx) == R.tile_grid(h - 10, w - 10)
    n = p * ty * tx * 2
    buf = torch.full((2 * GUARD + n,), SENTINEL, dtype=torch.float64, device=dev)
    out = buf[GUARD:GUARD + n]
    out.fill_(float("nan"))
    xd, yd = x.contiguous().to(dev), y.contiguous().to(dev)
    fn = lib.mcq_ssim_level_u8 if x.dtype == torch.uint8 else lib.mcq_ssim_level_f32
    rc = fn(xd.data_ptr(), yd.data_ptr(), p, h, w, out.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    _sync(f"ssim_level {tuple(x.shape)} {x.dtype}")
    assert rc == 0
    assert bool((buf[:GUARD] == SENTINEL).all() & (buf[GUARD + n:] == SENTINEL).all()), "a tile past the grid of mcq_ssim_tiles was written"
    assert torch.equal(xd.cpu(), x) and torch.equal(yd.cpu(), y)
    got = out.cpu().view(p, ty, tx, 2).numpy()
    assert np.isfinite(got).all(), "a tile sum left unwritten or non-finite"
    return got


def _truth(x, y):
    """(S64, S32) [P, ty, tx, 2] of x, y [P, H, W]: tile sums of maps64 and of the oracle's float32 maps."""
    s64, c64 = R.maps64(x.numpy(), y.numpy())
    s32, c32 = M.ssim_and_cs_maps(x.float()[None], y.float()[None], M.gauss_window())
    return (np.stack([R.tile_sums(s64), R.tile_sums(c64)], axis=-1),
            np.stack([R.tile_sums(s32[0].numpy()), R.tile_sums(c32[0].numpy())], axis=-1))


def _hold(got, s64, s32, counts, what):
    """Rules (1) and (2) per tile and sum; -> (worst e_hip / e_ref over the tiles where e_ref > 0, worst e_hip, worst |S - S32| / n)."""
    n = counts[None, :, :, None]
    e_hip, e_ref, d32 = np.abs(got - s64) / n, np.abs(s32 - s64) / n, np.abs(got - s32) / n
    pos = e_ref > 0
    ratio = float((e_hip[pos] / e_ref[pos]).max()) if pos.any() else 0.0
    bad1, bad2 = e_hip > np.maximum(4 * e_ref, FLOOR), d32 > FLOOR
    assert not bad1.any(), (f"{what}: tiles (plane, row, column, ssim|cs) {np.argwhere(bad1)[:8].tolist()} miss the truth: e_hip "
                            f"{e_hip[bad1][:8]}, e_ref {e_ref[bad1][:8]}")
    assert not bad2.any(), (f"{what}: tiles {np.argwhere(bad2)[:8].tolist()} are not the float32 restatement's: |S - S32| / n "
                            f"{d32[bad2][:8]} > 2^-23")
    return ratio, float(e_hip.max()), float(d32.max())


def _noise(seed, planes, h, w):
    x, y = M.make_u8_pair(seed, 1, h, w)
    return x[0, :planes].contiguous(), y[0, :planes].contiguous()


def _level_inputs(planes, h, w, floats):
    """{name: (x, y)} [planes, h, w] uint8 (float32 when `floats`, then with the pooled-looking pair)."""
    rr, cc = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    flat = torch.tensor([128, 7, 254][:planes], dtype=torch.uint8).view(-1, 1, 1).expand(planes, h, w).contiguous()
    board = torch.from_numpy(np.stack([(((rr // k + cc // k) & 1) * 255).astype(np.uint8) for k in (1, 2, 3)][:planes]))
    ends = torch.zeros((planes, h, w), dtype=torch.uint8)
    ends[1::2] = 255                                  # plane 1: 255 against 0
    cases = dict(noise=_noise(h * 1000 + w, planes, h, w), flat=(flat, flat + 1), board=(board, 255 - board), ends=(ends, 255 - ends))
    if floats:
        cases = {k: (a.float(), b.float()) for k, (a, b) in cases.items()}
        g = torch.Generator().manual_seed(h * 1000 + w)
        cases["pooled"] = tuple(torch.randint(0, 255 * 16 + 1, (planes, h, w), generator=g).float() / 16 for _ in range(2))
    return cases


# ---- the level kernel ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["u8", "f32"])
@pytest.mark.parametrize("wo", WOS)
@pytest.mark.parametrize("ho", HOS)
def test_level_tile_sums_at_every_seam(dev, ho, wo, form):
    """Rules (1) and (2) of the module docstring on every tile, for 1 and 3 planes and every input kind.  Recorded per case
    (metrics_leaf[level,...]): `worst_ratio` = e_hip / e_ref, `worst_e_hip`, `worst_vs_s32` = |S - S32| / n."""
    h, w = ho + 10, wo + 10
    counts = R.tile_counts(ho, wo)
    ratio = e_max = d_max = 0.0
    for planes in (1, 3):
        for name, (x, y) in _level_inputs(planes, h, w, form == "f32").items():
            got = _level(dev, x, y)
            s64, s32 = _truth(x, y)
            assert got.shape == s64.shape == (planes,) + counts.shape + (2,)
            r, e, d = _hold(got, s64, s32, counts, f"{form} {planes} x {h} x {w} {name}")
            ratio, e_max, d_max = max(ratio, r), max(e_max, e), max(d_max, d)
    record(f"metrics_leaf[level,{form},{h}x{w}]", worst_ratio=ratio, worst_e_hip=e_max, worst_vs_s32=d_max, floor=FLOOR)
    print(f"level {form} {h}x{w}: worst e_hip / e_ref {ratio:.4f}, worst e_hip {e_max:.3e}, worst |S - S32| / n {d_max:.3e}")


def test_level_wrapper_is_the_entry_point(dev):
    from mcquic_amd import ops
    x, y = _noise(3, 3, 43, 247)
    for a, b in ((x, y), (x.float(), y.float())):
        got = ops.ssim_level(a.view(1, 3, 43, 247).to(dev), b.view(1, 3, 43, 247).to(dev)).cpu()
        assert got.shape == (3, 3, 3, 2) and np.array_equal(got.numpy(), _level(dev, a, b))
    with pytest.raises(ValueError):
        ops.ssim_level(x[:, :10].to(dev), y[:, :10].to(dev))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.ssim_level(x, y)


# 43 x 247: a 33 x 237 map, 3 x 3 tiles, the last row of tiles one position high, the last column one wide.  A pixel (r, c) reaches the
# map positions rows r - 10 .. r, columns c - 10 .. c.
IMPULSES = {
    "inside": ((12, 60), {(0, 0)}),
    "row_seam": ((20, 60), {(0, 0), (1, 0)}),
    "column_seam": ((12, 122), {(0, 0), (0, 1)}),
    "corner": ((20, 122), {(0, 0), (0, 1), (1, 0), (1, 1)}),
    "ragged": ((37, 240), {(1, 1), (1, 2), (2, 1), (2, 2)}),
    "last_pixel": ((42, 246), {(2, 2)}),
}


@pytest.mark.parametrize("form", ["u8", "f32"])
@pytest.mark.parametrize("delta", [1, 255])
@pytest.mark.parametrize("where", list(IMPULSES))
def test_level_impulse_stays_in_its_footprint(dev, where, delta, form):
    """x == y but for one pixel: tiles outside the pixel's footprint return exactly n for both sums (identical windows give exactly 1:
    2 mu12 = mu1^2 + mu2^2 and 2 s12 = s1 + s2 bit for bit), tiles inside meet rules (1) and (2), and the output is the 3 x 3 grid."""
    (r, c), inside = IMPULSES[where]
    h, w = 43, 247
    counts = R.tile_counts(h - 10, w - 10)
    foot = {(i, j) for i in range(3) for j in range(3)
            if max(i * 16, r - 10) <= min(i * 16 + 15, r, h - 11) and max(j * 118, c - 10) <= min(j * 118 + 117, c, w - 11)}
    assert foot == inside and counts.shape == (3, 3)
    x, _ = _noise(77, 1, h, w)
    y = x.clone()
    if delta == 255:
        x[0, r, c], y[0, r, c] = 0, 255
    else:
        y[0, r, c] = x[0, r, c] + 1 if x[0, r, c] < 255 else 254
    if form == "f32":
        x, y = x.float(), y.float()
    got = _level(dev, x, y)
    assert got.shape == (1, 3, 3, 2)
    s64, s32 = _truth(x, y)
    for i in range(3):
        for j in range(3):
            if (i, j) not in foot:
                assert got[0, i, j, 0] == counts[i, j] and got[0, i, j, 1] == counts[i, j], f"tile ({i}, {j}) outside the footprint: {got[0, i, j]} != {counts[i, j]}"
            elif abs(s64[0, i, j, 1] - counts[i, j]) > counts[i, j] * 2.0 ** -20:        # (the last pixel's weight is 1e-6: |delta| = 1 drowns)
                assert got[0, i, j, 1] != counts[i, j], f"tile ({i}, {j}) inside the footprint did not see the pixel"
    _hold(got, s64, s32, counts, f"impulse {where} {delta} {form}")


# ---- halve ----------------------------------------------------------------------------------------------------------------------------------
def _halve_guarded(dev, x, y):
    """ops.ms_ssim_halve into outputs followed by guard words -> (xo, yo) on the device."""
    from mcquic_amd import ops
    shape = tuple(x.shape[:-2]) + ((x.shape[-2] + 1) // 2, (x.shape[-1] + 1) // 2)
    n = int(np.prod(shape))
    bufs = [torch.full((n + GUARD,), SENTINEL, dtype=torch.float32, device=dev) for _ in range(2)]
    for b in bufs:
        b[:n].fill_(float("nan"))
    xo, yo = ops.ms_ssim_halve(x, y, out=(bufs[0][:n].view(shape), bufs[1][:n].view(shape)))
    _sync(f"halve {tuple(x.shape)}")
    assert xo.data_ptr() == bufs[0].data_ptr() and yo.data_ptr() == bufs[1].data_ptr()
    assert all(bool((b[n:] == SENTINEL).all()) for b in bufs), "guard words behind a pooled image written"
    return xo, yo


@pytest.mark.parametrize("w", (11, 12, 13, 161, 162))
@pytest.mark.parametrize("h", (11, 12, 13, 161, 162))
def test_halve_chain_is_exact(dev, h, w):
    """Four pooling steps from uint8, each fed by the last, 1 and 4 planes: every level equals halve64 bit for bit (module docstring)."""
    for planes in (1, 4):
        g = torch.Generator().manual_seed(h * 1000 + w + planes)
        x = torch.randint(0, 256, (planes, h, w), generator=g, dtype=torch.uint8)
        y = torch.randint(0, 256, (planes, h, w), generator=g, dtype=torch.uint8)
        x[0, 0, :], x[0, :, 0], y[0, -1, :], y[0, :, -1] = 255, 255, 255, 255            # the rows and columns next to the padding
        rx, ry = R.pyramid64(x.numpy()), R.pyramid64(y.numpy())
        xd, yd = x.to(dev), y.to(dev)
        for level in range(1, 5):
            xd, yd = _halve_guarded(dev, xd, yd)
            assert xd.dtype == torch.float32 and tuple(xd.shape) == rx[level].shape
            assert np.array_equal(xd.cpu().double().numpy(), rx[level]), f"x, level {level}, {planes} planes"
            assert np.array_equal(yd.cpu().double().numpy(), ry[level]), f"y, level {level}, {planes} planes"


# ---- finish and the whole pipeline ------------------------------------------------------------------------------------------------------------
def _stage_inputs(shape):
    n, c, h, w = shape
    x3, y3 = M.make_u8_pair(h * 1000 + w, n * ((c + 2) // 3), h, w)
    x = x3.reshape(-1, h, w)[: n * c].reshape(n, c, h, w).contiguous()
    y = y3.reshape(-1, h, w)[: n * c].reshape(n, c, h, w).contiguous()
    return x, y


@pytest.mark.parametrize("shape", [(1, 3, 161, 161), (2, 1, 175, 389), (1, 4, 322, 163), (1, 1, 161, 2071)], ids=str)
def test_stages_of_a_full_call(dev, shape):
    """What a full mcq_ms_ssim_u8 call left in its workspace: the pooled images equal the halve chain bit for bit; the level table is
    the float32 of the level kernel's tile sums added in tile order over the count (ssim_finish_kernel, bit for bit) and meets the truth
    by rule (1) per level, plane and map; `out` is ops.ms_ssim's and the combine stage's bits.  (1, 1, 161, 2071): a second column tile
    in the level table's sums at every level.  Recorded: metrics_leaf[stages,...]."""
    from mcquic_amd import ops
    n, c, h, w = shape
    p = n * c
    x, y = _stage_inputs(shape)
    xd, yd = x.to(dev), y.to(dev)
    out, table, pooled = ops.ms_ssim_stages(xd, yd)
    _sync(f"ms_ssim_stages {shape}")
    assert torch.equal(out, ops.ms_ssim(xd, yd)) and torch.equal(out, ops.ms_ssim_combine(table))
    assert table.shape == (5, n, c, 2) and len(pooled) == 4
    want = R.combine64(table.cpu().numpy())
    c_hip, c_ref = np.abs(out.cpu().double().numpy() - want), np.abs(_combine_f32(table.cpu().numpy()) - want)
    assert (c_hip <= np.maximum(4 * c_ref, FLOOR)).all(), f"out is not the combination of its own level table: e_hip {c_hip}, e_ref {c_ref}"
    rx, ry = R.pyramid64(x.view(p, h, w).numpy()), R.pyramid64(y.view(p, h, w).numpy())
    ox, oy = x.view(p, h, w).float(), y.view(p, h, w).float()
    table = table.cpu().view(5, p, 2).numpy()
    ratio = e_max = 0.0
    multi = []
    for l in range(5):
        hl, wl = rx[l].shape[1:]
        if l:
            px, py = pooled[l - 1]
            assert np.array_equal(px.cpu().view(p, hl, wl).double().numpy(), rx[l]), f"pooled x of level {l}"
            assert np.array_equal(py.cpu().view(p, hl, wl).double().numpy(), ry[l]), f"pooled y of level {l}"
            lx, ly = px.cpu().view(p, hl, wl), py.cpu().view(p, hl, wl)
        else:
            lx, ly = x.view(p, h, w), y.view(p, h, w)
        count = float(hl - 10) * float(wl - 10)
        # finish: tile partials in tile order, one division, one rounding
        sums = _level(dev, lx, ly)
        multi.append(sums.shape[1] * sums.shape[2])
        acc = np.zeros((p, 2))
        for t in sums.reshape(p, -1, 2).transpose(1, 0, 2):
            acc = acc + t
        assert np.array_equal((acc / count).astype(np.float32), table[l]), f"level {l}: the table is not the tile sums in tile order over the count"
        # the truth and the float32 restatement of the means
        s64, c64 = R.maps64(rx[l], ry[l])
        s32, c32 = M.ssim_and_cs_maps(ox[None], oy[None], M.gauss_window())
        m64 = np.stack([s64.mean(axis=(1, 2)), c64.mean(axis=(1, 2))], axis=-1)
        m32 = np.stack([s32[0].double().mean(dim=(1, 2)).numpy(), c32[0].double().mean(dim=(1, 2)).numpy()], axis=-1)
        e_hip, e_ref = np.abs(table[l].astype(np.float64) - m64), np.abs(m32 - m64)
        assert (e_hip <= np.maximum(4 * e_ref, FLOOR)).all(), f"level {l}: e_hip {e_hip.tolist()}, e_ref {e_ref.tolist()}"
        above = (e_ref > 0) & (e_hip > FLOOR)           # (below the floor the table's own float32 rounding, 2^-25, is what differs)
        if above.any():
            ratio = max(ratio, float((e_hip[above] / e_ref[above]).max()))
        e_max = max(e_max, float(e_hip.max()))
        if l < 4:
            ox, oy = M._halve(ox), M._halve(oy)
    assert multi[0] > 1 and multi[1] > 1
    if shape == (1, 1, 161, 2071):
        assert all(R.tile_grid(a.shape[1] - 10, a.shape[2] - 10)[1] >= 2 for a in rx)
    record(f"metrics_leaf[stages,{n}x{c}x{h}x{w}]", worst_ratio_above_floor=ratio, worst_e_hip=e_max, out_e_hip=float(c_hip.max()), out_e_ref=float(c_ref.max()), floor=FLOOR)
    print(f"stages {shape}: level table worst e_hip / e_ref above the floor {ratio:.4f}, worst e_hip {e_max:.3e}; out e_hip {c_hip.max():.3e}, e_ref {c_ref.max():.3e}")


# ---- combine ----------------------------------------------------------------------------------------------------------------------------------
VARIANTS = ("random", "ones", "zero_cs", "negative", "all_zero", "tiny")


def _table(n, c, seed, variant_of):
    """[5, n, c, 2] float32: independent random columns in (0, 1], the columns the kernel must not read (SSIM on levels 0..3, CS on the
    last) far away at -7 or 3 on every other image; then per image the variant `variant_of(image)`."""
    rng = np.random.default_rng(seed)
    t = (1.0 - rng.random((5, n, c, 2))).astype(np.float32)
    t[:4, 0::2, :, 0], t[4, 0::2, :, 1] = -7.0, 3.0
    for i in range(n):
        v = VARIANTS[variant_of(i)]
        if v == "ones":
            t[:, i] = 1.0
        elif v == "zero_cs":
            t[2, i, 0, 1], t[2, i, 0, 0] = 0.0, 0.9
        elif v == "negative":
            t[1, i, c - 1, 1] = -0.3
            t[4, i, 0, 0] = -1e-3
        elif v == "all_zero":
            for ch in range(c):
                t[ch % 5, i, ch, 1 if ch % 5 < 4 else 0] = 0.0 if ch % 2 else -0.5
        elif v == "tiny":
            t[0, i, 0, 1], t[4, i, c - 1, 0] = 1e-30, 1e-30
    return t


def _combine_f32(t):
    """The kernel's formula op by op in torch float32: relu, pow, the product level by level, the channel sum, one division."""
    t = torch.from_numpy(t)
    w = torch.tensor(M.MS_WEIGHTS)
    v = torch.relu(torch.cat([t[:4, :, :, 1], t[4:, :, :, 0]], dim=0))
    prod = v[0] ** w[0]
    for l in range(1, 5):
        prod = prod * v[l] ** w[l]
    s = prod[:, 0]
    for ch in range(1, prod.shape[1]):
        s = s + prod[:, ch]
    return (s / float(prod.shape[1])).double().numpy()


@pytest.mark.parametrize("c", [1, 3, 4])
@pytest.mark.parametrize("n", [1, 65])
def test_combine_on_injected_tables(dev, n, c):
    """mcq_ms_ssim_combine_f32 on tables it did not make.  N = 65 needs two workgroups and cycles the variants by image; N = 1 runs one table
    per variant.  Against combine64, per image: e_hip <= max(4 e_ref, 2^-23), e_ref the same formula in torch float32 on that image;
    an image of which every channel holds a zero or a negative is exactly 0.0; all ones is exactly 1.0.  Recorded (the worst of
    either side, for the record only): metrics_leaf[combine,...]."""
    from mcquic_amd import ops
    tables = [_table(n, c, 100 * n + c, lambda i: i % len(VARIANTS))] if n > 1 else [_table(n, c, 10 * k + c, lambda i, k=k: k) for k in range(len(VARIANTS))]
    e_hip = e_ref = 0.0
    for k, t in enumerate(tables):
        got = ops.ms_ssim_combine(torch.from_numpy(t).to(dev)).cpu().double().numpy()
        _sync(f"combine {n} {c}")
        want = R.combine64(t)
        assert got.shape == want.shape == (n,)
        eh, er = np.abs(got - want), np.abs(_combine_f32(t) - want)
        bad = eh > np.maximum(4 * er, FLOOR)
        assert not bad.any(), f"table {k}, images {np.argwhere(bad).ravel().tolist()}: e_hip {eh[bad]}, e_ref {er[bad]}"
        e_hip, e_ref = max(e_hip, float(eh.max())), max(e_ref, float(er.max()))
        for i in range(n):
            v = VARIANTS[(i if n > 1 else k) % len(VARIANTS)]
            if v == "all_zero" or (c == 1 and v in ("zero_cs", "negative")):
                assert want[i] == 0.0 and got[i] == 0.0, f"image {i} ({v}): {got[i]!r}"
            elif v == "ones":
                assert got[i] == 1.0
            else:
                assert 0.0 < got[i] < 1.0, f"image {i} ({v}): {got[i]!r}"
    record(f"metrics_leaf[combine,n{n},c{c}]", worst_e_hip=e_hip, worst_e_ref=e_ref, floor=FLOOR)
    print(f"combine n{n} c{c}: worst e_hip {e_hip:.3e}, worst e_ref {e_ref:.3e}")


# ---- squared differences ------------------------------------------------------------------------------------------------------------------------
def _sq_want(x, y):
    return ((x.to(torch.int64) - y.to(torch.int64)) ** 2).flatten(1).sum(1)


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("per_image", [1, 15, 16, 17, 16383, 16384, 16385, 16400, 32768])
def test_sqdiff_sizes_around_the_vector_path_and_the_chunk(dev, per_image, n):
    from mcquic_amd import ops
    g = torch.Generator().manual_seed(per_image + n)
    x = torch.randint(0, 256, (n, 1, 1, per_image), generator=g, dtype=torch.uint8)
    y = torch.randint(0, 256, (n, 1, 1, per_image), generator=g, dtype=torch.uint8)
    xd, yd = x.to(dev), y.to(dev)
    assert xd.data_ptr() % 16 == 0 and yd.data_ptr() % 16 == 0
    assert torch.equal(ops.sqdiff_sum(xd, yd).cpu(), _sq_want(x, y))
    if per_image == 32768:
        x.fill_(255)
        y.fill_(0)
        assert torch.equal(ops.sqdiff_sum(x.to(dev), y.to(dev)).cpu(), torch.full((n,), 255 * 255 * 32768))
        assert torch.equal(ops.sqdiff_sum(y.to(dev), x.to(dev)).cpu(), torch.full((n,), 255 * 255 * 32768))


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("per_image", [16384, 16400])
def test_sqdiff_with_a_misaligned_base(dev, per_image, n):
    """Both tensors start one byte past a 16-byte boundary (contiguous views into larger buffers, which ops.sqdiff_sum passes on as they
    are): sizes that are multiples of 16 must then leave the 16-byte loads alone."""
    from mcquic_amd import ops
    g = torch.Generator().manual_seed(per_image + n)
    x = torch.randint(0, 256, (n, 1, 1, per_image), generator=g, dtype=torch.uint8)
    y = torch.randint(0, 256, (n, 1, 1, per_image), generator=g, dtype=torch.uint8)
    views = []
    for t in (x, y):
        buf = torch.zeros(n * per_image + 64, dtype=torch.uint8, device=dev)
        off = (1 - buf.data_ptr()) % 16
        v = buf[off: off + n * per_image].view(n, 1, 1, per_image)
        v.copy_(t)
        assert v.is_contiguous() and v.data_ptr() % 16 == 1
        views.append(v)
    assert torch.equal(ops.sqdiff_sum(views[0], views[1]).cpu(), _sq_want(x, y))
    aligned = x.to(dev)
    assert torch.equal(ops.sqdiff_sum(views[0], aligned).cpu(), torch.zeros(n, dtype=torch.int64))      # one base aligned, one not
