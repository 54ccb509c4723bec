"""The MS-SSIM loss kernels (mcquic_amd/csrc/msssim_loss.hip) restated on the CPU operation by operation, for
tests/test_gpu_msssim_leaf.py (which holds the kernels to it) and tests/test_msssim_refs.py (which holds it to oracle/metrics_ref.py
and to float64 autograd).  Nothing here imports mcquic_amd: it is numpy on the CPU, one float32 rounding per operation in the
kernels' order (the library is built with -ffp-contract=off, float divide is correctly rounded on both sides, numpy neither fuses nor
reassociates).  What a correct kernel returns bit for bit:

  saved      the pooled pyramids of levels 1..4 (`pyramids`, `pack_saved`)
  da, db     whenever the per-level scales are the same floats on both sides (`scales`: float64 with two `pow`, rounded to float32
             once -- the same bits for crafted values of exactly 1, within one float32 spacing otherwise)

and what it returns up to the order of a float64 sum: `values` (the float32 maps are exact here, their mean is taken exactly).

Planes are [P, H, W] float32 arrays, P = N * C; level 0 is the input + offset, level l + 1 the 2 x 2 mean of level l with the zero
padding of an odd side on the top / left."""
import math

import numpy as np

F = np.float32
TH, TW, HALO, LEVELS = 16, 118, 10, 5                       # map tile of the kernels, window size - 1
WIN = np.array([float.fromhex(h) for h in ("0x1.0d957p-10", "0x1.f1fe02p-8", "0x1.26eb18p-5", "0x1.bff0fep-4", "0x1.b43c3ep-3", "0x1.10656p-2",
                                            "0x1.b43c3ep-3", "0x1.bff0fep-4", "0x1.26eb18p-5", "0x1.f1fe02p-8", "0x1.0d957p-10")], dtype=F)
LEVEL_W = np.array([float.fromhex(h) for h in ("0x1.6f0068p-5", "0x1.247454p-2", "0x1.334d6ap-2", "0x1.e3f142p-3", "0x1.10ff98p-3")], dtype=F)
INTERIOR, BORDER, SEAM = 0, 1, 2
CLASS_NAMES = ("interior", "border", "seam")


# ---- sizes and layouts (make_pyramid / layout) --------------------------------------------------------------------------------------------
def pyramid_sizes(h, w):
    out = []
    for _ in range(LEVELS):
        out.append((h, w))
        h, w = (h + 2 * (h & 1) - 2) // 2 + 1, (w + 2 * (w & 1) - 2) // 2 + 1
    return out


def saved_layout(planes, h, w):
    """(sizes, off, floats): level l (1..4) has x at off[l] and y planes * H_l * W_l floats later."""
    sizes, off, fl = pyramid_sizes(h, w), [None], 0
    for hl, wl in sizes[1:]:
        off.append(fl)
        fl += 2 * planes * hl * wl
    return sizes, off, fl


def workspace_bytes(planes, h, w, backward):
    sizes, _, pyr = saved_layout(planes, h, w)
    if not backward:
        return planes * max(((wl - HALO + TW - 1) // TW) * ((hl - HALO + TH - 1) // TH) for hl, wl in sizes) * 8
    scale = (5 * planes + 63) & ~63
    return (scale + 5 * planes * (h - HALO) * (w - HALO) + pyr) * 4


# ---- forward ----------------------------------------------------------------------------------------------------------------------------
def pool_f32(x):
    """msl_halve_kernel: (((v0 + v1) + v2) + v3) / 4, rows 2i - ph, 2i - ph + 1 (zeros where that is row -1), columns alike."""
    p_, h, w = x.shape
    ph, pw = h & 1, w & 1
    p = np.zeros((p_, h + ph, w + pw), F)
    p[:, ph:, pw:] = x
    return (((p[:, 0::2, 0::2] + p[:, 0::2, 1::2]) + p[:, 1::2, 0::2]) + p[:, 1::2, 1::2]) / F(4)


def pyramids(a, b, offset):
    """([x_0..x_4], [y_0..y_4]): x_0 = a + offset in float32 (the kernels add it at every level-0 load)."""
    xs, ys = [a.astype(F) + F(offset)], [b.astype(F) + F(offset)]
    for _ in range(LEVELS - 1):
        xs.append(pool_f32(xs[-1]))
        ys.append(pool_f32(ys[-1]))
    return xs, ys


def pack_saved(xs, ys):
    return np.concatenate([t.ravel() for l in range(1, LEVELS) for t in (xs[l], ys[l])])


def blur_valid(q, win=WIN):
    """Vertical pass, then horizontal: w0 q0, then + w_t q_t for t = 1..10 (vertical_pass / horizontal)."""
    ho = q.shape[1] - HALO
    acc = win[0] * q[:, 0:ho]
    for t in range(1, 11):
        acc = acc + win[t] * q[:, t:t + ho]
    wo = q.shape[2] - HALO
    out = win[0] * acc[:, :, 0:wo]
    for t in range(1, 11):
        out = out + win[t] * acc[:, :, t:t + wo]
    return out


def moments(x, y):
    return [blur_valid(q) for q in (x, y, x * x, y * y, x * y)]


def c_of(k, data_range):
    d = float(F(data_range))
    return F((k * d) * (k * d))


def level_map(f, c1, c2, last):
    """msl_level_kernel: the cs map, on the last level the ssim map."""
    mu1_sq, mu2_sq, mu12 = f[0] * f[0], f[1] * f[1], f[0] * f[1]
    s1, s2, s12 = f[2] - mu1_sq, f[3] - mu2_sq, f[4] - mu12
    cs = (F(2) * s12 + c2) / ((s1 + s2) + c2)
    return ((F(2) * mu12 + c1) / ((mu1_sq + mu2_sq) + c1)) * cs if last else cs


def forward(a, b, offset, data_range, planes=None):
    """dict(xs, ys, saved, mean [5, P'] float64, absmean [5, P']) -- `mean`: the exact mean (math.fsum, one division) of each float32 map,
    `absmean` the same of its magnitudes (the scale of a summation error); of the planes in `planes` only (all when None)."""
    xs, ys = pyramids(a, b, offset)
    c1, c2 = c_of(0.01, data_range), c_of(0.03, data_range)
    sel = list(range(a.shape[0])) if planes is None else list(planes)
    mean, absmean = np.zeros((LEVELS, len(sel))), np.zeros((LEVELS, len(sel)))
    for l in range(LEVELS):
        m = level_map(moments(xs[l][sel], ys[l][sel]), c1, c2, l == LEVELS - 1)
        for i in range(len(sel)):
            flat = m[i].ravel().astype(np.float64)
            mean[l, i], absmean[l, i] = math.fsum(flat) / flat.size, math.fsum(np.abs(flat)) / flat.size
    return dict(xs=xs, ys=ys, saved=pack_saved(xs, ys), mean=mean, absmean=absmean)


def loss64(values):
    """1 - mean prod relu(v)^w in float64 on float32 `values` [5, P]."""
    v = np.maximum(values.astype(np.float64), 0.0)
    return 1.0 - float(np.prod(v ** LEVEL_W.astype(np.float64)[:, None], axis=0).mean())


def loss_f32(values):
    """msl_combine_kernel op by op: powf, the product level by level in float32, the sum in float64, 1 - float32(mean)."""
    v = np.maximum(values.astype(F), F(0))
    prod = np.power(v[0], LEVEL_W[0])
    for l in range(1, LEVELS):
        prod = prod * np.power(v[l], LEVEL_W[l])
    return F(1) - F(math.fsum(prod.astype(np.float64)) / prod.size)


# ---- backward ---------------------------------------------------------------------------------------------------------------------------
def scales(values, dloss, h, w):
    """msl_dv_kernel: float64, rounded to float32 once -> [5, P]."""
    v = values.astype(np.float64)
    planes = v.shape[1]
    wd = LEVEL_W.astype(np.float64)
    pos = v > 0.0
    vp = np.where(pos, v, 1.0)
    f = np.where(pos, np.power(vp, wd[:, None]), 0.0)
    g = -float(F(dloss)) / float(planes)
    out = np.zeros((LEVELS, planes), F)
    for l, (hl, wl) in enumerate(pyramid_sizes(h, w)):
        others = np.ones(planes)
        for k in range(LEVELS):
            if k != l:
                others = others * f[k]
        d = np.where(pos[l], ((g * wd[l]) * np.power(vp[l], wd[l] - 1.0)) * others, 0.0)
        out[l] = (d / (float(hl - HALO) * float(wl - HALO))).astype(F)
    return out


def grad_planes(f, s, c1, c2, last):
    """msl_grad_maps_kernel: [g_mu_x, g_xx, g_xy, g_mu_y, g_yy], each s * (the map's partial), an exact 0 where s == 0."""
    mx, my = f[0], f[1]
    s1, s2, s12 = f[2] - mx * mx, f[3] - my * my, f[4] - mx * my
    bden = (s1 + s2) + c2
    cs = (F(2) * s12 + c2) / bden
    gxy, gxx = F(2) / bden, -cs / bden
    gmx, gmy = F(2) * (mx * cs - my) / bden, F(2) * (my * cs - mx) / bden
    if last:
        q = (mx * mx + my * my) + c1
        lum = (F(2) * mx * my + c1) / q
        gmx = cs * (F(2) * (my - mx * lum) / q) + lum * gmx
        gmy = cs * (F(2) * (mx - my * lum) / q) + lum * gmy
        gxy = lum * gxy
        gxx = lum * gxx
    sb = s.astype(F)[:, None, None]
    zero = sb == 0
    return [np.where(zero, F(0), sb * g) for g in (gmx, gxx, gxy, gmy, gxx)]


def tblur(g, win=WIN, fault_col=None):
    """The transposed blur: the valid blur of the map zero-extended by 10 on every side.  `fault_col`: a deliberately wrong variant for
    the tests of the tests -- output column `fault_col` loses its last horizontal tap."""
    p = np.zeros((g.shape[0], g.shape[1] + 2 * HALO, g.shape[2] + 2 * HALO), g.dtype)
    p[:, HALO:-HALO, HALO:-HALO] = g
    if fault_col is None:
        return blur_valid(p, win)
    ho = p.shape[1] - HALO
    acc = win[0] * p[:, 0:ho]
    for t in range(1, 11):
        acc = acc + win[t] * p[:, t:t + ho]
    out = blur_valid(p, win)
    col = win[0] * acc[:, :, fault_col]
    for t in range(1, 10):
        col = col + win[t] * acc[:, :, fault_col + t]
    out[:, :, fault_col] = col
    return out


def pool_adjoint(d, h, w):
    """d of level l + 1 at the level-l pixels it averaged: pixel (r, c) -> ((r + ph) >> 1, (c + pw) >> 1)."""
    ri, ci = (np.arange(h) + (h & 1)) >> 1, (np.arange(w) + (w & 1)) >> 1
    return d[:, ri][:, :, ci]


def backward(a, b, offset, data_range, values, dloss, want_db=True, levels=None, with_scale=False, fault=None):
    """(da, db, Sa, Sb) [P, H, W]: msl_grad_maps_kernel + msl_grad_input_kernel, levels coarse to fine, d = (b0 + (2x) b1) + y b2, then
    + dnext * 0.25; the second pass with x and y swapped.  `levels`: only these levels' scales are kept (a per-level restatement: the
    others take the exact-zero path).  S (float64, with_scale): the same recursion with every term replaced by its magnitude,
    B'|g_mu| + 2|x| B'|g_xx| + |y| B'|g_xy| + pool_adjoint(S_next).  `fault = (level, column)`: see tblur."""
    p_, h, w = a.shape
    xs, ys = pyramids(a, b, offset)
    c1, c2 = c_of(0.01, data_range), c_of(0.03, data_range)
    sc = scales(values, dloss, h, w)
    if levels is not None:
        for l in range(LEVELS):
            if l not in levels:
                sc[l] = 0
    sizes = pyramid_sizes(h, w)
    win64 = WIN.astype(np.float64)
    dx = dy = sx = sy = None
    for l in range(LEVELS - 1, -1, -1):
        hl, wl = sizes[l]
        x, y = xs[l], ys[l]
        g = grad_planes(moments(x, y), sc[l], c1, c2, l == LEVELS - 1)
        fc = fault[1] if fault is not None and fault[0] == l else None
        passes = [(g[0], g[1], g[2], x, y, dx, sx)] + ([(g[3], g[4], g[2], y, x, dy, sy)] if want_db else [])
        res = []
        for gm, gsq, gxy, p, q, dnext, snext in passes:
            b0, b1, b2 = tblur(gm, fault_col=fc), tblur(gsq, fault_col=fc), tblur(gxy, fault_col=fc)
            d = (b0 + (F(2) * p) * b1) + q * b2
            if dnext is not None:
                d = d + pool_adjoint(dnext, hl, wl) * F(0.25)
            s = None
            if with_scale:
                t0, t1, t2 = (tblur(np.abs(t).astype(np.float64), win64) for t in (gm, gsq, gxy))
                s = t0 + 2.0 * np.abs(p).astype(np.float64) * t1 + np.abs(q).astype(np.float64) * t2
                if snext is not None:
                    s = s + pool_adjoint(snext, hl, wl) * 0.25
            res.append((d, s))
        dx, sx = res[0]
        if want_db:
            dy, sy = res[1]
    return dx, dy, sx, sy


# ---- region classes -------------------------------------------------------------------------------------------------------------------------
def region_classes(h, w):
    """uint8 [h, w] per level-0 pixel: SEAM -- at some level its column lies within 10 of a multiple (>= 1) of 118, the column edge of a
    map tile (msl_level_kernel, msl_grad_maps_kernel) and of an image tile (msl_grad_input_kernel, whose patch starts at c0 - 10);
    BORDER -- not a seam, and at some level within 10 of an image edge (the transposed blur's support is cut); INTERIOR -- the rest.
    Levels are mapped up through the pooling's index map.  Row tiles are 16 high, so EVERY row lies within 10 of a row seam at every
    level: row seams cannot tell pixels apart and all three classes contain them."""
    def up(n0, dim):
        idx, out = np.arange(n0), []
        for sz in [s[dim] for s in pyramid_sizes(h, w)]:
            out.append((idx.copy(), sz))
            idx = (idx + (sz & 1)) >> 1
        return out
    seam_c, border_c, border_r = np.zeros(w, bool), np.zeros(w, bool), np.zeros(h, bool)
    for idx, sz in up(w, 1):
        k = np.rint(idx / TW)
        seam_c |= (k >= 1) & (np.abs(idx - k * TW) <= HALO)
        border_c |= (idx < HALO) | (idx >= sz - HALO)
    for idx, sz in up(h, 0):
        border_r |= (idx < HALO) | (idx >= sz - HALO)
    cls = np.full((h, w), INTERIOR, np.uint8)
    cls[border_r[:, None] | border_c[None, :]] = BORDER
    cls[:, seam_c] = SEAM
    return cls


def pixel_levels(h, w, r, c):
    """[(level, row, column, on a column seam, within 10 of an edge)] of the level-0 pixel (r, c) mapped down the pyramid."""
    out = []
    for l, (hl, wl) in enumerate(pyramid_sizes(h, w)):
        k = int(np.rint(c / TW))
        out.append((l, r, c, k >= 1 and abs(c - k * TW) <= HALO, min(r, c) < HALO or r >= hl - HALO or c >= wl - HALO))
        r, c = (r + (hl & 1)) >> 1, (c + (wl & 1)) >> 1
    return out


def worst_by_class(err, cls):
    """{class name: max of err [P, H, W] over the pixels of the class} (absent classes left out)."""
    return {CLASS_NAMES[k]: float(err[:, cls == k].max()) for k in (INTERIOR, BORDER, SEAM) if bool((cls == k).any())}
