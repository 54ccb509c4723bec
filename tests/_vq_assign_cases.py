"""The cases of the assignment-kernel leaf tests, shared by tests/test_vq_assign_plan.py (each case's launch plan as a literal, asserted
against mcq_vq_assign_plan -- the plan vq_assign_launch of csrc/vq.hip itself launches by) and tests/test_gpu_vq_assign_leaf.py (the
launches).  Imports nothing of mcquic_amd: NumPy and the references of tests/_rate_ref.py / tests/_rate_map_ref.py only.

A case: name, (m, k, d, n, h, w), `plan` = (instance, cs_log2, zs, bw_log2) and `forms`: "plain" (mcq_vq_assign_ws_f32), "rate"
(mcq_vq_assign_rate_map_f32, RATE = true) or "both".  instance names the <SPC, XLDS> pair of vq_assign_kernel: SP8 d = 1..16, SP32
d = 49..64, SP128 d = 241..256 below four codeword tiles, LDS the same staged in LDS (always four slices), LOOP every other length.

The geometry the comments speak of: a wave holds a vector tile of 2 blocks of 32 pixels (BW = 1 << bw_log2 wide, 32 / BW high); a
workgroup's 4 waves are 4 >> cs_log2 vector tiles x (1 << cs_log2) slices of the ntile = ceil(k / 128) codeword tiles, grid.z = zs
ranges deal them further: per_slice = ceil(ntile / (CS zs)) tiles each, so slices past the end are empty, and whole ranges past the
end are not launched (`launched_ranges`)."""
from collections import namedtuple

import numpy as np

import _rate_map_ref as MR
import _rate_ref as RR

LOOP, SP8, SP32, SP128, LDS = 0, 1, 2, 3, 4          # MCQ_VQ_ASSIGN_* of include/mcquic_hip.h (tests/test_vq_assign_plan.py compares)
INSTANCE_NAMES = {LOOP: "<0, false>", SP8: "<8, false>", SP32: "<32, false>", SP128: "<128, false>", LDS: "<128, true>"}
RING = 8                                              # VQ_PF: the prefetch ring's depth, the unit Sp is padded to
WINDOWS = {SP8: (1, 16), SP32: (49, 64), SP128: (241, 256), LDS: (241, 256)}      # the vector lengths an unrolled instance serves

Case = namedtuple("Case", "name m k d n h w plan forms")

CASES = [
    # ---- <8>: d <= 16 ------------------------------------------------------------------------------------------------------------------
    Case("sp8_one_vector", 1, 5, 1, 1, 1, 1, (SP8, 0, 1, 5), "both"),              # one vector, half a k-step, one partial tile
    Case("sp8_full_tile", 1, 128, 5, 1, 7, 40, (SP8, 0, 1, 3), "plain"),           # a full tile: the spare norm tile right behind it; odd d
    Case("sp8_k129_two_slices", 2, 129, 7, 2, 5, 7, (SP8, 1, 1, 3), "both"),       # one-row second tile, two slices
    Case("sp8_15_blocks", 1, 200, 9, 1, 9, 33, (SP8, 1, 1, 4), "plain"),           # 15 blocks: the odd last block of a wave pair; block seams
    Case("sp8_3_tiles_2_slices", 2, 384, 16, 1, 3, 70, (SP8, 1, 1, 5), "both"),    # 2 + 1 tiles; 5 vector tiles: an inactive wave pair stays for the barrier
    Case("sp8_ranged_rate", 1, 1024, 3, 1, 5, 7, (SP8, 2, 2, 3), "rate"),          # smallest ranged rate-map
    Case("sp8_zs8", 2, 4096, 8, 1, 4, 4, (SP8, 2, 8, 3), "both"),
    Case("sp8_zs16", 1, 8192, 4, 1, 2, 2, (SP8, 2, 16, 4), "both"),
    Case("sp8_2048_waves", 2, 129, 2, 1, 256, 256, (SP8, 0, 1, 5), "plain"),       # the production regime: one wave walks both tiles, unsliced
    Case("sp8_empty_range", 1, 2100, 3, 1, 2, 2, (SP8, 2, 4, 4), "both"),          # 17 tiles dealt 2 a slot over 4 x 4: range 3 owns none and is not launched
    # ---- <0>: the run-time k-loop ------------------------------------------------------------------------------------------------------
    Case("loop_d17_w1", 1, 130, 17, 2, 33, 1, (LOOP, 1, 1, 2), "plain"),           # Sp = 16, 4 x 8 blocks, w = 1
    Case("loop_d24_rate", 2, 512, 24, 1, 5, 7, (LOOP, 2, 1, 3), "rate"),           # the bits load at the tile head (RATE && !SPC)
    Case("loop_d100_empty_slice", 1, 640, 100, 1, 5, 7, (LOOP, 2, 1, 3), "both"),  # Sp = 56; 5 tiles over 4 slices of 2: slice 3 is empty
    Case("loop_d33_ranged", 1, 1100, 33, 1, 9, 33, (LOOP, 2, 2, 4), "both"),       # 9 tiles over 2 ranges x 4 slices: empty slices in range 1
    Case("loop_d24_ranged_rate", 1, 1100, 24, 2, 5, 7, (LOOP, 2, 2, 3), "rate"),   # the same through rt.bits + tile0 of blockIdx.z
    # ---- <32>: d = 49 .. 64 ------------------------------------------------------------------------------------------------------------
    Case("sp32_d49", 2, 129, 49, 1, 5, 7, (SP32, 1, 1, 3), "both"),                # the bottom of the window: 15 channels from the descriptor's 0
    Case("sp32_d63", 1, 512, 63, 2, 9, 33, (SP32, 2, 1, 4), "plain"),              # one below the top
    Case("sp32_45_blocks", 1, 300, 64, 3, 17, 17, (SP32, 1, 1, 3), "plain"),       # 45 blocks, 23 vector tiles
    Case("sp32_ranged", 2, 1024, 64, 1, 5, 7, (SP32, 2, 2, 3), "both"),            # smallest ranged d = 64
    Case("sp32_zs4", 1, 2048, 64, 1, 3, 5, (SP32, 2, 4, 3), "both"),
    Case("sp32_7_empty_ranges", 1, 9000, 50, 1, 3, 3, (SP32, 2, 16, 3), "both"),   # 71 tiles dealt 2 a slot over 16 x 4: 9 of 16 ranges launched
    # ---- <128, false>: d = 241 .. 256, fewer than four tiles ---------------------------------------------------------------------------
    Case("sp128_d241", 1, 129, 241, 1, 5, 7, (SP128, 1, 1, 3), "both"),
    Case("sp128_d256_3_tiles", 1, 384, 256, 1, 9, 5, (SP128, 1, 1, 3), "both"),
    # ---- <128, true>: the vector tile staged in LDS ------------------------------------------------------------------------------------
    Case("lds_d255", 1, 512, 255, 2, 5, 7, (LDS, 2, 1, 3), "plain"),               # staged tile with a missing channel
    Case("lds_d256_empty_slice", 1, 640, 256, 1, 9, 33, (LDS, 2, 1, 4), "plain"),  # 5 tiles over 4 slices; 8 vector tiles
    Case("lds_d241_ranged", 1, 1024, 241, 1, 3, 3, (LDS, 2, 2, 3), "both"),        # staged and ranged
]

BY_NAME = {c.name: c for c in CASES}
PACK_CASES = ((1, 5, 1), (2, 129, 7), (1, 200, 49), (1, 384, 241))                  # (m, k, d) of the operand-stream test

REFUSED = [(0, 1, 8, 4, 4, 128), (1, 0, 8, 4, 4, 128), (1, 1, 0, 4, 4, 128), (1, 1, 8, 0, 4, 128), (1, 1, 8, 4, 0, 128), (1, 1, 8, 4, 4, 0),
           (-1, 1, 8, 4, 4, 128), (1, 1, 8, 4, 4, -128),
           (1, 2, 64, 4096, 2048, 512),                       # d h w 4 = 2 GiB: one group's channels leave the buffer descriptor's window
           (1 << 20, 1, 1, 256, 256, 8)]                      # 2^31 pixel blocks of 1 x 32 (N, m, d, h, w, k)


def dims(case):
    """(N, m, d, h, w, k): the argument order of the C entry points."""
    return case.n, case.m, case.d, case.h, case.w, case.k


def runs(case, form):
    return case.forms in (form, "both")


def sp(d):
    """k-steps (channel pairs) per codeword tile, padded to the ring's depth."""
    return ((d + 1) // 2 + RING - 1) // RING * RING


def launched_ranges(ntile, cs_log2, zs):
    """grid.z as include/mcquic_hip.h states it: every (range, slice) is dealt per = ceil(ntile / (CS zs)) tiles in order, and only the
    ceil(ntile / (CS per)) ranges that own a tile are launched (range z owns none iff z CS per >= ntile)."""
    cs = 1 << cs_log2
    per_range = cs * ((ntile + cs * zs - 1) // (cs * zs))
    return (ntile + per_range - 1) // per_range


def geometry(case):
    """What the launch's shape works out to under the case's literal plan: a dict of blocks, vector tiles, grid.x, waves that hold no
    vector tile (they stay for the barrier when sliced, leave at once when not), ntile, per_slice, the (range, slice) pairs that
    are dealt no codeword tile and the ranges that are launched (those whose first slice owns one)."""
    _, cs_log2, zs, bw_log2 = case.plan
    bw, bh = 1 << bw_log2, 32 >> bw_log2
    blocks = case.n * ((case.w + bw - 1) // bw) * ((case.h + bh - 1) // bh)
    vtiles = (blocks + 1) // 2
    per_wg = 4 >> cs_log2
    gx = (vtiles + per_wg - 1) // per_wg
    ntile = (case.k + 127) // 128
    cs = 1 << cs_log2
    per_slice = (ntile + cs * zs - 1) // (cs * zs)
    empty = [(z, s) for z in range(zs) for s in range(cs) if (z * cs + s) * per_slice >= ntile]
    return dict(launched=launched_ranges(ntile, cs_log2, zs), blocks=blocks, vtiles=vtiles, gx=gx, inactive_waves=(gx * per_wg - vtiles) * cs, ntile=ntile, per_slice=per_slice,
                empty=empty, partial_blocks=case.h % bh != 0 or case.w % bw != 0)


def seed(case):
    return 7000 + 17 * sum(ord(ch) for ch in case.name)


def integer_case(case):
    """Inputs of the exact-arithmetic tests: x [n, m d, h, w] and codebook [m, k, d] integers uniform in [-4, 4] (float32), a table
    uint32 [m, k + 1] whose widths are powers of two 2^0 .. 2^12 (bits = 16 - log2 width is then an integer in 4 .. 16; the kernels
    read widths only, so the table's total is left alone) and lambda float32 [n, h, w] drawn from {0, 0.25, 3}.

    Ties are built in, not hoped for.  With k0 = ceil(k / 3), codeword i + k0 and codeword i + 2 k0 repeat codeword i, so every vector's
    nearest codeword exists up to three times, k0 apart: over the k of the table that puts the copies into the other half-wave,
    another 32-row band, the same row of another tile (k = 384), another slice and another range; codeword i + 4 repeats codeword i
    for i = 0 mod 16 (the same 8 rows, the other half-wave).  The first index must win each time.  The second copy repeats the width
    too (an exact tie under the rate term), the third keeps its own draw (it wins where lambda bits says so)."""
    rng = np.random.default_rng([20261021, seed(case)])
    k, k0 = case.k, (case.k + 2) // 3
    x = rng.integers(-4, 5, size=(case.n, case.m * case.d, case.h, case.w)).astype(np.float32)
    cb = rng.integers(-4, 5, size=(case.m, k, case.d)).astype(np.float32)
    widths = np.int64(1) << rng.integers(0, 13, size=(case.m, k))
    for i in range(0, k0 - 4, 16):
        cb[:, i + 4] = cb[:, i]
    cb[:, k0:2 * k0] = cb[:, :min(k0, k - k0)]
    cb[:, 2 * k0:] = cb[:, :k - 2 * k0]
    widths[:, k0:2 * k0] = widths[:, :min(k0, k - k0)]
    cdf = np.zeros((case.m, k + 1), dtype=np.int64)
    cdf[:, 1:] = np.cumsum(widths, -1)
    lam = np.asarray((0.0, 0.25, 3.0), dtype=np.float32)[rng.integers(0, 3, size=(case.n, case.h, case.w))]
    lam.reshape(-1)[0] = 0.25                                        # (a case of one vector runs under the rate term too)
    return x, cb, cdf.astype(np.uint32), lam


def packed_stream(cb):
    """vq_pack_kernel's index rule restated: codebook [m, k, d] -> float32 [m][ntile][Sp][64][4] + VQ_PF * 256 zeros, flat.  Element
    (g, tile, s, lane, q) holds channel 2 s + (lane >> 5) of codeword 128 tile + 32 q + (lane & 31); 0 past k and past d."""
    m, k, d = cb.shape
    ntile, steps = (k + 127) // 128, sp(d)
    padded = np.zeros((m, ntile * 128, 2 * steps), dtype=np.float32)
    padded[:, :k, :d] = cb
    # [g, tile, q, j, s, hi] -> [g, tile, s, hi, j, q]; lane = 32 hi + j
    out = padded.reshape(m, ntile, 4, 32, steps, 2).transpose(0, 1, 4, 5, 3, 2)
    return np.concatenate([np.ascontiguousarray(out).reshape(-1), np.zeros(RING * 256, dtype=np.float32)])


def gaussian_case(case):
    """Inputs of the float64 audits: `_rate_ref.make_case`'s standard Gaussians and Dirichlet table under the case's seed, and lambda
    float32 [n, h, w] from `_rate_map_ref.map_lambdas` (the CPU emulation and the GPU test draw the same)."""
    x, cb, cdf = RR.make_case(case.m, case.k, case.d, case.h, case.w, n=case.n, seed=seed(case))
    return x, cb, cdf, MR.map_lambdas(case.n, case.h, case.w, seed(case))


def _row_chunks(case_shape, per_row, budget):
    h = case_shape[2]
    rows = max(1, int(budget // max(1, per_row)))
    return [(r, min(h, r + rows)) for r in range(0, h, rows)]


def audit_rows(x, cb, bits, lam, got, budget=8e6):
    """(differing, unexcused) of `got` [n, m, h, w] against the float64 argmin under the project's bound, summed over bands of rows so
    that no temporary of the references passes `budget` elements.  lam None: the plain form through `_rate_ref.audit` at lambda = 0
    (its cost tensor is [m, V, k, d]); lam [n, h, w]: `_rate_map_ref.audit` ([m, V, k], channel by channel)."""
    n, _, h, w = x.shape
    m, k, d = cb.shape
    differ = unexcused = 0
    for r0, r1 in _row_chunks(x.shape, m * n * w * k * (d if lam is None else 1), budget):
        xs, gs = x[:, :, r0:r1], np.asarray(got)[:, :, r0:r1]
        dn, un = RR.audit(xs, cb, bits, 0.0, gs) if lam is None else MR.audit(xs, cb, bits, lam[:, r0:r1], gs)
        differ, unexcused = differ + dn, unexcused + un
    return differ, unexcused


def argmin_rows(x, cb, bits, lam, budget=8e6):
    """int64 [n, m, h, w]: NumPy's first-index argmin of the float64 costs |x - c|^2 + lambda_v bits (lam None: the distances alone),
    formed channel by channel over bands of rows."""
    n, _, h, w = x.shape
    m, k, _ = cb.shape
    if lam is None:
        bits, lam = np.zeros((m, k)), np.zeros((n, h, w), dtype=np.float32)
    out = np.empty((n, m, h, w), dtype=np.int64)
    for r0, r1 in _row_chunks(x.shape, m * n * w * k, budget):
        out[:, :, r0:r1] = MR.argmin_map(x[:, :, r0:r1], cb, bits, lam[:, r0:r1])
    return out
