"""The cases of the soft-assignment backward leaf tests, shared by tests/test_soft_bwd_plan.py (each case's route as a literal,
asserted against mcq_vq_soft_bwd_plan -- the routing mcq_vq_soft_bwd_f32 launches by) and tests/test_gpu_soft_bwd_leaf.py (the
launches).  Imports nothing of mcquic_amd.

A case: name, (N, m, d, h, w, k) and `plan` = (dx_form, dc_form, dx_split): 0 the lane-per-channel kernels (vq_dx_kernel / vq_dc_kernel),
1 the tiled ones (vq_dx_tiled_kernel: 8 vectors a workgroup, four codeword slices; vq_dc_tiled_kernel: 16 codewords a workgroup, four
vector slices), 2 the MFMA forms (csrc/vq_bwd_mfma.hip); dx_split the workgroups per 32-row tile of vq_dx_mfma_kernel.

What the shapes are for (V = N h w vectors per group, rows = V m):
  vq_dx_mfma_kernel   a wave's slice is k / (16 split) codewords = that many / 8 chunks behind a ring of 4: 1, 3, 5 chunks (k = 128,
                      384, 640; one workgroup per tile) and 1, 2, 4 (k = 256, 512, 1024; two) -- a ring that overruns by 3, by 1, a
                      whole ring plus a tail of 1, an exact ring; rows / 32 = 256 | 255 at k = 256: the two sides of the tile-count rule
  vq_dc_mfma_kernel   a wave's slice is V / 8 vectors = V / 16 steps behind a ring of 16: 1, 3, 16, 17 steps (V = 16, 48, 256, 272) and
                      66 vectors per wave (V = 528: the index scan takes a second pass with 2 live lanes); V = 16 runs the ring past
                      the end of ddist and of the channel-major copy; at V = 48 with 16 vectors an image the slices cross images
  d                   64, 33, 32, 31, 1 on both MFMA forms: the second 32-channel block full, with one lane, empty, the first partly
                      filled; 65 and 80: a second pass of the lane-per-channel kernels' channel loop
  m = 3 or N >= 2 wherever the edge allows it: a group other than 0 and a second image are addressed."""
from collections import namedtuple

import torch

Case = namedtuple("Case", "name n m d h w k plan")

CASES = [
    # ---- dx on the MFMA form, one workgroup per tile (dC: MFMA, V = 64) -------------------------------------------------------------
    Case("dxm1_k128", 2, 3, 64, 4, 8, 128, (2, 2, 1)),            # 1 chunk per wave: the ring overruns 3
    Case("dxm1_k384", 2, 3, 33, 4, 8, 384, (2, 2, 1)),            # 3 chunks
    Case("dxm1_k640", 2, 3, 32, 4, 8, 640, (2, 2, 1)),            # 5 chunks: a whole ring and a tail of 1 (k % 256 != 0: no split)
    Case("dxm1_tiles256", 1, 1, 8, 64, 128, 256, (2, 2, 1)),      # rows / 32 = 256: enough tiles, no split although k % 256 == 0
    # ---- dx on the MFMA form, two workgroups per tile ----------------------------------------------------------------------------------
    Case("dxm2_k256", 2, 3, 31, 4, 8, 256, (2, 2, 2)),            # 1 chunk per wave
    Case("dxm2_k512", 2, 3, 1, 4, 8, 512, (2, 2, 2)),             # 2 chunks
    Case("dxm2_k1024", 2, 3, 64, 4, 8, 1024, (2, 2, 2)),          # 4 chunks: an exact ring
    Case("dxm2_tiles255", 1, 1, 8, 15, 544, 256, (2, 2, 2)),      # rows / 32 = 255: the partner of dxm1_tiles256
    # ---- dC on the MFMA form (k = 32: one block; k = 96: three), dx wherever the map sends it --------------------------------------------
    Case("dcm_v16_k32", 1, 3, 64, 4, 4, 32, (1, 2, 1)),           # 1 step per wave: the ring overruns 15, past the end of ddist / xt
    Case("dcm_v16_k96", 2, 3, 33, 2, 4, 96, (1, 2, 1)),
    Case("dcm_v48_k32", 3, 3, 32, 4, 4, 32, (1, 2, 1)),           # 3 steps; slices of 6 vectors cross the images of 16
    Case("dcm_v48_k96", 3, 2, 31, 4, 4, 96, (1, 2, 1)),
    Case("dcm_v256_k32", 2, 3, 1, 8, 16, 32, (1, 2, 1)),          # 16 steps: an exact ring (hw = 128, but k = 32: dx tiled)
    Case("dcm_v256_k96", 4, 3, 64, 8, 8, 96, (1, 2, 1)),
    Case("dcm_v272_k32", 8, 3, 64, 2, 17, 32, (0, 2, 1)),         # 17 steps: a whole ring and a tail of 1 (hw = 34: dx lane-per-channel)
    Case("dcm_v272_k96", 8, 2, 33, 2, 17, 96, (0, 2, 1)),
    Case("dcm_v528_k32", 3, 3, 32, 11, 16, 32, (1, 2, 1)),        # 66 vectors per wave: a second scan pass with 2 live lanes
    Case("dcm_v528_k96", 3, 2, 64, 11, 16, 96, (1, 2, 1)),
    # ---- mixed routes ------------------------------------------------------------------------------------------------------------------
    Case("mix_hw16_k128", 2, 3, 64, 4, 4, 128, (1, 2, 1)),        # dx tiled, dC MFMA
    Case("mix_both_1x1", 1, 1, 64, 4, 8, 128, (2, 2, 1)),         # one image, one group: both MFMA (V = 32)
    Case("mix_hw9_k128", 2, 3, 64, 3, 3, 128, (0, 1, 1)),         # an odd map: neither MFMA form
    # ---- the tiled forms ----------------------------------------------------------------------------------------------------------------
    Case("til_k16", 2, 3, 64, 2, 4, 16, (1, 1, 1)),               # one codeword per dx slice step; one dC workgroup a group
    Case("til_k48", 3, 2, 33, 2, 4, 48, (1, 1, 1)),
    Case("til_k128", 1, 3, 32, 2, 4, 128, (1, 1, 1)),             # V = 8: no whole vector pairs for eight dC waves
    Case("til_dc_v3", 3, 3, 31, 1, 1, 16, (0, 1, 1)),             # fewer vectors than dC waves
    Case("til_dc_v5", 1, 3, 1, 1, 5, 48, (0, 1, 1)),              # 2 + 2 + 1 + 0: the last dC wave's range is empty
    # ---- the lane-per-channel forms ----------------------------------------------------------------------------------------------------
    Case("lane_d65_k100", 2, 3, 65, 3, 5, 100, (0, 0, 1)),        # hw = 15; k = 100: two runs of 64, the second partial
    Case("lane_d80_k128", 2, 2, 80, 4, 8, 128, (0, 0, 1)),        # a shape both MFMA forms would take but for d
    Case("lane_k5", 2, 3, 16, 3, 5, 5, (0, 0, 1)),
    Case("lane_d64_k100", 1, 3, 64, 3, 5, 100, (0, 0, 1)),
]

BY_NAME = {c.name: c for c in CASES}
RING_DX, RING_DC = "dxm1_k640", "dcm_v272_k96"                    # the cases of the ring-mask tests

REFUSED = [(0, 3, 64, 4, 8, 128), (2, 0, 64, 4, 8, 128), (2, 3, 0, 4, 8, 128), (2, 3, 64, 0, 8, 128), (2, 3, 64, 4, 0, 128), (2, 3, 64, 4, 8, 0),
           (-1, 3, 64, 4, 8, 128), (2, 3, 64, 4, 8, -128),
           (32768, 1, 1, 256, 256, 8)]                            # rows = 2^31


def dims(case):
    return case.n, case.m, case.d, case.h, case.w, case.k


def seed(case):
    return 6000 + 13 * sum(ord(ch) for ch in case.name)


def index_pattern(n, m, h, w, k):
    """The sampled codewords [N, m, h, w] (int64), built so that the straight-through scatter is covered, not sampled.  The V = N h w
    vectors of group g, in (image, pixel) order, walk the codewords upwards from 29 + 11 g (mod k): vectors 0 and 1 share the start,
    vector j in 2 .. V - 2 takes start + j - 1, the last vector returns to the start.  So the start codeword is hit twice inside the
    first 64-vector scan pass of the first wave slice and once more from the last slice; the walk starts three codewords below a
    32-block's end and crosses it (c0 - 1 and c0 + 32 of the neighbours are hit); with V >= k + 2 every codeword of the group is
    hit, below that the V - 2 positions after a start that differs from group to group."""
    v = n * h * w
    out = torch.empty((n, m, h * w), dtype=torch.int64)
    for g in range(m):
        j = torch.arange(v)
        walk = torch.where((j == 0) | (j == v - 1), torch.zeros_like(j), (j - 1).clamp_min(0))
        out[:, g, :] = ((29 + 11 * g + walk) % k).reshape(n, h * w)
    return out.reshape(n, m, h, w)


def scatter_hits(case):
    """hits[g][c]: how many vectors of group g sample codeword c under index_pattern."""
    idx = index_pattern(case.n, case.m, case.h, case.w, case.k).reshape(case.n, case.m, -1)
    return torch.stack([torch.bincount(idx[:, g].reshape(-1), minlength=case.k) for g in range(case.m)])
