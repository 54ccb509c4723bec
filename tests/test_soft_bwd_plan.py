"""CPU: the routing of mcq_vq_soft_bwd_f32 (vq_soft_bwd_route of csrc/vq_train.hip: pure host code) through mcq_vq_soft_bwd_plan --
the decision the entry point itself launches by, not a copy of it.

(a) every case of tests/_soft_bwd_cases.py takes the route its literal says, and the table reaches every (form, split) row by the
    counts written out here, so that an edit of the table or of the routing cannot shrink what tests/test_gpu_soft_bwd_leaf.py
    covers unnoticed;
(b) over a few thousand shapes: what the kernels of a form read without a check holds wherever the plan names that form;
(c) the index pattern of the cases covers the straight-through scatter of vq_dc_mfma_kernel as the literals here say."""
import ctypes
import random

import pytest

import _soft_bwd_cases as K


@pytest.fixture(scope="module")
def lib():
    from mcquic_amd import _lib
    return _lib.load()


def plan(lib, n, m, d, h, w, k):
    """(dx_form, dc_form, dx_split), or None for a shape the entry point refuses."""
    out = (ctypes.c_int32 * 3)(-1, -1, -1)
    ok = lib.mcq_vq_soft_bwd_plan(n, m, d, h, w, k, out)
    assert ok in (0, 1)
    if not ok:
        assert list(out) == [-1, -1, -1], "a refused query wrote its output"
        return None
    return tuple(out)


@pytest.mark.parametrize("case", K.CASES, ids=[c.name for c in K.CASES])
def test_case_route(lib, case):
    assert plan(lib, *K.dims(case)) == case.plan


def test_table_reaches_every_form():
    names = [c.name for c in K.CASES]
    assert len(set(names)) == len(names) == 30
    count = lambda pred: sum(1 for c in K.CASES if pred(c.plan))
    # the seven rows of the launcher's table, as literal counts
    assert count(lambda p: p[0] == 2 and p[2] == 1) == 5             # vq_dx_mfma_kernel, one workgroup per tile
    assert count(lambda p: p[0] == 2 and p[2] == 2) == 4             # vq_dx_mfma_kernel, two workgroups per tile + vq_zero_kernel
    assert count(lambda p: p[0] == 1) == 12                          # vq_dx_tiled_kernel
    assert count(lambda p: p[0] == 0) == 9                           # vq_dx_kernel
    assert count(lambda p: p[1] == 2) == 20                          # vq_dc_mfma_kernel
    assert count(lambda p: p[1] == 1) == 6                           # vq_dc_tiled_kernel
    assert count(lambda p: p[1] == 0) == 4                           # vq_dc_kernel
    assert all(p[2] == 1 for p in (c.plan for c in K.CASES) if p[0] != 2)
    # the mixed routes and the edges the cases are there for
    pairs = {c.plan[:2] for c in K.CASES}
    assert pairs == {(2, 2), (1, 2), (0, 2), (0, 1), (1, 1), (0, 0)}
    mfma_dx = [c for c in K.CASES if c.plan[0] == 2]
    assert {c.k // (16 * c.plan[2]) // 8 for c in mfma_dx if c.plan[2] == 1} == {1, 2, 3, 5}         # chunks per wave (2: dxm1_tiles256)
    assert {c.k // (16 * c.plan[2]) // 8 for c in mfma_dx if c.plan[2] == 2} == {1, 2, 4}
    assert {c.n * c.m * c.h * c.w // 32 for c in mfma_dx if c.k == 256} >= {255, 256}
    mfma_dc = [c for c in K.CASES if c.plan[1] == 2]
    assert {c.n * c.h * c.w // 16 for c in mfma_dc} >= {1, 3, 16, 17, 33}                         # ring steps per wave
    assert {c.k for c in mfma_dc} >= {32, 96}
    for cases in (mfma_dx, mfma_dc):
        assert {c.d for c in cases} >= {64, 33, 32, 31, 1}
    assert {c.d for c in K.CASES if c.plan == (0, 0, 1)} >= {65, 80} and {c.k for c in K.CASES if c.plan == (0, 0, 1)} >= {5, 100}
    assert {c.k for c in K.CASES if c.plan[0] == 1 and c.h * c.w == 8} >= {16, 48, 128}
    assert {c.n * c.h * c.w for c in K.CASES if c.plan[1] == 1} >= {3, 5} and {c.k for c in K.CASES if c.plan[1] == 1} >= {16, 48, 128}
    assert all(K.BY_NAME[n].plan[i] == 2 for n, i in ((K.RING_DX, 0), (K.RING_DC, 1)))
    assert sum(1 for c in K.CASES if c.m >= 3 or c.n >= 2) == 27      # (one image and one group only where the edge needs it)


def test_refusals(lib):
    for shape in K.REFUSED:
        assert plan(lib, *shape) is None, shape
    assert lib.mcq_vq_soft_bwd_plan(2, 3, 64, 4, 8, 128, None) == 0      # no output
    assert plan(lib, 32767, 1, 1, 256, 256, 8) == (0, 0, 1)              # rows = 2^31 - 65536: taken, and too large for a buffer resource
    p = ctypes.c_void_p(64)                                             # never dereferenced: the checks come first
    from mcquic_amd import _lib
    for shape, status in ((K.REFUSED[0], _lib.MCQ_EINVAL), (K.REFUSED[-2], _lib.MCQ_EINVAL), (K.REFUSED[-1], _lib.MCQ_ETOOLARGE)):
        assert lib.mcq_vq_soft_bwd_f32(p, p, p, p, p, p, p, p, p, p, *shape, None) == status, shape
    assert lib.mcq_vq_soft_bwd_f32(None, p, p, p, p, p, p, p, p, p, 2, 3, 64, 4, 8, 128, None) == _lib.MCQ_EINVAL


def _random_shapes(count):
    rng = random.Random(1313)
    shapes = set()
    while len(shapes) < count:
        r = rng.random()
        if r < 0.45:                                                 # around the MFMA conditions
            n, m, d = rng.randint(1, 9), rng.choice((1, 2, 3, 12)), rng.choice((1, 8, 31, 32, 33, 63, 64, 65, 80, 128))
            h, w = rng.choice((1, 2, 3, 4, 8, 15, 16, 17, 32, 64)), rng.choice((1, 2, 4, 8, 16, 17, 34, 128, 544))
            k = rng.choice((16, 32, 48, 96, 100, 128, 256, 384, 512, 640, 1024, 8192))
        elif r < 0.9:                                                # anything small
            n, m, d, h, w, k = rng.randint(1, 16), rng.randint(1, 4), rng.randint(1, 96), rng.randint(1, 40), rng.randint(1, 40), rng.randint(1, 1100)
        else:                                                        # around the 2 GiB windows of the buffer resources
            n, m, d = rng.choice((8, 64, 512, 4096)), rng.choice((1, 2, 16)), rng.choice((16, 64))
            h, w, k = rng.choice((16, 64, 256)), rng.choice((16, 64, 256)), rng.choice((128, 1024, 8192, 65536))
        shapes.add((n, m, d, h, w, k))
    return sorted(shapes)


def test_plan_invariants_sweep(lib):
    seen = set()
    for n, m, d, h, w, k in _random_shapes(4000):
        p = plan(lib, n, m, d, h, w, k)
        hw, v, rows = h * w, n * h * w, n * m * h * w
        what = f"{(n, m, d, h, w, k)}: {p}"
        if p is None:
            assert rows > 2 ** 31 - 1, what
            continue
        dxf, dcf, split = p
        assert dxf in (0, 1, 2) and dcf in (0, 1, 2) and split in (1, 2), what
        seen.add(p)
        if dxf == 2:
            # whole 32-row tiles of one (image, group); wave slices of whole 8-codeword chunks; 32-bit byte offsets into ddist and the codebook
            assert d <= 64 and hw % 32 == 0 and k % (16 * split) == 0 and k // (16 * split) % 8 == 0, what
            assert rows * k * 4 < 2 ** 31 and m * k * d * 4 < 2 ** 31, what
            assert split == (2 if rows // 32 < 256 and k % 256 == 0 else 1), what
        else:
            assert split == 1, what
        if dxf == 1:
            assert d <= 64 and hw % 8 == 0 and k % 16 == 0, what
        if dcf == 2:
            # whole vector pairs per wave slice, pairs inside one image; whole 32-codeword blocks; 32-bit byte offsets into ddist and xt
            assert d <= 64 and k % 32 == 0 and hw % 2 == 0 and v % 16 == 0, what
            assert rows * k * 4 < 2 ** 31 and v * m * d * 4 < 2 ** 31, what
        if dcf == 1:
            assert d <= 64 and k % 16 == 0, what
        # no form is passed over: a shape a faster form takes is not left to a slower one
        fits = rows * k * 4 < 2 ** 31
        if d <= 64 and hw % 32 == 0 and k % 128 == 0 and fits and m * k * d * 4 < 2 ** 31:
            assert dxf == 2, what
        elif d <= 64 and hw % 8 == 0 and k % 16 == 0:
            assert dxf == 1, what
        else:
            assert dxf == 0, what
        if d <= 64 and k % 32 == 0 and hw % 2 == 0 and v % 16 == 0 and fits and v * m * d * 4 < 2 ** 31:
            assert dcf == 2, what
        elif d <= 64 and k % 16 == 0:
            assert dcf == 1, what
        else:
            assert dcf == 0, what
    assert {(a, s) for a, _, s in seen} == {(0, 1), (1, 1), (2, 1), (2, 2)} and {b for _, b, _ in seen} == {0, 1, 2}, seen


# ---- (c) the straight-through scatter of vq_dc_mfma_kernel -----------------------------------------------------------------------------------
# A case with V >= k + 2 hits EVERY codeword of every 32-block in every group; the others hit the V - 2 codewords after a start that
# differs by group -- that many of a block's 32 accumulator places (register x half).  Which case is which is a literal below.
def test_index_pattern_covers_the_scatter():
    full = set()
    for c in K.CASES:
        if c.plan[1] != 2:
            continue
        hits = K.scatter_hits(c)
        v, per = c.n * c.h * c.w, c.n * c.h * c.w // 8
        assert int(hits.sum()) == v * c.m
        for g in range(c.m):
            start = (29 + 11 * g) % c.k
            # the start codeword: vectors 0 and 1 (one scan pass of wave 0) and the last vector (wave 7), on top of the walk's own visits
            assert int(hits[g, start]) >= 3 and per >= 2, c.name
            assert int((hits[g] > 0).sum()) == min(v - 2, c.k), c.name
        # group 0's walk crosses a block's end: codeword 31 and codeword 32 (0 where k = 32) -- c0 - 1 and c0 + 32 of each other's neighbour
        assert int(hits[0, 31]) > 0 and int(hits[0, 32 % c.k]) > 0, c.name
        if bool((hits > 0).all()):
            full.add(c.name)
    assert full == {"dxm1_tiles256", "dxm2_tiles255", "dcm_v48_k32", "dcm_v256_k32", "dcm_v256_k96", "dcm_v272_k32", "dcm_v272_k96",
                    "dcm_v528_k32", "dcm_v528_k96"}
    # the small cases together: every one of the 32 places of a block is hit in some group of some case with V < k + 2
    places = set()
    for c in K.CASES:
        if c.plan[1] == 2 and c.name not in full:
            hits = K.scatter_hits(c)
            places |= {int(i) % 32 for g in range(c.m) for i in hits[g].nonzero().reshape(-1)}
    assert len(places) == 32
