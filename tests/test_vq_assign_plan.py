"""CPU: the launch plan of the assignment kernel (vq_assign_plan of csrc/vq.hip: pure host code) through mcq_vq_assign_plan -- the
decision vq_assign_launch and mcq_vq_assign_workspace_bytes themselves take, not a copy of it.

(a) every case of tests/_vq_assign_cases.py takes the plan its literal says, and the table reaches every <SPC, XLDS, RATE> instance,
    slice split, range count and block shape by the counts written out here, so that an edit of the table or of the planner cannot
    shrink what tests/test_gpu_vq_assign_leaf.py covers unnoticed;
(b) over a few thousand random shapes and over every tile count 1 .. 72: what the kernel relies on without a check holds wherever the
    plan says so, and the launch runs exactly the codeword ranges whose first slice owns a tile;
(c) the bar of the GPU test is honest: the kernel's float32 sequence, emulated in NumPy on the very inputs the GPU test draws, stays
    inside the rounding bound at every position and under the 1 % cap of excused positions."""
import ctypes
import random

import numpy as np
import pytest

import _rate_map_ref as MR
import _rate_ref as RR
import _vq_assign_cases as K


@pytest.fixture(scope="module")
def lib():
    from mcquic_amd import _lib
    return _lib.load()


def plan(lib, n, m, d, h, w, k, rate=0):
    """(instance, Sp, cs_log2, zs, bw_log2, vector_tiles), or None for a shape the entry points refuse."""
    out = (ctypes.c_int32 * 6)(*[-1] * 6)
    ok = lib.mcq_vq_assign_plan(n, m, d, h, w, k, rate, out)
    assert ok in (0, 1)
    if not ok:
        assert list(out) == [-1] * 6, "a refused query wrote its output"
        return None
    return tuple(out)


@pytest.mark.parametrize("case", K.CASES, ids=[c.name for c in K.CASES])
def test_case_plan(lib, case):
    geo = K.geometry(case)
    for rate in (0, 1):                                              # the rate operand picks the kernel's form, not its plan
        instance, steps, cs_log2, zs, bw_log2, vtiles = plan(lib, *K.dims(case), rate=rate)
        assert (instance, cs_log2, zs, bw_log2) == case.plan
        assert steps == K.sp(case.d) and vtiles == geo["vtiles"]
    nvec = case.n * case.m * case.h * case.w
    assert lib.mcq_vq_assign_workspace_bytes(*K.dims(case)) == (case.plan[2] * nvec * 8 if case.plan[2] > 1 else 0)


def test_instance_constants_are_the_headers():
    from mcquic_amd import _lib
    assert (_lib.MCQ_VQ_ASSIGN_LOOP, _lib.MCQ_VQ_ASSIGN_SP8, _lib.MCQ_VQ_ASSIGN_SP32, _lib.MCQ_VQ_ASSIGN_SP128,
            _lib.MCQ_VQ_ASSIGN_SP128_LDS) == (K.LOOP, K.SP8, K.SP32, K.SP128, K.LDS) == (0, 1, 2, 3, 4)
    V, I = ctypes.c_void_p, ctypes.c_int32
    assert _lib.SYMBOLS["mcq_vq_assign_plan"] == (I, [I, I, I, I, I, I, I, V])
    assert _lib.MCQ_ABI_VERSION == 18                                # additive


def launch_table():
    """{(instance, RATE): [case names]}: which cases launch each of the ten instantiations of vq_assign_kernel in a form they name."""
    table = {(inst, rate): [] for inst in K.INSTANCE_NAMES for rate in (False, True)}
    for c in K.CASES:
        for rate in (False, True):
            if K.runs(c, "rate" if rate else "plain"):
                table[(c.plan[0], rate)].append(c.name)
    return table


def test_table_reaches_every_instance(capsys):
    names = [c.name for c in K.CASES]
    assert len(set(names)) == len(names) == 26
    assert [c.forms for c in K.CASES].count("both") == 15 and [c.forms for c in K.CASES].count("rate") == 3
    table = launch_table()
    with capsys.disabled():
        for (inst, rate), cases in sorted(table.items()):
            print(f"\nvq_assign_kernel{K.INSTANCE_NAMES[inst][:-1]}, {'true' if rate else 'false'}>: {', '.join(cases)}", end="")
        print()
    # the ten instantiations, as literal counts (plain, rate)
    assert {key: len(v) for key, v in table.items()} == {
        (K.SP8, False): 9, (K.SP8, True): 7, (K.LOOP, False): 3, (K.LOOP, True): 4, (K.SP32, False): 6, (K.SP32, True): 4,
        (K.SP128, False): 2, (K.SP128, True): 2, (K.LDS, False): 3, (K.LDS, True): 1}
    assert table[(K.LOOP, True)] == ["loop_d24_rate", "loop_d100_empty_slice", "loop_d33_ranged", "loop_d24_ranged_rate"]
    assert table[(K.SP128, True)] == ["sp128_d241", "sp128_d256_3_tiles"] and table[(K.LDS, True)] == ["lds_d241_ranged"]
    count = lambda pred: sum(1 for c in K.CASES if pred(c))          # noqa: E731
    # slices, ranges, block shapes
    assert [count(lambda c, v=v: c.plan[1] == v) for v in (0, 1, 2)] == [3, 8, 15]
    assert [count(lambda c, v=v: c.plan[2] == v) for v in (1, 2, 4, 8, 16)] == [16, 5, 2, 1, 2]
    assert [count(lambda c, v=v: c.plan[3] == v) for v in (2, 3, 4, 5)] == [1, 16, 6, 3]
    # every ranged case with d <= 64 also runs under the rate term; ranging meets every instance that can take four slices
    assert all(K.runs(c, "rate") for c in K.CASES if c.plan[2] > 1 and c.d <= 64)
    assert {c.plan[0] for c in K.CASES if c.plan[2] > 1 and K.runs(c, "rate")} == {K.SP8, K.LOOP, K.SP32, K.LDS}
    geo = {c.name: K.geometry(c) for c in K.CASES}
    # a slice (or a whole range's tail) that owns no codeword tile
    assert [c.name for c in K.CASES if geo[c.name]["empty"]] == ["sp8_empty_range", "loop_d100_empty_slice", "loop_d33_ranged", "loop_d24_ranged_rate",
                                                                  "sp32_7_empty_ranges", "lds_d256_empty_slice"]
    # ... and whole ranges that are dealt none: they are not launched (the sweeps below say where that happens)
    assert {c.name: (geo[c.name]["launched"], c.plan[2]) for c in K.CASES if geo[c.name]["launched"] != c.plan[2]} == {
        "sp8_empty_range": (3, 4), "sp32_7_empty_ranges": (9, 16)}
    # an odd block count: the last wave holds one real block and one clamped copy
    assert count(lambda c: geo[c.name]["blocks"] % 2 == 1) == 13
    assert {geo[c.name]["blocks"] for c in K.CASES} >= {1, 2, 9, 15, 45, 2048}
    # waves with no vector tile: they leave at once when unsliced (2 cases), stay for the barrier when sliced (5)
    assert count(lambda c: geo[c.name]["inactive_waves"] > 0 and c.plan[1] == 0) == 2
    assert count(lambda c: geo[c.name]["inactive_waves"] > 0 and c.plan[1] > 0) == 5
    assert count(lambda c: geo[c.name]["partial_blocks"]) == 25 and not geo["sp8_2048_waves"]["partial_blocks"]
    # an unrolled instance below its full vector length: the channels past d come from the descriptor's range check
    below = {inst: sorted(c.d for c in K.CASES if c.plan[0] == inst and c.d < K.WINDOWS[inst][1]) for inst in K.WINDOWS}
    assert below == {K.SP8: [1, 2, 3, 3, 4, 5, 7, 8, 9], K.SP32: [49, 50, 63], K.SP128: [241], K.LDS: [241, 255]}
    assert count(lambda c: c.plan[0] in K.WINDOWS and K.WINDOWS[c.plan[0]][0] < c.d < K.WINDOWS[c.plan[0]][1]) == 11    # strictly inside
    assert all(K.WINDOWS[c.plan[0]][0] <= c.d <= K.WINDOWS[c.plan[0]][1] for c in K.CASES if c.plan[0] in K.WINDOWS)
    assert {c.d for c in K.CASES if c.plan[0] == K.LOOP} == {17, 24, 33, 100}                                          # both loop windows
    assert {c.d % 2 for c in K.CASES if K.runs(c, "rate")} == {0, 1} and {c.m for c in K.CASES} == {1, 2} and {c.n for c in K.CASES} == {1, 2, 3}
    assert {(m, k, d) for m, k, d in K.PACK_CASES} == {(1, 5, 1), (2, 129, 7), (1, 200, 49), (1, 384, 241)}


def test_refusals(lib):
    from mcquic_amd import _lib
    for shape in K.REFUSED:
        assert plan(lib, *shape) is None and plan(lib, *shape, rate=1) is None, shape
        assert lib.mcq_vq_assign_workspace_bytes(*shape) == 0, shape
    assert lib.mcq_vq_assign_plan(1, 1, 8, 4, 4, 128, 0, None) == 0        # no output
    assert plan(lib, 1, 1, 8, 4, 4, 128, rate=2) is None and plan(lib, 1, 1, 8, 4, 4, 128, rate=-1) is None
    # the neighbours of the two size limits are taken
    assert plan(lib, 1, 2, 64, 4096, 2047, 512) is not None
    assert plan(lib, (1 << 20) - 1, 1, 1, 256, 256, 8) == (K.SP8, 8, 0, 1, 5, (1 << 30) - 1024)
    # the entry points refuse the same shapes with the status of before (the pointers are never dereferenced: the checks come first)
    p = ctypes.c_void_p(64)
    for shape, status in ((K.REFUSED[0], _lib.MCQ_EINVAL), (K.REFUSED[-3], _lib.MCQ_EINVAL), (K.REFUSED[-2], _lib.MCQ_ETOOLARGE),
                          (K.REFUSED[-1], _lib.MCQ_ETOOLARGE)):
        assert lib.mcq_vq_assign_ws_f32(p, p, p, *shape, None, None) == status, shape
        assert lib.mcq_vq_assign_f32(p, p, p, *shape, None) == status, shape
        assert lib.mcq_vq_assign_rate_map_f32(p, p, p, p, 1, 0, 0, p, *shape, None, None) == status, shape


def _random_shapes(count):
    rng = random.Random(2424)
    shapes = set()
    while len(shapes) < count:
        r = rng.random()
        if r < 0.5:                                                  # around the windows of the instances and the tile counts of the splits
            n, m = rng.randint(1, 4), rng.choice((1, 2, 3, 12))
            d = rng.choice((1, 2, 15, 16, 17, 32, 47, 48, 49, 63, 64, 65, 128, 239, 240, 241, 255, 256, 257, 300))
            h, w = rng.choice((1, 2, 3, 5, 8, 9, 16, 33, 64)), rng.choice((1, 2, 3, 4, 7, 8, 15, 16, 17, 31, 32, 33, 70, 128))
            k = rng.choice((1, 5, 127, 128, 129, 256, 257, 384, 385, 512, 640, 896, 897, 1024, 1100, 2048, 2305, 3072, 4096, 4224, 6500, 8192, 9000))
        elif r < 0.9:                                                # anything small, k over the whole ranged regime
            n, m, d, h, w, k = rng.randint(1, 8), rng.randint(1, 4), rng.randint(1, 270), rng.randint(1, 40), rng.randint(1, 40), rng.randint(1, 9216)
        else:                                                        # many vectors: whole rounds of waves, no ranging
            n, m, d = rng.choice((8, 32, 256)), rng.choice((1, 2, 12)), rng.choice((4, 16, 64, 256))
            h, w, k = rng.choice((16, 64, 256)), rng.choice((16, 48, 256)), rng.choice((128, 512, 2048, 8192))
        shapes.add((n, m, d, h, w, k))
    return sorted(shapes)


def _check_plan(lib, shape, seen, trimmed):
    """Every invariant of one shape's plan; records (instance, cs_log2, zs, bw_log2) and, where fewer ranges are launched than the
    tiles are dealt over, trimmed[(CS, zs, launched)] += {ntile}."""
    n, m, d, h, w, k = shape
    p = plan(lib, n, m, d, h, w, k)
    what = f"{shape}: {p}"
    assert p is not None and p == plan(lib, n, m, d, h, w, k, rate=1), what
    instance, steps, cs_log2, zs, bw_log2, vtiles = p
    ntile, cs = (k + 127) // 128, 1 << cs_log2
    seen.add((instance, cs_log2, zs, bw_log2))
    # the ring: whole rounds of VQ_PF k-steps that cover every channel pair, with less than one round of padding
    assert steps % K.RING == 0 and 2 * steps >= d > 2 * (steps - K.RING), what
    assert instance == {8: K.SP8, 32: K.SP32, 128: K.LDS if cs_log2 == 2 else K.SP128}.get(steps, K.LOOP), what
    if instance in K.WINDOWS:
        assert K.WINDOWS[instance][0] <= d <= K.WINDOWS[instance][1], what
    # the staged instance is compiled for four slices a workgroup (one vector tile), and takes every d = 241..256 shape that has them
    assert (instance == K.LDS) == (steps == 128 and ntile >= 4), what
    # slices and ranges: no more slices than tiles; zs a power of two up to 16, never more ranges than tiles per slice
    assert cs_log2 in (0, 1, 2) and cs <= ntile, what
    assert zs in (1, 2, 4, 8, 16), what
    assert zs == 1 or (ntile >> cs_log2) >= zs, what
    # The kernel deals per_slice = ceil(ntile / (CS zs)) tiles to every (range, slice) in order: range z owns a tile iff
    # z CS per_slice < ntile.  The launch runs `launched` ranges (the header's rule, `_vq_assign_cases.launched_ranges`;
    # tests/test_gpu_vq_assign_leaf.py sees in the workspace that exactly those ran): every one of them starts with a tile in its first
    # slice -- the slice that folds its workgroup and writes --, the next one would not, and more than half of zs remain.
    per_slice = (ntile + cs * zs - 1) // (cs * zs)
    launched = K.launched_ranges(ntile, cs_log2, zs)
    assert 1 <= launched <= zs and 2 * launched > zs, what
    assert all(z * cs * per_slice < ntile for z in range(launched)), what
    assert launched * cs * per_slice >= ntile, what
    if launched < zs:
        trimmed.setdefault((cs, zs, launched), set()).add(ntile)
    # blocks of 32 pixels; a vector tile is two of them
    assert bw_log2 in (2, 3, 4, 5), what
    bw, bh = 1 << bw_log2, 32 >> bw_log2
    assert vtiles == (n * ((w + bw - 1) // bw) * ((h + bh - 1) // bh) + 1) // 2, what
    assert zs == 1 or (vtiles * m << cs_log2) * (zs // 2) < 1536, what      # ranging stops once ~1536 waves exist
    assert lib.mcq_vq_assign_workspace_bytes(n, m, d, h, w, k) == (zs * n * m * h * w * 8 if zs > 1 else 0), what


def test_plan_invariants_sweep(lib):
    seen, trimmed = set(), {}
    for shape in _random_shapes(4000):
        _check_plan(lib, shape, seen, trimmed)
    assert {s[0] for s in seen} == {K.LOOP, K.SP8, K.SP32, K.SP128, K.LDS} and {s[1] for s in seen} == {0, 1, 2}, seen
    assert {s[2] for s in seen} == {1, 2, 4, 8, 16} and {s[3] for s in seen} == {2, 3, 4, 5}, seen
    assert {key[1] for key in trimmed} == {4, 8, 16}, trimmed            # the sweep reaches trimmed launches at every zs that has them


def test_every_tile_count(lib):
    """Every tile count 1 .. 72 (k = 128 t - 127 and 128 t), for launches from one vector to thousands of waves and a vector length of
    every instance: the invariants, and as a literal where the launch runs fewer ranges than the tiles are dealt over -- whenever
    CS zs per_slice overshoots ntile by a whole range, {(CS, zs, launched): tile counts}."""
    seen, trimmed = set(), {}
    for n, h, w, m in ((1, 1, 1, 1), (1, 8, 8, 1), (1, 16, 24, 2), (2, 32, 48, 2), (8, 64, 64, 2), (32, 48, 32, 12)):
        for d in (4, 33, 64, 256):
            for t in range(1, 73):
                for k in (128 * t - 127, 128 * t):
                    _check_plan(lib, (n, m, d, h, w, k), seen, trimmed)
    assert {s[1] for s in seen} == {0, 1, 2} and {s[2] for s in seen} == {1, 2, 4, 8, 16}, seen
    span = lambda a, b: set(range(a, b + 1))                             # noqa: E731
    assert trimmed == {(4, 4, 3): span(17, 24) | span(33, 36),           # 2 tiles a slot; 3 a slot where the waves stop zs at 4
                       (4, 8, 5): span(33, 40), (4, 8, 6): span(41, 48), (4, 8, 7): span(49, 56),
                       (4, 16, 9): span(65, 72)}, trimmed


# ---- (c) the cap is honest --------------------------------------------------------------------------------------------------------------------
EMULATED = [c for c in K.CASES if c.k * c.n * c.h * c.w * c.m <= 5e6]


def test_only_the_large_case_is_left_to_the_gpu():
    assert [c.name for c in K.CASES if c not in EMULATED] == ["sp8_2048_waves"]      # 34 M costs: its paths are sp8_full_tile's


@pytest.mark.parametrize("case", EMULATED, ids=[c.name for c in EMULATED])
def test_float32_sequence_stays_under_the_excuse_cap(case):
    x, cb, cdf, lam = K.gaussian_case(case)
    bits = RR.penalty_table(cdf)
    assert np.isfinite(bits).all()
    if K.runs(case, "plain"):
        got = RR.emulate_assign_f32(x, cb, RR.c2_f32(cb))
        differ, unexcused = K.audit_rows(x, cb, bits, None, got)
        assert unexcused == 0 and differ <= RR.EXCUSED_CAP * got.size, (case.name, "plain", differ, unexcused, got.size)
    if K.runs(case, "rate"):
        got = MR.emulate_assign_f32(x, cb, cdf, lam)
        differ, unexcused = K.audit_rows(x, cb, bits, lam, got)
        assert unexcused == 0 and differ <= RR.EXCUSED_CAP * got.size, (case.name, "rate", differ, unexcused, got.size)
        if got.size > 8:
            assert not np.array_equal(got, MR.emulate_assign_f32(x, cb, cdf, np.zeros_like(lam))), "the lambdas change nothing: the case tests no rate term"


def test_integer_inputs_are_exact_in_float32():
    """The premise of the GPU file's exact tests, checked here on every case: with integer inputs in [-4, 4] every partial sum of the
    kernel (|x|^2, |c|^2 <= 16 d, |<x, c>| <= 16 d, the distance <= 64 d, plus lambda bits <= 48 in quarters) is an integer or a multiple
    of 1/4 far below 2^24, so the float32 sequence equals the float64 argmin at EVERY position -- and ties are everywhere."""
    for case in K.CASES:
        assert 64 * case.d + 4 * 48 < 2 ** 22                        # in quarters: below 2^24
    ties = 0
    for case in (K.BY_NAME[n] for n in ("sp8_k129_two_slices", "loop_d24_rate", "sp32_d49", "lds_d241_ranged", "sp8_zs16")):
        x, cb, cdf, lam = K.integer_case(case)
        bits = RR.penalty_table(cdf)
        assert np.array_equal(bits, np.round(bits)) and bits.min() >= 4 and bits.max() <= 16
        want = K.argmin_rows(x, cb, bits, lam)
        assert np.array_equal(MR.emulate_assign_f32(x, cb, cdf, lam), want)
        assert np.array_equal(RR.emulate_assign_f32(x, cb, RR.c2_f32(cb)), K.argmin_rows(x, cb, None, None))
        cost = MR.costs(x, cb, bits, lam)
        ties += int((np.sort(cost, -1)[..., 0] == np.sort(cost, -1)[..., 1]).sum())
    assert ties >= 20, ties
