"""The cases of the weight-gradient leaf tests, shared by tests/test_wgrad_refs.py (the references at these geometries),
tests/test_wgrad_plan.py (the branch table: which plan features a case exercises, asserted against mcq_conv2d_wgrad_nchw_plan) and
tests/test_gpu_wgrad_leaf.py (the launches).  Imports nothing of mcquic_amd.

Cin 20 / Cout 40: one ragged 32-tile in each axis (72 / 40 for the 64 x 64 tile of the 1x1 walk); 3 input channels: the stem.

A case: name, form, (N, Cin, H, W, Cout) with H, W the INPUT map, kernel size, stride, the `nconv` values it is launched with, and for
the strip-walk forms `plan`: nconv -> the literal of what the launch's plan has

    F        floats a lane reads per row (4 or 8)
    chunks   several row ranges per (image, strip)            (row_chunks > 1)
    ups      a wave owns several walks                        (ups > 1)
    ragged   the last workgroup has waves without a walk      (splits % 4 != 0)
    whole    the launch was planned as a whole                (3x3 stride 1 with at least 32 strip-rows: the second search of rows_plan_search)
    grouped  nconv > 1 only: "same" -- the one-by-one plan; "shared" -- the shared wave budget of the small-map path changed it;
             "whole" -- the whole-launch search cut the launch differently because of nconv

Forms: rows3 / s2 / rows1 -- the strip walks of csrc/wgrad_rows.hip (workspace query > 1); tiny -- its small-map LDS kernel (query == 1,
channels not in sixteens); t16_3 / t16_1 -- the 16 x 16-tile kernel of csrc/wgrad_t16.h (query == 1); nhwc -- every row query == 0:
mcq_nchw_to_nhwc_pair_f32 + mcq_conv2d_wgrad_f32 (csrc/train_ops.hip).

The gmax fall-back of a grouped launch (a grouped plan with more groups than the workspace query sizes by runs the one-by-one plan)
has no case: it cannot be reached.  Where the whole-launch search does not apply (fewer than 32 strip-rows) the wave budget is at
most 7, the shared one 4 .. 6, and over every (images x strips, rows) with fewer than 32 strip-rows the shared plan has fewer walks per
range and never more groups; where it applies the search itself only admits cuts within gmax, and a grouped search finds a cut
whenever the one-by-one search does.  test_wgrad_plan.py's sweep asserts what the fall-back is there for (groups <= gmax, the
launch inside nconv x the one-problem workspace) over a few thousand shapes instead."""
from collections import namedtuple

Case = namedtuple("Case", "name form n cin h w cout ks stride nconvs plan")


def _p(F, chunks, ups, ragged, whole, grouped=None):
    return dict(F=F, chunks=chunks, ups=ups, ragged=ragged, whole=whole, grouped=grouped)


_SAME_F4 = {1: _p(4, False, False, True, True), 2: _p(4, False, False, True, True, "same"), 3: _p(4, False, False, True, True, "same"),
            16: _p(4, False, False, True, True, "same")}
_SAME_F8 = {1: _p(8, True, False, False, True), 2: _p(8, True, False, False, True, "same"), 3: _p(8, True, False, False, True, "same"),
            16: _p(8, True, False, False, True, "same")}

CASES = [
    # ---- strip walk 3x3 ---------------------------------------------------------------------------------------------------------------
    Case("rows3_f4_2x8x24", "rows3", 2, 20, 8, 24, 40, 3, 1, (1, 2, 3, 16), _SAME_F4),          # three strips, six walks: 4 + 2 waves
    Case("rows3_f4_1x8x8", "rows3", 1, 20, 8, 8, 40, 3, 1, (1,), {1: _p(4, False, False, True, False)}),      # ONE walk: three idle waves
    Case("rows3_f8_2x8x32", "rows3", 2, 20, 8, 32, 40, 3, 1, (1,), {1: _p(8, True, False, False, True)}),
    Case("rows3_f8_2x24x16", "rows3", 2, 20, 24, 16, 40, 3, 1, (1, 2, 3, 16), _SAME_F8),        # six row ranges a column
    Case("rows3_f8_cin3", "rows3", 2, 3, 8, 32, 40, 3, 1, (1,), {1: _p(8, True, False, False, True)}),
    # 42 tiles x 16 problems: the shared budget is 4 waves a tile (6 one by one) -> two walks per wave, 3 waves, one group instead of two
    Case("rows3_shared_1x8x48", "rows3", 1, 200, 8, 48, 192, 3, 1, (1, 16),
         {1: _p(8, True, False, True, False), 16: _p(8, True, True, True, False, "shared")}),
    # 9 walks: one by one 9 waves in three groups; three problems together 5 waves of two walks in two groups
    Case("rows3_whole_3x8x24", "rows3", 3, 200, 8, 24, 192, 3, 1, (1, 3),
         {1: _p(4, False, False, True, True), 3: _p(4, False, True, True, True, "whole")}),
    # ---- stride 2 (H, W: the input; the walk runs over the H/2 x W/2 map) ----------------------------------------------------------------
    Case("s2_2x8x16", "s2", 2, 20, 8, 16, 40, 3, 2, (1,), {1: _p(4, False, True, True, False)}),
    Case("s2_cin3_2x16x32", "s2", 2, 3, 16, 32, 40, 3, 2, (1,), {1: _p(4, False, False, False, False)}),
    # ---- 1x1 walk -----------------------------------------------------------------------------------------------------------------------
    Case("rows1_f4_2x2x8", "rows1", 2, 72, 2, 8, 40, 1, 1, (1,), {1: _p(4, False, True, True, False)}),
    Case("rows1_f8_2x4x16", "rows1", 2, 72, 4, 16, 40, 1, 1, (1,), {1: _p(8, False, True, True, False)}),
    Case("rows1_f4_3x6x24", "rows1", 3, 20, 6, 24, 136, 1, 1, (1,), {1: _p(4, False, True, True, False)}),
    # ---- small-map LDS kernel --------------------------------------------------------------------------------------------------------------
    Case("tiny_9x3x5", "tiny", 9, 20, 3, 5, 40, 3, 1, (1, 3), None),            # image groups 8 + 1
    Case("tiny_1x1x1", "tiny", 1, 20, 1, 1, 40, 3, 1, (1,), None),
    Case("tiny_2x6x7", "tiny", 2, 20, 6, 7, 40, 3, 1, (1,), None),              # (8 x 7 needs 73.5 KB of LDS: declined, see nhwc_3x3_8x7)
    # ---- 16 x 16-tile kernel --------------------------------------------------------------------------------------------------------------
    Case("t16_3x6x6", "t16_3", 3, 32, 6, 6, 48, 3, 1, (1, 3), None),
    Case("t16_9x6x6", "t16_3", 9, 32, 6, 6, 48, 3, 1, (1, 3), None),            # 7 images a stage: two stages
    Case("t16_2x16x16", "t16_3", 2, 16, 16, 16, 16, 3, 1, (1, 3), None),        # one image per stage, split by pixel quads
    Case("t16_1x2x2", "t16_3", 1, 48, 2, 2, 32, 3, 1, (1, 3), None),            # one quad: one wave works
    Case("t16k1_3x6x6", "t16_1", 3, 32, 6, 6, 48, 1, 1, (1,), None),
    Case("t16k1_9x6x6", "t16_1", 9, 32, 6, 6, 48, 1, 1, (1,), None),
    Case("t16k1_2x16x16", "t16_1", 2, 16, 16, 16, 16, 1, 1, (1,), None),
    Case("t16k1_1x2x2", "t16_1", 1, 48, 2, 2, 32, 1, 1, (1,), None),
    # ---- NHWC form ------------------------------------------------------------------------------------------------------------------------
    Case("nhwc_3x3_9x11", "nhwc", 2, 20, 9, 11, 40, 3, 1, (1,), None),          # odd Wo: the per-lane pixel walk
    Case("nhwc_3x3_9x10", "nhwc", 2, 20, 9, 10, 40, 3, 1, (1,), None),          # even Wo: the wave-uniform pair walk
    Case("nhwc_3x3_8x7", "nhwc", 2, 20, 8, 7, 40, 3, 1, (1,), None),            # 56 pixels, but more LDS than the small-map kernel has
    Case("nhwc_s2_7x10", "nhwc", 2, 20, 7, 10, 40, 3, 2, (1,), None),           # -> 4 x 5
    Case("nhwc_s2_6x12", "nhwc", 2, 20, 6, 12, 40, 3, 2, (1,), None),           # -> 3 x 6: even Wo
    Case("nhwc_1x1_5x9", "nhwc", 2, 20, 5, 9, 40, 1, 1, (1,), None),
]

BY_NAME = {c.name: c for c in CASES}
STRIP_FORMS = ("rows3", "s2", "rows1")


def squares(case):
    """The square_x variants a case runs."""
    return (False, True) if case.ks == 1 else (False,)


def seed(case):
    return 4000 + 17 * sum(ord(ch) for ch in case.name)
