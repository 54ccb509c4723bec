"""CPU: the launch plan of the weight-gradient strip walks (rows_plan of csrc/wgrad_rows.hip: pure host code), through
mcq_conv2d_wgrad_nchw_plan -- the planner the launchers call, the gmax fall-back of a grouped launch included.

(a) the invariants every launch relies on, over a few thousand shapes: the kernels read them without a check (a wave whose walk index
    is past `units` leaves; the reduce pass reads `groups` partial tiles and 4 `groups` bias partials a convolution; the workspace
    holds nconv x the one-problem query).  The last assertion is the overrun condition itself.
(b) the branch table: which plan features each strip-walk case of tests/_wgrad_cases.py exercises, as literals, so that an edit of
    the planner's routing cannot shrink what tests/test_gpu_wgrad_leaf.py covers unnoticed."""
import ctypes
import itertools
import random

import pytest

import _wgrad_cases as K

NAMES = ("F", "strips", "row_chunks", "rpc", "units", "splits", "ups", "groups", "gmax")
CHANNELS = (3, 8, 20, 32, 40, 72, 128, 192)
NCONVS = (1, 2, 3, 7, 16)


@pytest.fixture(scope="module")
def lib():
    from mcquic_amd import _lib
    return _lib.load()


def plan(lib, n, cin, h, w, cout, taps, stride2, nconv=1):
    """The plan as a dict, or None where the strip walk does not take the shape (h, w: the input map)."""
    out = (ctypes.c_int32 * 9)(*([-1] * 9))
    ok = lib.mcq_conv2d_wgrad_nchw_plan(n, cin, h, w, cout, taps, int(stride2), nconv, out)
    assert ok in (0, 1)
    if not ok:
        assert list(out) == [-1] * 9, "a refused query wrote its output"
        return None
    return dict(zip(NAMES, out))


def one_problem_floats(lib, n, cin, h, w, cout, taps, stride2):
    q = lib.mcq_conv2d_wgrad_s2_nchw_workspace_floats if stride2 else (lib.mcq_conv2d_wgrad_nchw_workspace_floats if taps == 9 else lib.mcq_conv2d_wgrad1x1_nchw_workspace_floats)
    return q(n, cin, h, w, cout)


def _sweep_shapes(taps, stride2, count):
    """Seeded sample of N 1..8, walk maps with H, W multiples of 8 up to 256 (even H for 1x1 and stride 2), channels of CHANNELS."""
    rng = random.Random(100 * taps + stride2)
    hs = range(2, 257, 2) if (taps == 1 or stride2) else range(8, 257, 8)
    shapes = set()
    # the small end in full (where the budgets and the rounding bite), the rest sampled
    for n, h, w in itertools.product((1, 2, 3), [v for v in hs if v <= 24], (8, 16, 24, 32)):
        shapes.add((n, rng.choice(CHANNELS), h, w, rng.choice(CHANNELS)))
    while len(shapes) < count:
        shapes.add((rng.randint(1, 8), rng.choice(CHANNELS), rng.choice(hs), 8 * rng.randint(1, 32), rng.choice(CHANNELS)))
    return sorted(shapes)


@pytest.mark.parametrize("taps,stride2", [(9, False), (1, False), (9, True)], ids=["3x3", "1x1", "stride2"])
def test_plan_invariants_sweep(lib, taps, stride2):
    body_rows = {4: 8, 8: 4}
    planned = declined = 0
    for n, cin, mh, mw, cout in _sweep_shapes(taps, stride2, 1200):
        h, w = (2 * mh, 2 * mw) if stride2 else (mh, mw)             # the entry points take the input map
        one = one_problem_floats(lib, n, cin, h, w, cout, taps, stride2)
        for nconv in NCONVS:
            p = plan(lib, n, cin, h, w, cout, taps, stride2, nconv)
            what = f"{n}x{cin}->{cout} {h}x{w} taps {taps} stride2 {stride2} nconv {nconv}: {p}"
            if p is None:                                          # the one-pass kernel's shapes (query 1), or a tensor of 1 GiB (query 0)
                assert one in (0, 1), what
                declined += 1
                continue
            planned += 1
            assert one > 1, what
            rb = 2 if (taps == 1 or stride2) else body_rows[p["F"]]
            assert p["F"] in (4, 8) and p["strips"] * 2 * p["F"] == mw, what
            assert 1 <= p["splits"] <= p["units"], what
            assert p["ups"] >= 1 and (p["units"] + p["ups"] - 1) // p["ups"] == p["splits"], what
            assert p["groups"] == (p["splits"] + 3) // 4, what
            assert p["rpc"] > 0 and p["rpc"] % rb == 0, what
            assert p["row_chunks"] * p["rpc"] >= mh and (p["row_chunks"] - 1) * p["rpc"] < mh, what
            assert p["units"] == n * p["strips"] * p["row_chunks"], what
            assert p["groups"] <= p["gmax"], what
            # what the launch writes (part[conv][group][tap][co][ci] + bias_part[conv][4 group][co]) against what the caller was told to bring
            assert nconv * p["groups"] * (taps * cout * cin + 4 * cout) <= nconv * one, what
            if nconv == 1:
                assert p["gmax"] * (taps * cout * cin + 4 * cout) == one, what
    assert planned >= 3000 and declined < planned, (planned, declined)


def test_plan_query_refusals(lib):
    out = (ctypes.c_int32 * 9)()
    q = lib.mcq_conv2d_wgrad_nchw_plan
    assert q(2, 20, 8, 24, 40, 9, 0, 1, None) == 0                     # no output
    assert q(2, 20, 8, 24, 40, 5, 0, 1, out) == 0                      # taps
    assert q(2, 20, 8, 24, 40, 1, 1, 1, out) == 0                      # no 1x1 stride-2 walk
    assert q(2, 20, 8, 24, 40, 9, 0, 0, out) == 0 and q(2, 20, 8, 24, 40, 9, 0, lib.mcq_conv2d_wgrad_nchw_max_group() + 1, out) == 0
    assert q(2, 20, 8, 12, 40, 9, 0, 1, out) == 0                      # W no multiple of 8
    assert q(2, 20, 12, 16, 40, 9, 0, 1, out) == 0                     # 3x3: H no multiple of 8
    assert q(2, 20, 6, 16, 40, 1, 0, 1, out) == 1 and q(2, 20, 5, 16, 40, 1, 0, 1, out) == 0      # 1x1: even H
    assert q(2, 20, 6, 16, 40, 9, 1, 1, out) == 0 and q(2, 20, 12, 16, 40, 9, 1, 1, out) == 1     # stride 2: W / 2 a multiple of 8
    assert q(2, 32, 8, 16, 48, 9, 0, 1, out) == 0 and q(2, 32, 8, 16, 48, 1, 0, 1, out) == 0      # <= 512 pixels, channels in sixteens: 16 x 16 tiles


# ---- (b) the branch table ------------------------------------------------------------------------------------------------------------------
STRIP = [(c, nconv) for c in K.CASES if c.form in K.STRIP_FORMS for nconv in c.nconvs]


def features(lib, case, nconv):
    """What the query says about a case, in the terms of _wgrad_cases.py's literals."""
    taps, s2 = case.ks * case.ks, case.stride == 2
    p = plan(lib, case.n, case.cin, case.h, case.w, case.cout, taps, s2, nconv)
    assert p is not None, f"{case.name}: not a strip-walk shape"
    mh = case.h // 2 if s2 else case.h
    whole = taps == 9 and not s2 and case.n * mh * p["strips"] // 8 >= 4       # (the condition of rows_plan_search's second search)
    grouped = None
    if nconv > 1:
        one = plan(lib, case.n, case.cin, case.h, case.w, case.cout, taps, s2, 1)
        grouped = "same" if p == one else ("whole" if whole else "shared")
    return dict(F=p["F"], chunks=p["row_chunks"] > 1, ups=p["ups"] > 1, ragged=p["splits"] % 4 != 0, whole=whole, grouped=grouped), p


@pytest.mark.parametrize("case,nconv", STRIP, ids=[f"{c.name}-n{k}" for c, k in STRIP])
def test_branch_table(lib, case, nconv):
    got, p = features(lib, case, nconv)
    assert got == case.plan[nconv], f"{case.name} nconv {nconv}: plan {p}"


def test_branch_table_covers_every_feature():
    rows = [c.plan[k] for c, k in STRIP]
    for key, values in (("F", (4, 8)), ("chunks", (False, True)), ("ups", (False, True)), ("ragged", (False, True)),
                        ("whole", (False, True)), ("grouped", (None, "same", "shared", "whole"))):
        for v in values:
            assert any(r[key] == v for r in rows), f"no strip-walk case with {key} = {v}"
    for form in K.STRIP_FORMS:                                       # each walk kernel at both values of what it can vary
        mine = [c.plan[k] for c, k in STRIP if c.form == form]
        assert {r["ragged"] for r in mine} >= ({True, False} if form != "rows1" else {True}), form
        assert {r["F"] for r in mine} == ({4} if form == "s2" else {4, 8}), form
    forms = {c.form for c in K.CASES}
    assert forms == {"rows3", "s2", "rows1", "tiny", "t16_3", "t16_1", "nhwc"}
    assert {k for c in K.CASES if c.form == "rows3" for k in c.nconvs} >= {1, 2, 3, 16}
    assert all(3 in c.nconvs for c in K.CASES if c.form == "t16_3") and any(3 in c.nconvs for c in K.CASES if c.form == "tiny")


def test_routes_of_the_other_forms(lib):
    """The forms without a plan: what the workspace queries say (1 = a one-pass kernel without workspace, 0 = not this entry point's)."""
    from mcquic_amd import _lib  # noqa: F401  (the library is loaded by the fixture)
    for c in K.CASES:
        dims = (c.n, c.cin, c.h, c.w, c.cout)
        q3, q1, q2 = lib.mcq_conv2d_wgrad_nchw_workspace_floats(*dims), lib.mcq_conv2d_wgrad1x1_nchw_workspace_floats(*dims), lib.mcq_conv2d_wgrad_s2_nchw_workspace_floats(*dims)
        sixteens = c.cin % 16 == 0 and c.cout % 16 == 0
        if c.form == "rows3":
            assert q3 > 1, c.name
        elif c.form == "s2":
            assert q2 > 1, c.name
        elif c.form == "rows1":
            assert q1 > 1, c.name
        elif c.form == "tiny":
            assert q3 == 1 and not sixteens and plan(lib, *dims, 9, False) is None, c.name
        elif c.form == "t16_3":
            assert q3 == 1 and sixteens and plan(lib, *dims, 9, False) is None, c.name
        elif c.form == "t16_1":
            assert q1 == 1 and sixteens and plan(lib, *dims, 1, False) is None, c.name
        else:
            assert (q3 if (c.ks, c.stride) == (3, 1) else q2 if c.stride == 2 else q1) == 0, c.name
            assert lib.mcq_conv2d_wgrad_workspace_floats(*dims, c.ks, c.stride) > 0, c.name
