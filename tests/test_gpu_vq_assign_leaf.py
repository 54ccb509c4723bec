"""vq_assign_kernel (csrc/vq.hip) on every template instance, slice split and codeword range, plain and under the per-vector rate term,
on the cases of tests/_vq_assign_cases.py -- whose plans tests/test_vq_assign_plan.py holds to literals through mcq_vq_assign_plan --
plus the operand stream of vq_pack_kernel and vq_gather_kernel.

Bars.  Integer inputs: NumPy's first-index argmin of the float64 costs at EVERY position, nothing excused (why the float32 kernel is
exact there: `test_exact_arithmetic`).  Gaussian inputs: the float64 argmin, a differing position excused only inside the project's
bound (d + 4) 2^-23 (|x|^2 + |c|^2 + 2 |x.c| + lambda_v bits) (`_rate_ref.audit`, `_rate_map_ref.audit`), at most 1 % of a case's
positions (`_rate_ref.EXCUSED_CAP`; the CPU emulation of tests/test_vq_assign_plan.py stays under it on the same inputs).  The three
entry forms agree bit for bit.  Every launch here writes its codes into the middle of a larger buffer and gets a workspace with a
tail behind mcq_vq_assign_workspace_bytes: both margins must come back untouched.  Pack and gather: bit for bit."""

import numpy as np
import pytest
import torch

import _rate_ref as RR
import _vq_assign_cases as K

pytestmark = pytest.mark.gpu

CODE_SENTINEL = -0x5A5A5A5A5A5A5A5B
CODE_MARGIN = 1024                    # int64 words in front of and behind the codes
WS_SENTINEL = 0xA5
WS_MARGIN = 4096                      # bytes behind the workspace
IDS = [c.name for c in K.CASES]


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


_STATE = {}


def _state(dev, case, kind):
    """One case's inputs, made once and left unchanged: NumPy and device copies, the plain pack, the bits section, a cache of references."""
    key = (str(dev), case.name, kind)
    if key not in _STATE:
        from mcquic_amd import ops
        x, cb, cdf, lam = K.integer_case(case) if kind == "integer" else K.gaussian_case(case)
        _STATE[key] = dict(x=x, cb=cb, cdf=cdf, lam=lam, bits=RR.penalty_table(cdf), xd=_t(x, dev), pack=ops.PackedCodebook(_t(cb, dev)),
                           bits_d=ops.pack_bits(_t(cdf, dev)), lam_d=_t(lam, dev), want={}, got={})
    return _STATE[key]


def _launch(case, st, form, lam_d=None):
    """One launch of `form` -- "ws" (mcq_vq_assign_ws_f32 with the workspace the size query asks for), "nows" (mcq_vq_assign_f32: one
    workgroup per vector tile) or "rate" (mcq_vq_assign_rate_map_f32 with `lam_d`: [n, h, w] or [n]) -- into guarded buffers.  Returns
    the codes int64 [n, m, h, w] (NumPy) after checking that every code was written, lies in [0, k) and that the margins are intact."""
    from mcquic_amd import _lib, ops
    lib = _lib.load()
    dev = st["xd"].device
    n, m, d, h, w, k = K.dims(case)
    nvec = n * m * h * w
    big = torch.full((nvec + 2 * CODE_MARGIN,), CODE_SENTINEL, dtype=torch.int64, device=dev)
    codes = big[CODE_MARGIN:CODE_MARGIN + nvec]
    nbytes = lib.mcq_vq_assign_workspace_bytes(n, m, d, h, w, k)
    assert nbytes == (case.plan[2] * nvec * 8 if case.plan[2] > 1 else 0)
    ws = torch.full((nbytes + WS_MARGIN,), WS_SENTINEL, dtype=torch.uint8, device=dev)     # (zs = 1: a workspace nobody may touch)
    with ops._guard(dev):
        if form == "ws":
            rc = lib.mcq_vq_assign_ws_f32(st["xd"].data_ptr(), st["pack"].packed.data_ptr(), codes.data_ptr(), n, m, d, h, w, k, ws.data_ptr(),
                                          ops._stream())
        elif form == "nows":
            rc = lib.mcq_vq_assign_f32(st["xd"].data_ptr(), st["pack"].packed.data_ptr(), codes.data_ptr(), n, m, d, h, w, k, ops._stream())
        else:
            assert form == "rate" and lam_d.is_contiguous() and tuple(lam_d.shape) in ((n,), (n, h, w))
            sn, sy, sx = (1, 0, 0) if lam_d.dim() == 1 else (h * w, w, 1)
            rc = lib.mcq_vq_assign_rate_map_f32(st["xd"].data_ptr(), st["pack"].packed.data_ptr(), st["bits_d"].data_ptr(), lam_d.data_ptr(),
                                                sn, sy, sx, codes.data_ptr(), n, m, d, h, w, k, ws.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    assert rc == 0, f"{case.name} {form}: status {rc}"
    assert bool((big[:CODE_MARGIN] == CODE_SENTINEL).all()) and bool((big[CODE_MARGIN + nvec:] == CODE_SENTINEL).all()), \
        f"{case.name} {form}: a code was written outside [n, m, h, w]"
    assert bool((ws[nbytes:] == WS_SENTINEL).all()), f"{case.name} {form}: the workspace was written past its {nbytes} bytes"
    if form == "nows":
        assert bool((ws == WS_SENTINEL).all())
    elif nbytes:
        # [zs][nvec] best distances, then [zs][nvec] codewords: the ranges that own a tile were launched and wrote every vector, the
        # ranges that own none (sp8_empty_range, sp32_7_empty_ranges) were not launched, and the fold read none of their words
        zs, launched = case.plan[2], K.geometry(case)["launched"]
        words = ws[:nbytes].view(torch.int32).reshape(2, zs, nvec)
        sentinel = int(np.array([WS_SENTINEL] * 4, dtype=np.uint8).view(np.int32)[0])
        idx = words[1].cpu().numpy()
        assert (idx[:launched] >= 0).all() and (idx[:launched] < k).all(), f"{case.name} {form}: a launched range left a vector unwritten"
        assert (idx[launched:] == sentinel).all() and bool((words[0, launched:] == sentinel).all()), \
            f"{case.name} {form}: a range past the {launched} that own a tile was launched"
    got = codes.cpu().numpy().reshape(n, m, h, w)
    assert (got != CODE_SENTINEL).all(), f"{case.name} {form}: {int((got == CODE_SENTINEL).sum())} codes were never written"
    assert got.min() >= 0 and got.max() < k, f"{case.name} {form}: codes outside [0, {k})"
    return got


def _want(st, form):
    """The float64 first-index argmin of a case's inputs, computed once."""
    if form not in st["want"]:
        st["want"][form] = K.argmin_rows(st["x"], st["cb"], None, None) if form == "plain" else K.argmin_rows(st["x"], st["cb"], st["bits"], st["lam"])
    return st["want"][form]


@pytest.mark.parametrize("case", K.CASES, ids=IDS)
def test_exact_arithmetic(dev, case):
    """Integer inputs in [-4, 4], widths that are powers of two, lambda in {0, 1/4, 3}.  Every number the kernel forms is then exact in
    float32: a product x c or x x is an integer of magnitude <= 16; |x|^2, |c|^2 and every partial sum of <x, c> -- in whatever order
    the MFMA adds a k-step's two products -- are integers of magnitude <= 16 d <= 4096; x2 + c2 <= 8192 and fma(-2, inter, x2 + c2) is
    the integer |x - c|^2 <= 64 d <= 16384; bits = 16 - log2(2^e) is an integer in 4 .. 16, so fma(lambda, bits, dist) is a multiple of
    1/4 below 16384 + 48 -- all far inside the 2^24 integers (2^22 quarters) float32 holds exactly.  The codes must therefore equal
    the float64 argmin, first index on ties, at every position, and `_vq_assign_cases.integer_case` plants ties across half-waves,
    32-row bands, tiles, slices and ranges, with and without the rate term."""
    st = _state(dev, case, "integer")
    for form in ("plain", "rate"):
        if not K.runs(case, form):
            continue
        got = _launch(case, st, "ws") if form == "plain" else _launch(case, st, "rate", st["lam_d"])
        want = _want(st, form)
        bad = got != want
        assert not bad.any(), (f"{case.name} {form}: {int(bad.sum())} of {got.size} codes differ from the exact argmin, first at "
                               f"{tuple(np.argwhere(bad)[0])}: got {got[bad][0]}, want {want[bad][0]}")
    if case.forms == "both" and case.k >= 128:
        assert not np.array_equal(_want(st, "plain"), _want(st, "rate")), "the rate term changes nothing: the case tests no rate path"


@pytest.mark.parametrize("case", K.CASES, ids=IDS)
def test_gaussian_inputs_against_float64(dev, case):
    st = _state(dev, case, "gaussian")
    for form in ("plain", "rate"):
        if not K.runs(case, form):
            continue
        got = _launch(case, st, "ws") if form == "plain" else _launch(case, st, "rate", st["lam_d"])
        differ, unexcused = K.audit_rows(st["x"], st["cb"], st["bits"], None if form == "plain" else st["lam"], got)
        print(f"{case.name} {form}: {differ} of {got.size} positions excused, {unexcused} unexcused")
        assert unexcused == 0, f"{case.name} {form}: {unexcused} codes differ from float64 beyond the rounding bound"
        assert differ <= RR.EXCUSED_CAP * got.size, f"{case.name} {form}: {differ} of {got.size} positions differ inside the bound"


def _plain_codes(case, st):
    """The codes of the workspace form on a case's inputs, launched once: what the form and gather tests start from."""
    if "ws" not in st["got"]:
        st["got"]["ws"] = _launch(case, st, "ws")
    return st["got"]["ws"]


@pytest.mark.parametrize("kind", ["gaussian", "integer"])
@pytest.mark.parametrize("case", K.CASES, ids=IDS)
def test_forms_agree(dev, case, kind):
    """With a workspace, without one (no ranges: one workgroup per vector tile) and under an all-zero lambda map (fma(0, bits, dist) =
    dist), per vector and per image: the same codes bit for bit -- on the Gaussian inputs and on the integer inputs, where ties are
    everywhere, so ranged and unranged launches must break them alike: every form there is the exact first-index argmin."""
    st = _state(dev, case, kind)
    dev_ = st["xd"].device
    ws = _plain_codes(case, st)
    if kind == "integer":
        assert np.array_equal(ws, _want(st, "plain"))
    assert np.array_equal(_launch(case, st, "nows"), ws), "ranged and one-workgroup forms disagree"
    assert np.array_equal(_launch(case, st, "rate", torch.zeros((case.n, case.h, case.w), device=dev_)), ws), "a zero map is not the plain code"
    assert np.array_equal(_launch(case, st, "rate", torch.zeros((case.n,), device=dev_)), ws), "a zero per-image lambda is not the plain code"


@pytest.mark.parametrize("case", K.CASES, ids=IDS)
def test_nothing_outside_the_output_is_written(dev, case):
    """Partial blocks (lanes without a pixel), waves without a vector tile, the clamped copy of an odd last block and the range
    workspace: every form with per-vector and per-image lambdas, on the integer inputs; `_launch` holds the margins around the codes
    and behind the workspace, and the workspace's own rows to the ranges that were launched."""
    st = _state(dev, case, "integer")
    for form, lam in (("ws", None), ("nows", None), ("rate", st["lam_d"]), ("rate", st["lam_d"][:, 0, 0].contiguous())):
        _launch(case, st, form, lam)


@pytest.mark.parametrize("m, k, d", K.PACK_CASES)
def test_operand_stream(dev, m, k, d):
    """vq_pack_kernel's section of the packed codebook, [m][ntile][Sp][64][4] and the zero tail of VQ_PF k-steps, bit for bit against
    the index rule restated in NumPy; padded codewords and channels past d are +0.  (The norm section behind it:
    tests/test_gpu_rate_encode.py::test_pack_sections.)"""
    from mcquic_amd import _lib, ops
    rng = np.random.default_rng([11, m, k, d])
    cb = rng.standard_normal((m, k, d)).astype(np.float32)
    cb[cb == 0] = 1.0                                                # a zero in the stream is padding, nothing else
    want = K.packed_stream(cb)
    ntile = (k + 127) // 128
    assert want.size == (m * ntile * K.sp(d) + K.RING) * 256
    packed = ops.PackedCodebook(_t(cb, dev)).packed.cpu().numpy()
    assert packed.size == _lib.load().mcq_packed_codebook_floats(m, k, d) == want.size + m * (ntile + 1) * 256
    got = packed[:want.size]
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), f"{int((got.view(np.int32) != want.view(np.int32)).sum())} words differ"
    assert int((got != 0).sum()) == m * k * d and (got[-K.RING * 256:].view(np.int32) == 0).all()


def _ulps(got, want64):
    want32 = want64.astype(np.float32)
    return np.abs(got.astype(np.float64) - want64) / np.maximum(np.spacing(np.abs(want32)).astype(np.float64), 2.0 ** -149)


@pytest.mark.parametrize("case", K.CASES, ids=IDS)
def test_gather(dev, case):
    """vq_gather_kernel on the case's own codes: the rows of the codebook bit for bit, with and without the SiLU twin; the twin inside
    the bar of tests/test_gpu_ops.py::test_silu_accuracy (3.5 ulp of the float64 value, 2.75 where |c| <= 10)."""
    from mcquic_amd import ops
    st = _state(dev, case, "gaussian")
    codes = _plain_codes(case, st)
    n, m, h, w = codes.shape
    rows = st["cb"][np.arange(m)[None, :, None, None], codes]                   # [n, m, h, w, d]
    want = np.ascontiguousarray(rows.transpose(0, 1, 4, 2, 3)).reshape(n, m * case.d, h, w)
    cd = _t(codes, dev)
    plain = ops.vq_gather(cd, st["pack"])
    assert ops.silu_twin(plain) is None and np.array_equal(plain.cpu().numpy().view(np.int32), want.view(np.int32))
    both = ops.vq_gather(cd, st["pack"], dual_silu=True)
    assert np.array_equal(both.cpu().numpy().view(np.int32), want.view(np.int32))
    w64 = want.astype(np.float64)
    err = _ulps(ops.silu_twin(both).cpu().numpy(), w64 / (1.0 + np.exp(-w64)))
    assert err.max() <= 3.5 and err[np.abs(want) <= 10.0].max() <= 2.75, (case.name, err.max())


def test_gather_clamps_codes_outside_the_codebook(dev):
    """Codes below 0 go to codeword 0, codes >= k to codeword k - 1 (the header's contract; the reference would raise)."""
    from mcquic_amd import ops
    case = K.BY_NAME["sp8_k129_two_slices"]
    st = _state(dev, case, "gaussian")
    n, m, h, w, k = case.n, case.m, case.h, case.w, case.k
    rng = np.random.default_rng(5)
    codes = rng.integers(0, k, size=(n, m, h, w))
    outside = np.asarray([-1, -2, -(1 << 40), -(1 << 63), k, k + 1, 1 << 31, 1 << 32, (1 << 63) - 1], dtype=np.int64)
    flat = codes.reshape(-1)
    where = rng.choice(flat.size, size=3 * outside.size, replace=False)
    flat[where] = np.tile(outside, 3)
    want_codes = np.clip(codes, 0, k - 1)
    assert (want_codes != codes).sum() == where.size and {0, k - 1} <= set(want_codes.reshape(-1)[where].tolist())
    rows = st["cb"][np.arange(m)[None, :, None, None], want_codes]
    want = np.ascontiguousarray(rows.transpose(0, 1, 4, 2, 3)).reshape(n, m * case.d, h, w)
    got = ops.vq_gather(_t(codes, dev), st["pack"], dual_silu=True)
    assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
    w64 = want.astype(np.float64)
    assert _ulps(ops.silu_twin(got).cpu().numpy(), w64 / (1.0 + np.exp(-w64))).max() <= 2.75
