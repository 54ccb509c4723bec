"""GPU: every kernel form behind mcq_vq_soft_bwd_f32 -- the two backward contractions of the soft assignment -- launched through the
C ABI (mcq_nchw_to_nhwc_pair_f32 for the channel-major copies, then the entry point) into buffers the test owns, against the exact
and float64 references of tests/_soft_bwd_refs.py (held to float64 autograd by tests/test_soft_bwd_refs.py).

The forms (tests/_soft_bwd_cases.py; tests/test_soft_bwd_plan.py holds each case's route as a literal): vq_dx_mfma_kernel with one and
with two workgroups per tile (the latter behind vq_zero_kernel, adding onto dx) at 1 .. 5 chunks per wave around its ring of 4 and on
both sides of the tile-count rule, vq_dc_mfma_kernel at 1, 3, 16, 17 ring steps and a second index-scan pass, d = 64, 33, 32, 31, 1
on both; the tiled forms with fewer vectors than waves and an empty last slice; the lane-per-channel forms with a second pass of the
channel loop and a partial run of 64.  The route is asserted from mcq_vq_soft_bwd_plan -- the decision the entry point itself
launches by -- before every launch.

Every launch: dx, dC and the two channel-major copies each sit in an allocation of their own between 4096 sentinel floats, filled
with NaN first -- an entry the launch skips, or one the two-workgroup form adds onto without the zeroing, arrives as NaN.  Afterwards:
sentinels unchanged bit for bit, no NaN in dx / dC, every input equal to its clone, and a second launch into fresh NaN-filled buffers
returns the same bits (every form claims determinism, the two-addend atomic form in so many words).  Every pointer is 16-byte aligned.

Two data sets per case, the sampled codewords built by _soft_bwd_cases.index_pattern (every place of a 32-codeword block's
accumulators hit, one codeword hit twice within a scan pass and again from another wave slice, a block's neighbours hit):
  (i)  integers of [-3, 3] as float32, rowsum their exact sum: every partial sum in any order is an integer far below 2^24, so dx and dC
       must EQUAL soft_bwd_int -- a dropped or doubled codeword or vector, another group's codebook, a scatter into the wrong
       register, a missing zeroing or an unmasked ring entry shows whatever its size;
  (ii) uniform floats of [-1, 1) (ddist too: no 1e-3 scale that would hide the contraction under the straight-through term), rowsum
       the float32 rounding of the float64 row sum: e = max |got - soft_bwd64| / soft_bwd_scale64 for the kernel and for
       soft_bwd_seq_f32 (ONE float32 chain over all codewords / all vectors), e_hip <= max(4 e_seq, 1.2e-7) for dx and for dC each,
       the bar and floor of tests/test_gpu_conv_epilogues.py and tests/test_gpu_wgrad_leaf.py.

test_ring_mask: one NaN in ddist, rowsum left finite, in the k = 640 case (vq_dx_mfma_kernel: five chunks behind a ring of four) and
the V = 272 case (vq_dc_mfma_kernel: 17 steps behind a ring of 16).  IEEE propagation puts NaN in that vector's dx (every channel of the
group) and in that codeword's dC row; every other entry must carry the clean launch's bits.
  next_wave  the NaN sits at the first codeword of wave 1's slice of the dx kernel and the first vector of wave 1's slice of the dC
             kernel: the entry wave 0's ring reads past its own slice.  What this holds is the containment of a NaN to its row of dx
             and its row of dC through the slices' folds -- an unmasked ring entry of a NEIGHBOURING WAVE carries the same vectors
             (dx) / the same codewords (dC) and so lands in entries that are NaN anyway: those masks are pinned by data set (i),
             which every slice of 1, 3, 5 chunks and of 1, 3, 17 steps fails when the mask is dropped (tried);
  next_row   the NaN sits at codeword 0 of a vector inside a tile: the LAST wave's ring of the dx kernel runs past the end of its row
             of ddist into the next vector's first codewords, so an unmasked entry puts the NaN into the vector before (tried: fails
             when the mask is dropped).  The dC kernel has no such entry: past its last wave's slice lies the end of ddist, which the
             buffer resource reads as 0.

Measured on an MI355X (profiles/r13_soft_bwd_leaf_errors.json, 30 entries soft_bwd_leaf[<case>] with e_hip / e_seq for dx and dC): the
one-chain sum is a yardstick for every form.  Worst e_hip / e_seq per form -- dx: MFMA one workgroup per tile 0.37 (mix_both_1x1,
5.07e-8 against 1.36e-7), MFMA two workgroups 0.30 (dxm2_tiles255, 4.87e-8 against 1.63e-7), tiled 0.66, lane-per-channel 1.00 (k <= 64:
its one run of 64 is the yardstick's own chain; 0.47 .. 0.82 above that); dC: MFMA 1.02 (dcm_v16_k32, 1.42e-7 against 1.38e-7: two
vectors per slice, 0.23 at V = 8192), tiled 1.16 (til_dc_v5, 8.32e-8 against 7.20e-8), lane-per-channel 1.00 in all four cases
(vq_dc_kernel is the yardstick's chain, bit for bit in these figures).  The integer data set is exact in every case and form; no
kernel changed with this test."""
import ctypes

import pytest
import torch

import _soft_bwd_cases as K
import _soft_bwd_refs as S
from _record import record

pytestmark = pytest.mark.gpu

GUARD = 4096
SENTINEL = -12345.678
FLOOR = 1.2e-7
NAN = float("nan")
FORM = {0: "lane", 1: "tiled", 2: "mfma"}


class _Guarded:
    """`numel` floats filled with NaN between GUARD sentinel floats on both sides, one allocation (the payload 16-byte aligned)."""

    def __init__(self, numel, dev):
        self.numel = int(numel)
        self.buf = torch.full((2 * GUARD + self.numel,), SENTINEL, dtype=torch.float32, device=dev)
        self.view = self.buf[GUARD:GUARD + self.numel]
        self.view.fill_(NAN)
        self.ptr = self.view.data_ptr()
        assert self.ptr % 16 == 0

    def intact(self):
        bits = self.buf.view(torch.int32)
        want = torch.tensor([SENTINEL], dtype=torch.float32).view(torch.int32).item()
        return bool((bits[:GUARD] == want).all() & (bits[GUARD + self.numel:] == want).all())


def _launch(lib, case, dev_inputs):
    """One launch with every check of a single launch; dev_inputs = (ddist, rowsum, x, cb, ddeq, index, hot) on the device.
    Returns (dx, dC) on the CPU, NaN and all."""
    n, m, d, h, w, k = K.dims(case)
    out = (ctypes.c_int32 * 3)()
    assert lib.mcq_vq_soft_bwd_plan(n, m, d, h, w, k, out) == 1 and tuple(out) == case.plan, f"{case.name}: routed {tuple(out)}, meant for {case.plan}"
    ddist, rowsum, x, cb, ddeq, index, hot = dev_inputs
    dev = x.device
    keep = [t.clone() for t in dev_inputs]
    c, hw = m * d, h * w
    xt, dqt = _Guarded(n * hw * c, dev), _Guarded(n * hw * c, dev)
    dx, dcb = _Guarded(n * c * hw, dev), _Guarded(m * k * d, dev)
    assert all(t.is_contiguous() and t.data_ptr() % 16 == 0 for t in dev_inputs)
    rc = lib.mcq_nchw_to_nhwc_pair_f32(x.data_ptr(), xt.ptr, c, hw, 0, ddeq.data_ptr(), dqt.ptr, c, hw, n, None)
    torch.cuda.synchronize()
    assert rc == 0, f"{case.name}: mcq_nchw_to_nhwc_pair_f32 returned {rc}"
    assert torch.equal(xt.view.reshape(n, hw, c), x.reshape(n, c, hw).permute(0, 2, 1)), f"{case.name}: the channel-major copy of x"
    assert torch.equal(dqt.view.reshape(n, hw, c), ddeq.reshape(n, c, hw).permute(0, 2, 1)), f"{case.name}: the channel-major copy of dDeq"
    keep_t = xt.view.clone(), dqt.view.clone()
    rc = lib.mcq_vq_soft_bwd_f32(ddist.data_ptr(), rowsum.data_ptr(), x.data_ptr(), xt.ptr, dqt.ptr, index.data_ptr(), hot.data_ptr(), cb.data_ptr(),
                                 dx.ptr, dcb.ptr, n, m, d, h, w, k, None)
    torch.cuda.synchronize()
    assert rc == 0, f"{case.name}: mcq_vq_soft_bwd_f32 returned {rc}"
    assert all(g.intact() for g in (xt, dqt, dx, dcb)), f"{case.name}: a sentinel was written"
    for a, b in zip(list(dev_inputs) + [xt.view, dqt.view], keep + list(keep_t)):
        same = torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)
        assert same, f"{case.name}: an input was written"
    return dx.view.cpu().reshape(n, c, h, w), dcb.view.cpu().reshape(m, k, d)


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _inputs(case, kind):
    n, m, d, h, w, k = K.dims(case)
    ddist, rowsum, x, cb, ddeq, hot = (S.int_inputs if kind == "int" else S.uniform_inputs)(n, m, d, h, w, k, K.seed(case) + (kind == "uniform"))
    return ddist, rowsum, x, cb, ddeq, K.index_pattern(n, m, h, w, k), hot


@pytest.mark.parametrize("case", K.CASES, ids=[c.name for c in K.CASES])
def test_soft_bwd_leaf(dev, case):
    from mcquic_amd import _lib
    lib = _lib.load()
    failures = []
    for kind in ("int", "uniform"):
        args = _inputs(case, kind)
        on_dev = tuple(t.to(dev) for t in args)
        dx, dc = _launch(lib, case, on_dev)
        for t, what in ((dx, "dx"), (dc, "dC")):
            assert not bool(torch.isnan(t).any()), f"{case.name} {kind}: NaN in {what} (an entry never written, or added onto an unzeroed one)"
        dx2, dc2 = _launch(lib, case, on_dev)
        assert _bits_equal(dx, dx2) and _bits_equal(dc, dc2), f"{case.name} {kind}: a second identical launch gives other bits"
        if kind == "int":
            ix, ic = S.soft_bwd_int(*args)
            for got, want, what in ((dx, ix.to(torch.float32), "dx"), (dc, ic.to(torch.float32), "dC")):
                bad = int((got != want).sum())
                if bad:
                    failures.append(f"{case.name} int: {bad} of {want.numel()} {what} entries differ from the integer sums "
                                    f"(max |diff| {float((got - want).abs().max())}, first at {tuple(int(i) for i in (got != want).nonzero()[0])})")
            int_exact = not failures
            continue
        x64, c64 = S.soft_bwd64(*args)
        sx, sc = S.soft_bwd_scale64(*args)
        qx, qc = S.soft_bwd_seq_f32(*args)
        figures = {}
        for what, got, seq, want, scale, form in (("dx", dx, qx, x64, sx, case.plan[0]), ("dc", dc, qc, c64, sc, case.plan[1])):
            e_hip, e_seq = S.rel_err(got, want, scale), S.rel_err(seq, want, scale)
            bar = max(4 * e_seq, FLOOR)
            figures.update({f"e_hip_{what}": e_hip, f"e_seq_{what}": e_seq, f"bar_{what}": bar})
            print(f"soft_bwd_leaf[{case.name}] {what} ({FORM[form]}) e_hip {e_hip:.3e} e_seq {e_seq:.3e} ratio {e_hip / e_seq if e_seq else 0.0:.2f} bar {bar:.3e}")
            if not e_hip <= bar:
                failures.append(f"{case.name} {what} ({FORM[form]}): e_hip {e_hip:.3e} > max(4 e_seq, floor) = {bar:.3e} (e_seq {e_seq:.3e})")
        record(f"soft_bwd_leaf[{case.name}]", dx_form=FORM[case.plan[0]], dc_form=FORM[case.plan[1]], dx_split=case.plan[2],
               e_hip=max(figures["e_hip_dx"], figures["e_hip_dc"]), e_seq=max(figures["e_seq_dx"], figures["e_seq_dc"]),
               int_exact=int_exact, **figures)
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("name,where", [(K.RING_DX, "next_wave"), (K.RING_DC, "next_wave"), (K.RING_DX, "next_row")],
                         ids=[f"{K.RING_DX}-next_wave", f"{K.RING_DC}-next_wave", f"{K.RING_DX}-next_row"])
def test_ring_mask(dev, name, where):
    from mcquic_amd import _lib
    lib = _lib.load()
    case = K.BY_NAME[name]
    n, m, d, h, w, k = K.dims(case)
    hw, v = h * w, n * h * w
    assert case.plan[1] == 2 and v % 16 == 0
    g = 1
    r = v // 8                                                       # the first vector of wave 1's slice of vq_dc_mfma_kernel
    if where == "next_row":
        # the LAST wave's ring of vq_dx_mfma_kernel runs past the end of its row of ddist: lane i holds codewords 0 .. 23 of row
        # row0 + i + 1 when the slice ends.  A NaN at codeword 0 of vector r belongs to dx of r alone; unmasked it reaches r - 1.
        assert case.plan[0] == 2 and r % 32 != 0
        c = 0
    else:
        c = k // (16 * case.plan[2]) if case.plan[0] == 2 else 33    # the first codeword of wave 1's slice of vq_dx_mfma_kernel
    if name == K.RING_DX:
        assert case.plan[0] == 2 and k // (16 * case.plan[2]) // 8 == 5      # five chunks: a wave's ring holds chunks 5 .. 7 when its slice ends
    else:
        assert r // 2 == 17                                          # 17 steps: wave 0's ring holds steps 17 .. 31 of wave 1 when it ends
    a, p = divmod(r, hw)
    args = _inputs(case, "uniform")
    clean = _launch(lib, case, tuple(t.to(dev) for t in args))
    assert all(bool(torch.isfinite(t).all()) for t in clean)
    ddist = args[0].clone()
    ddist.reshape(n, m, hw, k)[a, g, p, c] = NAN
    dx, dc = _launch(lib, case, tuple(t.to(dev) for t in (ddist,) + args[1:]))
    want_x = torch.zeros((n, m, d, hw), dtype=torch.bool)
    want_x[a, g, :, p] = True
    want_c = torch.zeros((m, k, d), dtype=torch.bool)
    want_c[g, c] = True
    for got, ref, want, what in ((dx, clean[0], want_x.reshape(n, m * d, h, w), "dx"), (dc, clean[1], want_c, "dC")):
        nan = torch.isnan(got)
        assert bool(nan[want].all()), f"{name}: the NaN did not reach its own {what} entries"
        stray = int((nan & ~want).sum())
        assert stray == 0, f"{name}: {stray} {what} entries outside vector {r} / codeword {c} of group {g} are NaN: a ring entry past the slice was used"
        assert torch.equal(got[~want].view(torch.int32), ref[~want].view(torch.int32)), f"{name}: {what} entries beside the NaN's changed bits"
