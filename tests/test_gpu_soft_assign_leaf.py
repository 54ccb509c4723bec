"""GPU: the soft assignment of the training quantizer (csrc/vq_train.hip), kernel by kernel, against float64 references written
from the mathematics (tests/_leaf_refs.py: soft_bwd64, inner64; tests/test_leaf_ops_reference.py ties soft_bwd64 to the oracle's
own autograd) and against the oracle itself for the discrete results.

`mcq_vq_softmax_bwd_f32` and `mcq_vq_gumbel_sample_f32` choose one of four kernels by the row length k -- 64, 256 or 1024 threads
holding the row in registers for k <= 512 / 2048 / 8192, a wave walking the row beyond -- and the whole-model gradient tests reach
the first form with a float64 reference only.  Here every form runs on both sides of its boundary, on rows that do not fill the
last workgroup, with three groups of which one has its temperature below the bound.

Bars: for every asserted quantity, e_hip = the kernel against float64 and e_f32 = the same formulas in float32 on the CPU against
float64, both in the scales of R.soft_bwd_scales64 / R.inner_scale64 (a sum that cancels is measured against the sum of its terms'
magnitudes, never against itself); e_hip <= max(4 e_f32, 1.2e-7) -- the factor of _leaf_refs.py for kernels with a transcendental,
the floor one float32 spacing at the scale.  Both figures of every case go to the run's record (tests/_record.py)."""
import math

import pytest
import torch

import _leaf_refs as R
from _record import record
from oracle import mcquic_ref as O

pytestmark = pytest.mark.gpu

FLOOR = 1.2e-7                                   # one float32 spacing relative to the scale
BOUND = 0.5
TEMPERATURE = (1.3, 0.2, 0.8)                    # group 1 below the bound
ROWS_SHAPE = (2, 3, 1, 5)                        # n, m, h, w: 30 rows = 7 workgroups of four and one of two; hw = 5, so g = (row / 5) % 3
BWD_K = (8, 63, 64, 65, 512, 513, 2048, 2049, 8192, 8193, 20000)


def _bar(key, e_hip, e_f32):
    bar = max(4.0 * e_f32, FLOOR)
    record(key, e_hip=e_hip, e_f32=e_f32, bar=bar)
    print(f"{key}: e_hip {e_hip:.3e}  e_f32 {e_f32:.3e}  bar {bar:.3e}")
    assert e_hip <= bar, f"{key}: kernel {e_hip:.3e} > max(4 x {e_f32:.3e}, {FLOOR:.1e})"


# ---- soft-max backward ------------------------------------------------------------------------------------------------------------------
def _bwd_case(k, seed, all_dropped_row=None, upper_clamp=False):
    """(post, raw, u, dS, dlogits, temperature) on ROWS_SHAPE + (k,): raw in [-4, 0] tb; a 20 % drop applied as fl32(raw + -1e9), in
    rows 0, 7, 13 and 29 on the largest entry too; the Gumbel draw on float32's grid with the clamped end 0 present; dS ~ 0.1 N(0, 1),
    dlogits ~ 0.05 U(-.5, .5).  `upper_clamp`: the draw holds 1 - 2^-24 too, which the clamp turns into Gumbel noise of 15.9: that
    entry then has y = 1 - O(k e^-13) and holds its row.  The cases with `dlogits` carry it, and without `dlogits`
    test_softmax_bwd_row_held_by_one_entry does."""
    n, m, h, w = ROWS_SHAPE
    rows = n * m * h * w
    g = torch.Generator().manual_seed(seed)
    temp = torch.tensor(TEMPERATURE, dtype=R.F32).reshape(m, 1, 1, 1)
    tb = R.row_tb(temp, BOUND, m, h * w, rows, R.F32)
    raw = (torch.rand((rows, k), generator=g) * -4.0) * tb[:, None]
    mask = torch.rand((rows, k), generator=g) < 0.2
    for r in (0, 7, 13, 29):
        mask[r, raw[r].argmax()] = True
    if all_dropped_row is not None:
        mask[all_dropped_row] = True
    post = torch.where(mask, raw + -1e9, raw)
    u = torch.rand((rows, k), generator=g)
    u[2, 0] = 0.0
    if upper_clamp:
        u[3, k - 1] = 1.0 - 2.0 ** -24
    ds = torch.randn((rows, k), generator=g) * 0.1
    dl = (torch.rand((rows, k), generator=g) - 0.5) * 0.05
    shape = ROWS_SHAPE + (k,)
    return tuple(t.reshape(shape).contiguous() for t in (post, raw, u, ds, dl)) + (temp,)


def _run_bwd(dev, post, raw, u, ds, dl, temp, rng=None, dtrow_rows=None):
    """One launch against soft_bwd64; `rng`: the kernel remakes the draw `u` itself.  Returns the (e_hip, e_f32) pairs."""
    from mcquic_amd import ops
    n, m, h, w, k = post.shape
    args = (post, raw, u, ds, dl, temp, BOUND, m, h * w)
    want = R.soft_bwd64(*args)
    scales = R.soft_bwd_scales64(want[0], raw, temp, BOUND, m, h * w)
    e_f32 = R.soft_bwd_errs(R.soft_bwd_f32(*args), want, scales, dtrow_rows)
    post_d, ds_d = post.to(dev), ds.to(dev)
    rowsum, dtrow = ops.vq_softmax_bwd(post_d, None if rng is not None else u.to(dev), ds_d, temp.to(dev), BOUND,
                                       None if dl is None else dl.to(dev), None if dl is None else raw.to(dev), rng)
    assert torch.equal(post_d.cpu(), post), "the saved logits were written to"
    assert rowsum.shape == post.shape[:-1] and dtrow.shape == post.shape[:-1]
    got = (ds_d.cpu(), rowsum.cpu(), dtrow.cpu())                     # d dist is written over dS
    e_hip = R.soft_bwd_errs(got, want, scales, dtrow_rows)
    return list(zip(("ddist", "rowsum", "dtrow"), e_hip, e_f32))


@pytest.mark.parametrize("with_dlogits", [False, True])
@pytest.mark.parametrize("k", BWD_K)
def test_softmax_bwd(dev, k, with_dlogits):
    """d dist (in place over dS), rowsum and dtrow of ops.vq_softmax_bwd against R.soft_bwd64 at both sides of every dispatch
    boundary (512 | 513, 2048 | 2049, 8192 | 8193), every k % 64 around a wave (63, 64, 65), the smallest row and k = 20000, with
    and without a gradient on the logits themselves.  No discrete decision is involved: every row of every case is asserted.

    Measured on an MI355X (profiles/r08_soft_assign_leaf_errors.json), all 66 figures inside their bars: d dist e_hip 2.1e-7 .. 9.1e-7
    at e_f32 1.9e-7 .. 1.5e-5, the ratio e_hip / e_f32 at most 2.2; rowsum and dtrow 3.6e-9 .. 5.5e-7, ratio at most 3.8.

    This test found a defect.  The kernels computed dz = y (dS - <y, dS>) as written, and in a row that one entry holds (y = 0.90
    in a row of the k = 2049 case) that entry's dS - <y, dS> is a difference of nearly equal numbers: d dist came out at 1.810e-6
    against e_f32 4.111e-7 there (bar 1.645e-6), and at 3.6e-6 / 7.5e-6 for k = 63 / 64.  A more accurate Gumbel logarithm left that
    figure unchanged to the last digit; taking dS of the arg-max entry out of every term first (the same number, since sum y = 1)
    brought it to 8.892e-7, and k = 63 / 64 to 8.0e-7 / 3.7e-7."""
    post, raw, u, ds, dl, temp = _bwd_case(k, 1000 + k, upper_clamp=with_dlogits)
    assert 0.1 < float((post < -1e8).float().mean()) < 0.4 or k == 8
    for name, e_hip, e_f32 in _run_bwd(dev, post, raw, u, ds, dl if with_dlogits else None, temp):
        _bar(f"soft_assign_bwd[k={k},dlogits={with_dlogits}].{name}", e_hip, e_f32)


@pytest.mark.parametrize("with_dlogits", [False, True])
@pytest.mark.parametrize("k", [513, 8193])
def test_softmax_bwd_remakes_the_draw(dev, k, with_dlogits):
    """The same with the Gumbel draw made inside the kernel from a generator snapshot (a row kernel and the wave-per-row one); the
    float64 reference is given ops.hash_uniform's materialisation of stream 1 as its draw."""
    from mcquic_amd import ops
    post, raw, _, ds, dl, temp = _bwd_case(k, 2000 + k)
    rng = torch.tensor([0x5EED0000 + k, 3], dtype=torch.int64, device=dev)
    u = ops.hash_uniform(rng, 1, post.shape).cpu()
    assert float(u.min()) >= 0.0 and float(u.max()) < 1.0 and 0.45 < float(u.mean()) < 0.55
    for name, e_hip, e_f32 in _run_bwd(dev, post, raw, u, ds, dl if with_dlogits else None, temp, rng=rng):
        _bar(f"soft_assign_bwd_rng[k={k},dlogits={with_dlogits}].{name}", e_hip, e_f32)


@pytest.mark.parametrize("k", [513, 8193])
def test_softmax_bwd_row_held_by_one_entry(dev, k):
    """No gradient on the logits, and row 3 holds a draw of 1 - 2^-24: Gumbel noise 15.9 on one entry, which then has y = 1 - O(k e^-13).
    That entry's dS - <y, dS> is a difference of nearly equal numbers, and it is the row's largest d dist -- the case the kernels
    meet by taking dS of the arg-max entry out of every term first (see vq_softmax_bwd_kernel); a row kernel and the wave-per-row
    one.  Same references, scales and bar as test_softmax_bwd: the float32 yardstick keeps the plain formula, and its own error on
    this row (2.8e-5 of the row's largest d dist at k = 513) is what the bar is made of."""
    post, raw, u, ds, _, temp = _bwd_case(k, 5000 + k, upper_clamp=True)
    assert float(post.reshape(-1, k)[3, k - 1]) > -1e8                    # the entry is not dropped: it does hold the row
    for name, e_hip, e_f32 in _run_bwd(dev, post, raw, u, ds, None, temp):
        _bar(f"soft_assign_bwd_one_entry[k={k}].{name}", e_hip, e_f32)


def test_softmax_bwd_with_a_row_dropped_whole(dev):
    """k = 513, no gradient on the logits, and row 11 with EVERY entry dropped: its logits are all fl32(raw - 1e9) = -1e9 exactly.
    Float32's spacing there is 64 and the Gumbel noise lies in [-2.8, 15.9], so logit + noise IS -1e9 again for every entry -- in
    the reference implementation's float32 tensors as in the kernel -- and the row's soft-max is the uniform one.  The float64
    reference, which would keep the noise, is therefore given a constant draw (0.5) for that row and the true draw for all others;
    the kernel gets the true draw everywhere.  d dist and rowsum of that row are asserted like every other row's.  Its dtrow is
    only required to be finite: without `dlogits` the kernel takes raw / tb from the post-drop value, which has lost `raw` to that
    rounding, so what it sums is dz (-1e9 / tb) -- a rounding residue of sum dz = 0 scaled by 1e9 -- where the mathematics has
    sum dz raw / tb.  Such a row has probability prod_c f_c (every codeword's frequency at once), which vanishes for any real
    frequency table; all other rows' dtrow are asserted."""
    from mcquic_amd import ops
    k, row = 513, 11
    post, raw, u, ds, _, temp = _bwd_case(k, 3000 + k, all_dropped_row=row)
    n, m, h, w = ROWS_SHAPE
    assert bool((post.reshape(-1, k)[row] == -1e9).all())
    noise = -torch.log(-torch.log(u.double().clamp(R.EPS_F32, 1.0 - R.EPS_F32)))
    assert float(noise.abs().max()) < 32.0 and bool(((post.reshape(-1, k)[row] + noise.reshape(-1, k)[row].float()) == -1e9).all())
    u_ref = u.clone()
    u_ref.view(-1, k)[row] = 0.5
    args = (post, raw, u_ref, ds, None, temp, BOUND, m, h * w)
    want = R.soft_bwd64(*args)
    scales = R.soft_bwd_scales64(want[0], raw, temp, BOUND, m, h * w)
    others = torch.ones(post.shape[:-1], dtype=torch.bool)
    others.view(-1)[row] = False
    e_f32 = R.soft_bwd_errs(R.soft_bwd_f32(post, raw, u, ds, None, temp, BOUND, m, h * w), want, scales, others)
    ds_d = ds.to(dev)
    rowsum, dtrow = ops.vq_softmax_bwd(post.to(dev), u.to(dev), ds_d, temp.to(dev), BOUND)
    assert bool(torch.isfinite(dtrow).all())
    e_hip = R.soft_bwd_errs((ds_d.cpu(), rowsum.cpu(), dtrow.cpu()), want, scales, others)
    for name, a, b in zip(("ddist", "rowsum", "dtrow"), e_hip, e_f32):
        _bar(f"soft_assign_bwd_all_dropped[k={k}].{name}", a, b)


# ---- <dDeq, c_k> ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 8192, 64, 1, 2, 3), (3, 513, 10, 2, 3, 5), (2, 31, 1, 1, 1, 1), (12, 200, 16, 1, 4, 4), (1, 8193, 4, 1, 1, 2)])
def test_vq_inner(dev, shape):
    """ops.vq_inner against the float64 einsum, relative to sum_j |x_j c_kj|; the yardstick is the float32 chain in channel order.
    The shapes split the codeword tiles over grid.z with a last partial split (k = 8193: 65 tiles), leave a partial tile
    (513, 31, 200), a vector length of one and twelve groups."""
    from mcquic_amd import ops
    m, k, d, n, h, w = shape
    x, cb = R.randn((n, m * d, h, w), 4000 + k), R.randn((m, k, d), 4001 + k, 0.3)
    want, scale = R.inner64(x, cb), R.inner_scale64(x, cb)
    got = ops.vq_inner(x.to(dev), ops.PackedCodebook(cb.to(dev))).cpu()
    assert got.shape == want.shape
    _bar(f"soft_assign_inner[m{m}-k{k}-d{d}-{n}x{h}x{w}]", R.scaled_err(got, want, scale), R.scaled_err(R.inner_f32(x, cb), want, scale))


# ---- forward sample at the dispatch boundaries ------------------------------------------------------------------------------------------
SAMPLE_SEEDS = {513: 0, 2049: 0, 8193: 1, 20000: 0}          # 8193: seed 0 is clean too, but drops no row's largest logit


def _level_case(m, k, d, n, h, w, seed):
    """(x, codebook, temperature > BOUND, freq with half the codes unused, drop exponent, u_drop, u_gumbel in [eps32, 1 - eps32]).
    With half the codes unused the drop's exponent is ~3/4 log2 k and a fifth of all logits is dropped, the largest often among them."""
    g = torch.Generator().manual_seed(seed)
    cb = torch.randn((m, k, d), generator=g) * math.sqrt(2 / (5 * d))
    x = torch.randn((n, m * d, h, w), generator=g) * 0.1
    temp = torch.rand((m, 1, 1, 1), generator=g) + 0.6
    freq = (torch.rand((m, k), generator=g) ** 3 + 1e-3) * (torch.rand((m, k), generator=g) < 0.5)
    freq = freq / freq.sum(-1, keepdim=True)
    shape = (n, m, h, w, k)
    u1 = torch.rand(shape, generator=g)
    u2 = torch.rand(shape, generator=g).clamp(R.EPS_F32, 1.0 - R.EPS_F32)
    usage = (freq > O.EPS).float().mean().clamp(0., 1.)
    expo = -(math.log2(k) - 1) * (usage ** 2) + math.log2(k)
    return x, cb, temp, freq, expo, u1, u2


def _oracle_sample(logit0, freq, u1, u2, dtype):
    post = O.random_drop(logit0.to(dtype), freq.to(dtype), u1.to(dtype))
    sample, _, index = O.gumbel_softmax_hard(post, u2.to(dtype))
    return post, sample, index[..., 0], post.argmax(-1)


def sample_case(k, seed):
    """The forward case of one k and what the oracle makes of it in float32 and float64; `clean`: the two agree on every drop
    decision, code and sample index -- no decision of the case sits on a threshold that float32 rounding could move."""
    m, d, n, h, w = 3, 4, 1, 2, 2
    x, cb, temp, freq, expo, u1, u2 = _level_case(m, k, d, n, h, w, seed)
    logit0 = O.vq_logit(x, cb, temp, torch.tensor([BOUND]))
    p32, s32, i32, c32 = _oracle_sample(logit0, freq, u1, u2, torch.float32)
    p64, _, i64, c64 = _oracle_sample(logit0, freq, u1, u2, torch.float64)
    clean = torch.equal(p32 < -1e8, p64 < -1e8) and torch.equal(i32, i64) and torch.equal(c32, c64)
    near = int((((u1 ** expo) - freq[:, None, None, :]).abs() < 1e-6).sum())
    return dict(logit0=logit0, freq=freq, expo=expo, u1=u1, u2=u2, post=p32, sample=s32, index=i32, code=c32, clean=clean, near=near, cb=cb)


@pytest.mark.parametrize("k", sorted(SAMPLE_SEEDS))
def test_gumbel_sample_beyond_each_boundary(dev, k):
    """The comparison of test_gpu_train_forward.py::test_logits_and_sample_random_shapes at the first k of each row form and of
    the wave-per-row kernel (513, 2049, 8193) and at k = 20000, on twelve rows: dropped logits, codes, sample index, straight-through
    value and soft dequantisation against the oracle's random_drop / gumbel_softmax_hard / dequant_soft.

    The seed of every k is fixed (SAMPLE_SEEDS) such that the oracle run in float32 and in float64 agree on every drop decision,
    every code and every sample index -- checked again here, on the CPU -- so no decision sits on its threshold and every k is
    asserted in full; a differing drop mask fails with the threshold audit's figures instead of ending the case.  The stricter
    "no entry with |u^e - f| < 1e-6" cannot be had from ANY seed at these k: f ~ 2 / k <= 4e-3 and u^e has density ~1 / (e f^(1 - 1/e))
    there, so of the 12 k entries of a case some hundreds lie that close in absolute terms (counted below, `near`) while their
    relative distance from the threshold is still thousands of float32 spacings; agreement of the two precisions is the condition
    that says what the absolute figure was meant to."""
    from mcquic_amd import ops
    c = sample_case(k, SAMPLE_SEEDS[k])
    assert c["clean"], f"k={k} seed {SAMPLE_SEEDS[k]}: the float32 and float64 oracle runs differ in a decision"
    dropped = c["post"] < -1e8
    assert 0.1 < float(dropped.float().mean()) < 0.5
    assert int((dropped.gather(-1, c["logit0"].argmax(-1, keepdim=True))).sum()) >= 1          # a row's largest logit is dropped
    lg = c["logit0"].clone().to(dev)
    code, index, hot = ops.vq_gumbel_sample(lg, c["u1"].to(dev), c["u2"].to(dev), c["freq"].to(dev), c["expo"].to(dev))
    diff = (lg.cpu() - c["post"]).abs() > 1e-3
    if diff.any():
        margin = ((c["u1"] ** c["expo"]) - c["freq"][:, None, None, :]).abs()[diff]
        assert False, f"k={k}: {int(diff.sum())} drop decisions differ from the oracle's, the farthest {float(margin.max()):.3e} from its threshold"
    assert torch.equal(lg.cpu(), c["post"])                               # fl32(logit + -1e9), or the logit itself
    assert torch.equal(code.cpu(), c["code"])
    assert torch.equal(index.cpu(), c["index"])
    want_hot = torch.gather(c["sample"], -1, c["index"][..., None])[..., 0]
    assert (hot.cpu() - want_hot).abs().max().item() < 1e-6
    deq = ops.vq_dequant_soft(index, hot, ops.PackedCodebook(c["cb"].to(dev))).cpu()
    assert (deq - O.dequant_soft(c["sample"], c["cb"])).abs().max().item() < 1e-6
    record(f"soft_assign_sample[k={k}]", seed=SAMPLE_SEEDS[k], entries_within_1e6_of_threshold=c["near"], dropped=int(dropped.sum()))


# ---- the chain as autograd sees it --------------------------------------------------------------------------------------------------------
CHAIN_SEEDS = {(3, 2049, 10): 0, (2, 8193, 16): 0}


def chain_case(m, k, d, seed):
    n, (h, w) = 1, ((2, 2) if m == 3 else (2, 3))                         # twelve rows
    x, cb, temp, freq, expo, u1, u2 = _level_case(m, k, d, n, h, w, seed)
    g = torch.Generator().manual_seed(seed + 77)
    wd = torch.randn((n, m * d, h, w), generator=g)
    wl = (torch.rand((n, m, h, w, k), generator=g) - 0.5) * 0.05
    return dict(x=x, cb=cb, temp=temp, freq=freq, expo=expo, u1=u1, u2=u2, wd=wd, wl=wl)


def chain_oracle(c, dtype, logit_loss):
    """The level through the oracle's vq_logit, random_drop, gumbel_softmax_hard and dequant_soft in `dtype`, loss = sum deq Wd
    (+ sum logits Wl): (dx, dcodebook, dtemperature), the discrete results, and the scale of dtemperature -- per group
    sum |dz raw / T| over its rows and codewords, dz the gradient at the raw logits (the temperature term cancels like dtrow)."""
    x, cb, temp = (c[n].to(dtype).clone().requires_grad_() for n in ("x", "cb", "temp"))
    raw = O.vq_logit(x, cb, temp, torch.tensor([BOUND], dtype=dtype))
    raw.retain_grad()
    post = O.random_drop(raw, c["freq"].to(dtype), c["u1"].to(dtype))
    sample, _, index = O.gumbel_softmax_hard(post, c["u2"].to(dtype))
    deq = O.dequant_soft(sample, cb)
    loss = (deq * c["wd"].to(dtype)).sum()
    if logit_loss:
        loss = loss + (post * c["wl"].to(dtype)).sum()
    loss.backward()
    dt_scale = (raw.grad * raw.detach() / temp.detach()[None, :, :, :, :]).abs().sum((0, 2, 3, 4)).reshape(temp.shape)
    return dict(dx=x.grad, dcb=cb.grad, dt=temp.grad, deq=deq.detach(), code=post.argmax(-1), index=index[..., 0], dropped=post.detach() < -1e8, dt_scale=dt_scale)


def chain_clean(c):
    a, b = chain_oracle(c, torch.float32, False), chain_oracle(c, torch.float64, False)
    return all(torch.equal(a[n], b[n]) for n in ("code", "index", "dropped"))


@pytest.mark.parametrize("logit_loss", [False, True])
@pytest.mark.parametrize("mkd", sorted(CHAIN_SEEDS))
def test_soft_quantize_chain(dev, mkd, logit_loss):
    """SoftQuantizeFn (logits, sample, soft dequantisation forward; vq_inner, vq_softmax_bwd, vq_soft_bwd, vq_temperature_grad
    backward) at the first k of the 1024-thread row form and of the wave-per-row form, twelve rows, against the oracle's level in
    float64 with the same draws.  Codes and sample index are the oracle's (seeds fixed such that its float32 and float64 runs
    agree on them and on every drop, rechecked here); dx and dcodebook are measured relative to the largest entry of the float64
    tensor -- a d- resp. k-term contraction without a cancelling structure of its own, the scale the whole-model gradient tests use --
    and dtemperature relative to sum |dz raw / T| of its group.  Yardstick: the oracle's level in float32 on the CPU.

    Measured on an MI355X, all twelve figures inside their bars: dx e_hip 1.6e-7 .. 3.8e-7 (e_f32 2.5e-7 .. 4.9e-7), dcodebook
    2.5e-8 .. 4.8e-8 (3.8e-8 .. 7.2e-8), dtemperature 1.3e-9 .. 5.4e-8 (5.7e-10 .. 5.3e-8).

    This test found a defect.  vq_dx_kernel -- the form taken when k is no multiple of 16 -- contracted d dist with the codebook in
    one float32 chain over all k; with a gradient on the logits every one of the k terms is of like size, and dx came out at
    2.283e-6 against e_f32 2.729e-7 at (2, 8193, 16) (bar 1.092e-6), 1.465e-6 without the logit loss.  Neither a more accurate
    Gumbel logarithm nor the better-conditioned d dist moved those figures; summing in runs of 64 codewords gives 2.980e-7 and
    3.452e-7."""
    from mcquic_amd import ops
    from mcquic_amd.autograd import SoftQuantizeFn
    m, k, d = mkd
    c = chain_case(m, k, d, CHAIN_SEEDS[mkd])
    assert bool((c["temp"] > BOUND).all())
    assert chain_clean(c), f"{mkd} seed {CHAIN_SEEDS[mkd]}: the float32 and float64 oracle runs differ in a decision"
    want, f32 = chain_oracle(c, torch.float64, logit_loss), chain_oracle(c, torch.float32, logit_loss)
    x, cb, temp = (c[n].to(dev).requires_grad_() for n in ("x", "cb", "temp"))
    deq, code, logits, _ = SoftQuantizeFn.apply(x, cb, temp, c["freq"].to(dev), c["u1"].to(dev), c["u2"].to(dev), c["expo"].reshape(1).to(dev),
                                                ops.PackedCodebook(cb.detach()), BOUND)
    assert torch.equal(code.cpu(), want["code"])
    assert torch.equal(logits.detach().cpu() < -1e8, want["dropped"])
    assert (deq.detach().cpu() - want["deq"]).abs().max().item() < 1e-6   # the sample index: another one is another codeword, off by ~0.1
    loss = (deq * c["wd"].to(dev)).sum()
    if logit_loss:
        loss = loss + (logits * c["wl"].to(dev)).sum()
    loss.backward()
    got = dict(dx=x.grad.cpu(), dcb=cb.grad.cpu(), dt=temp.grad.cpu())
    scales = dict(dx=want["dx"].abs().max(), dcb=want["dcb"].abs().max(), dt=want["dt_scale"])
    for name in ("dx", "dcb", "dt"):
        assert got[name].shape == want[name].shape
        _bar(f"soft_assign_chain[m{m}-k{k}-d{d},logit_loss={logit_loss}].{name}", R.scaled_err(got[name], want[name], scales[name]),
             R.scaled_err(f32[name], want[name], scales[name]))
