"""GPU: every weight-gradient kernel form, launched through the C ABI into buffers the test owns, against the exact and float64
references of tests/_wgrad_refs.py (held to float64 autograd by tests/test_wgrad_refs.py).

The forms (tests/_wgrad_cases.py; tests/test_wgrad_plan.py holds each strip-walk case's plan features as literals): the 3x3, stride-2
and 1x1 strip walks of csrc/wgrad_rows.hip at F = 4 and 8, with one and several row ranges, one and several walks per wave, full and
ragged last workgroups, grouped launches planned like the single one, by the shared wave budget and by the whole-launch search; its
small-map LDS kernel; the 16 x 16-tile kernel of csrc/wgrad_t16.h (3x3 single and grouped, 1x1 plain and squared); the NHWC form of
csrc/train_ops.hip behind mcq_nchw_to_nhwc_pair_f32, per-lane and wave-uniform pixel walk.

Every launch: dW, db and the workspace each sit in an allocation of their own between 4096 sentinel floats, the workspace exactly
the size the query states (nconv x for a grouped launch, 1 float for the one-pass forms; the NHWC copies count as workspace), all
three filled with NaN first -- a partial tile or bias partial the launch never writes, or an output entry it skips, arrives as NaN.
Afterwards: sentinels unchanged bit for bit, no NaN in dW / db, x and dy equal to their clones, a second identical launch into fresh
NaN-filled buffers returns the same bits (every form's source claims determinism, the NHWC form's header included: "a second,
deterministic pass (no atomics)" -- no exception is made), and a launch with a null db returns the same dW bits.  The route is
asserted before the launch (workspace queries == 1 / > 1 / == 0, the plan query).

Two data sets per case and variant:
  (i)  integers of [-3, 3] as float32: every partial sum in any order is an integer below 2^24, so dW and db must EQUAL wgrad_int --
       a dropped, doubled or misplaced pixel, a wrong border tap or tile mask shows whatever its size;
  (ii) uniform floats of [-1, 1): e = max |got - wgrad64| / wgrad_scale64 for the kernel and for wgrad_seq_f32 (ONE float32 chain over
       all pixels: every form sums shorter chains and folds them), e_hip <= max(4 e_seq, 1.2e-7), the bar and floor of
       tests/test_gpu_conv_epilogues.py.
Grouped launches: problem c holds the data rolled by c channels (its references are the single problem's, rolled), every problem is
held to (i) / (ii); a second launch replaces the last problem by a copy of problem 0 and problem 1's dbias entry by NULL: equal data
give equal bits, the others the first launch's bits.

Measured on an MI355X (profiles/r11_wgrad_leaf_errors.json, 50 entries wgrad_leaf[<case>[+sq][ n<nconv>]]): the one-chain sum is a
yardstick for these kernels -- the worst e_hip / e_seq is 1.09 (the one-walk 3x3 launch rows3_f4_1x8x8, 2.06e-7 against 1.88e-7, and
the small-map kernel at 6 x 7, whose fma chain over the pixels is the yardstick's own order: 1.00 at the other two maps); the 16 x 16
tiles reach 0.25 .. 0.99, the NHWC form 0.27 .. 0.97, the strip walks with several walks 0.19 .. 0.88.  The integer data set is exact
in every form, grouped launches included; no kernel changed with this test."""
import ctypes

import pytest
import torch

import _wgrad_cases as K
import _wgrad_refs as W
from _record import record

pytestmark = pytest.mark.gpu

GUARD = 4096
SENTINEL = -12345.678
FLOOR = 1.2e-7
NAN = float("nan")


class _Guarded:
    """`numel` floats filled with NaN between GUARD sentinel floats on both sides, one allocation."""

    def __init__(self, numel, dev):
        self.numel = int(numel)
        self.buf = torch.full((2 * GUARD + self.numel,), SENTINEL, dtype=torch.float32, device=dev)
        self.view = self.buf[GUARD:GUARD + self.numel]
        self.view.fill_(NAN)
        self.ptr = self.view.data_ptr()

    def intact(self):
        bits = self.buf.view(torch.int32)
        want = torch.tensor([SENTINEL], dtype=torch.float32).view(torch.int32).item()
        return bool((bits[:GUARD] == want).all() & (bits[GUARD + self.numel:] == want).all())


_QUERY = {"rows3": "mcq_conv2d_wgrad_nchw_workspace_floats", "tiny": "mcq_conv2d_wgrad_nchw_workspace_floats",
          "t16_3": "mcq_conv2d_wgrad_nchw_workspace_floats", "s2": "mcq_conv2d_wgrad_s2_nchw_workspace_floats",
          "rows1": "mcq_conv2d_wgrad1x1_nchw_workspace_floats", "t16_1": "mcq_conv2d_wgrad1x1_nchw_workspace_floats"}


def _route(lib, case, nconv):
    """Asserts the route the case takes and returns the workspace floats of the launch."""
    dims = (case.n, case.cin, case.h, case.w, case.cout)
    taps, s2 = case.ks * case.ks, case.stride == 2
    out = (ctypes.c_int32 * 9)()
    planned = lib.mcq_conv2d_wgrad_nchw_plan(*dims, taps, int(s2), nconv, out)
    if case.form == "nhwc":
        rows = {(3, 1): lib.mcq_conv2d_wgrad_nchw_workspace_floats, (3, 2): lib.mcq_conv2d_wgrad_s2_nchw_workspace_floats,
                (1, 1): lib.mcq_conv2d_wgrad1x1_nchw_workspace_floats}[(case.ks, case.stride)]
        assert rows(*dims) == 0 and planned == 0, f"{case.name}: meant for the NHWC form"
        nws = lib.mcq_conv2d_wgrad_workspace_floats(*dims, case.ks, case.stride)
        assert nws > 0
        return nws
    one = getattr(lib, _QUERY[case.form])(*dims)
    if case.form in K.STRIP_FORMS:
        assert one > 1 and planned == 1, f"{case.name}: meant for the strip walk"
        groups, gmax = out[7], out[8]
        want = case.plan[nconv]
        assert (out[0], out[2] > 1, out[6] > 1, out[5] % 4 != 0) == (want["F"], want["chunks"], want["ups"], want["ragged"]), f"{case.name}: plan {list(out)}"
        assert groups <= gmax and nconv * groups * (taps * case.cout * case.cin + 4 * case.cout) <= nconv * one
        return nconv * one
    assert one == 1 and planned == 0, f"{case.name}: meant for a one-pass kernel"
    assert (case.cin % 16 == 0 and case.cout % 16 == 0) == case.form.startswith("t16"), case.name
    return 1


def _launch(lib, dev, case, square, xs, dys, bias):
    """One launch of len(xs) problems (device tensors); bias: per problem, whether db is asked for.  All checks of a single launch;
    returns [(dW, db or None)] on the CPU."""
    nconv = len(xs)
    n, cin, h, w, cout, ks = case.n, case.cin, case.h, case.w, case.cout, case.ks
    nws = _route(lib, case, nconv)
    keep_x, keep_d = [t.clone() for t in xs], [t.clone() for t in dys]
    dws = [_Guarded(cout * cin * ks * ks, dev) for _ in range(nconv)]
    dbs = [_Guarded(cout, dev) if b else None for b in bias]
    ws = _Guarded(nws, dev)
    guarded = dws + [b for b in dbs if b is not None] + [ws]
    dbp = [b.ptr if b is not None else None for b in dbs]
    if case.form == "nhwc":
        assert nconv == 1
        ho, wo = W.out_hw(h, w, ks, case.stride)
        xt, dyt = _Guarded(xs[0].numel(), dev), _Guarded(dys[0].numel(), dev)
        guarded += [xt, dyt]
        rc = lib.mcq_nchw_to_nhwc_pair_f32(xs[0].data_ptr(), xt.ptr, cin, h * w, int(square), dys[0].data_ptr(), dyt.ptr, cout, ho * wo, n, None)
        assert rc == 0, f"{case.name}: mcq_nchw_to_nhwc_pair_f32 returned {rc}"
        rc = lib.mcq_conv2d_wgrad_f32(xt.ptr, dyt.ptr, dws[0].ptr, dbp[0], ws.ptr, n, cin, h, w, cout, ks, case.stride, None)
    elif case.form == "s2":
        assert nconv == 1 and not square
        rc = lib.mcq_conv2d_wgrad_s2_nchw_f32(xs[0].data_ptr(), dys[0].data_ptr(), dws[0].ptr, dbp[0], ws.ptr, n, cin, h, w, cout, None)
    elif case.ks == 1:
        assert nconv == 1
        rc = lib.mcq_conv2d_wgrad1x1_nchw_f32(xs[0].data_ptr(), dys[0].data_ptr(), dws[0].ptr, dbp[0], ws.ptr, n, cin, h, w, cout, int(square), None)
    elif nconv == 1:
        assert not square
        rc = lib.mcq_conv2d_wgrad_nchw_f32(xs[0].data_ptr(), dys[0].data_ptr(), dws[0].ptr, dbp[0], ws.ptr, n, cin, h, w, cout, None)
    else:
        assert not square
        table = ctypes.c_void_p * nconv
        rc = lib.mcq_conv2d_wgrad_nchw_group_f32(table(*[t.data_ptr() for t in xs]), table(*[t.data_ptr() for t in dys]), table(*[g.ptr for g in dws]),
                                                 table(*dbp) if any(bias) else None, nconv, ws.ptr, n, cin, h, w, cout, None)
    torch.cuda.synchronize()
    assert rc == 0, f"{case.name}: launch returned {rc}"
    assert all(g.intact() for g in guarded), f"{case.name} nconv {nconv}: a sentinel was written"
    assert all(torch.equal(a, b) for a, b in zip(xs + dys, keep_x + keep_d)), f"{case.name}: an input was written"
    out = []
    for c in range(nconv):
        dw, db = dws[c].view.cpu().reshape(cout, cin, ks, ks), (None if dbs[c] is None else dbs[c].view.cpu())
        assert not bool(torch.isnan(dw).any()), f"{case.name} problem {c}: NaN in dW (an entry or a partial tile never written)"
        assert db is None or not bool(torch.isnan(db).any()), f"{case.name} problem {c}: NaN in db (a bias partial never written)"
        out.append((dw, db))
    return out


def _same_bits(a, b):
    return all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for pair_a, pair_b in zip(a, b) for p, q in zip(pair_a, pair_b) if p is not None and q is not None)


def _rolled(t, c):
    return torch.roll(t, c, dims=1).contiguous()


def _ref_rolled(dw, db, c):
    return torch.roll(dw, (c, c), dims=(0, 1)), torch.roll(db, c, dims=0)


@pytest.mark.parametrize("case", K.CASES, ids=[c.name for c in K.CASES])
def test_wgrad_leaf(dev, case):
    from mcquic_amd import _lib
    lib = _lib.load()
    failures = []
    for square in K.squares(case):
        tag = case.name + ("+sq" if square else "")
        for kind in ("int", "uniform"):
            make = W.int_inputs if kind == "int" else W.uniform_inputs
            x, dy = make(case.n, case.cin, case.h, case.w, case.cout, case.ks, case.stride, K.seed(case) + (kind == "uniform"))
            if kind == "int":
                iw, ib = W.wgrad_int(x, dy, case.ks, case.stride, square)
                refs = (iw.to(torch.float32), ib.to(torch.float32))
            else:
                w64, b64 = W.wgrad64(x, dy, case.ks, case.stride, square)
                sw, sb = W.wgrad_scale64(x, dy, case.ks, case.stride, square)
                qw, qb = W.wgrad_seq_f32(x, dy, case.ks, case.stride, square)
                e_seq = max(W.rel_err(qw, w64, sw), W.rel_err(qb, b64, sb))
                bar = max(4 * e_seq, FLOOR)

            def hold(results, what, shifts):
                """Every problem of a launch against its (rolled) references."""
                worst = 0.0
                for (dw, db), c in zip(results, shifts):
                    if kind == "int":
                        rw, rb = _ref_rolled(*refs, c)
                        bad = int((dw != rw).sum()) + (0 if db is None else int((db != rb).sum()))
                        if bad:
                            failures.append(f"{what} problem shift {c}: {bad} entries differ from the integer sums "
                                            f"(max |diff| {float((dw - rw).abs().max())})")
                    else:
                        rw, rb = _ref_rolled(w64, b64, c)
                        zw, zb = _ref_rolled(sw, sb, c)
                        worst = max(worst, W.rel_err(dw, rw, zw), 0.0 if db is None else W.rel_err(db, rb, zb))
                if kind == "uniform":
                    record(f"wgrad_leaf[{what}]", form=case.form, e_hip=worst, e_seq=e_seq, ratio=worst / e_seq if e_seq else 0.0, bar=bar)
                    print(f"wgrad_leaf[{what}] e_hip {worst:.3e} e_seq {e_seq:.3e} ratio {worst / e_seq if e_seq else 0.0:.2f} bar {bar:.3e}")
                    if not worst <= bar:
                        failures.append(f"{what}: e_hip {worst:.3e} > max(4 e_seq, floor) = {bar:.3e} (e_seq {e_seq:.3e})")

            for nconv in case.nconvs:
                what = f"{tag}{'' if nconv == 1 else f' n{nconv}'}"
                shifts = list(range(nconv))
                xs, dys = [_rolled(x, c).to(dev) for c in shifts], [_rolled(dy, c).to(dev) for c in shifts]
                first = _launch(lib, dev, case, square, xs, dys, [True] * nconv)
                hold(first, f"{what} {kind}" if kind == "int" else what, shifts)
                again = _launch(lib, dev, case, square, xs, dys, [True] * nconv)
                assert _same_bits(first, again), f"{what} {kind}: a second identical launch gives other bits"
                if nconv == 1:
                    nodb = _launch(lib, dev, case, square, xs, dys, [False])
                    assert nodb[0][1] is None and _same_bits([(first[0][0], None)], [(nodb[0][0], None)]), f"{what} {kind}: a null db changes dW"
                else:
                    # the last problem a copy of problem 0, problem 1 without a db; then a table without any db
                    xs2, dys2 = xs[:-1] + [xs[0].clone()], dys[:-1] + [dys[0].clone()]
                    bias = [c != 1 for c in shifts]
                    second = _launch(lib, dev, case, square, xs2, dys2, bias)
                    assert second[1][1] is None
                    assert _same_bits(first[:-1], second[:-1]), f"{what} {kind}: the launch with a null dbias entry gives other bits"
                    assert _same_bits([second[0]], [second[-1]]), f"{what} {kind}: equal data in two problems, unequal bits"
                    nodb = _launch(lib, dev, case, square, xs, dys, [False] * nconv)
                    assert _same_bits([(a[0], None) for a in first], [(a[0], None) for a in nodb]), f"{what} {kind}: a null dbias table changes dW"
    assert not failures, "\n".join(failures)
