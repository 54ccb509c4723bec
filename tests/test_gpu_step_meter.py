"""mcquic_amd.monitor.StepMeter (csrc/step_meter.hip) alone: every column of its rows against tests/_meter_ref.py (float64, written from the
formulas and the reference), integers and carried bits exactly, over the level sets and count patterns of tests/_meter_cases.py; the ring,
the watchdog, capture and determinism.

Bars of the float columns: 4 x the worst relative error measured on an MI355X over exactly these cases (docs/experiments.md section 19,
profiles/step_meter_errors.json); a reference value of 0 must be met exactly."""
import math

import numpy as np
import pytest
import torch

import _meter_cases as C
import _meter_ref as M
from _record import record

pytestmark = pytest.mark.gpu
PIXELS = 3 * 64 * 64
# Worst relative errors measured on an MI355X over the five level sets x five count patterns below; the test holds 4 x these.  They are
# float32's rounding of the stored value (2^-24 = 6.0e-8): the kernels form their sums in double.  `ema_entropy` and `step_bits` cover the
# per-(level, group) partials as well as the row's columns.  The same sums in float32 numpy: 1e-5 (bpp), 5e-5 (step_entropy), 3e-3
# (ema_entropy, from x log2 x next to x = 1), tests/test_meter_ref.py.
MEASURED = {"db": 1.382e-7, "ema_entropy": 4.789e-8, "step_bits": 5.632e-8, "code_usage": 4.080e-8, "bpp": 6.590e-8, "usage": 3.113e-8,
            "hit": 2.957e-8, "step_entropy": 6.572e-8}
BARS = {k: 4 * v for k, v in MEASURED.items()}


def _meter(dev, levels, seed=11, **kw):
    from mcquic_amd import monitor
    from mcquic_amd.modules.entropyCoder import VariousMCoder
    coder = VariousMCoder([m for m, _ in levels], [k for _, k in levels]).to(dev)
    f = C.freqs(levels, seed)
    with torch.no_grad():
        for p, t in zip(coder._freqEMA, f):
            p.copy_(torch.from_numpy(t))
    kw.setdefault("capacity", 8)
    kw.setdefault("pixels", PIXELS)
    return monitor.StepMeter(coder, **kw), coder, f


def _flat(counts, dev):
    return torch.from_numpy(np.concatenate([c.reshape(-1) for c in counts])).to(dev)


def _f32(x, dev):
    return torch.tensor(float(x), dtype=torch.float32, device=dev)


def _rel(got, want, col, worst, where):
    """Relative error of one float column against float64; an exact 0 is required where the reference is 0."""
    got, want = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(want, dtype=np.float64).reshape(-1)
    assert np.isfinite(got).all(), (col, where, got)
    zero = want == 0
    assert (got[zero] == 0).all(), (col, where, got, want)
    if (~zero).any():
        err = float(np.max(np.abs(got[~zero] - want[~zero]) / np.abs(want[~zero])))
        worst[col] = max(worst.get(col, 0.0), err)


@pytest.mark.parametrize("name", list(C.LEVEL_SETS))
def test_rows_against_float64(dev, name):
    levels = C.LEVEL_SETS[name]
    meter, coder, f = _meter(dev, levels)
    losses = C.losses(len(C.COUNT_KINDS), 3)
    worst, shadow = {}, np.float32("nan")
    skipped = torch.zeros((), dtype=torch.int64, device=dev)
    for it, kind in enumerate(C.COUNT_KINDS):
        counts = C.counts(levels, kind, 20 + it)
        gn, lr = np.float32(0.5 + it), np.float32(1e-4 * (it + 1))
        skipped.fill_(it * 3)
        meter.update(_f32(losses[it], dev), _flat(counts, dev), grad_norm=_f32(gn, dev), lr=_f32(lr, dev), skipped=skipped)
        want, parts = M.row(f, counts, float(losses[it]), PIXELS)
        got_parts = {k: v.cpu().numpy() for k, v in meter.partials().items()}
        r = meter.read()
        assert r["steps"].tolist() == [it] and r["count"] == it + 1 and r["dropped"] == 0 and r["first_bad_step"] == -1
        # integers: exact
        for key, i in (("used", 0), ("hit", 2), ("total", 3)):
            ref = np.concatenate([p[i] for p in parts])
            assert got_parts[key].tolist() == ref.tolist(), (key, kind)
        assert r["skipped"][0] == it * 3
        # inputs: their bits
        assert r["loss"][0].tobytes() == losses[it].tobytes() and r["grad_norm"][0].tobytes() == gn.tobytes() and r["lr"][0].tobytes() == lr.tobytes()
        # the shadow: bit for bit the float32 recurrence fed the kernel's own db
        shadow = M.ema_f32(shadow, r["db"][0])
        assert r["db_ema"][0].tobytes() == shadow.tobytes(), (kind, r["db_ema"][0], shadow)
        # floats
        _rel(r["db"], want[1], "db", worst, kind)
        _rel(got_parts["ema_entropy"], np.concatenate([p[1] for p in parts]), "ema_entropy", worst, kind)
        _rel(got_parts["step_bits"], np.concatenate([p[4] for p in parts]), "step_bits", worst, kind)
        _rel(r["code_usage"], want[6], "code_usage", worst, kind)
        _rel(r["bpp"], want[7], "bpp", worst, kind)
        for j, col in enumerate(("usage", "ema_entropy", "hit", "step_entropy")):
            _rel(r[col][0], want[M.HEAD + j:: 4], col, worst, kind)
        # the patterns' own properties
        if kind == "zero-group":
            assert got_parts["hit"][0] == 0 and got_parts["total"][0] == 0 and got_parts["step_bits"][0] == 0
        if kind == "one-hot":
            row = sum(m for m, _ in levels[:-1])
            assert got_parts["hit"][row] == 1 and got_parts["total"][row] == 7 and got_parts["step_bits"][row] == 0
        if kind == "uniform":
            for l, (m, k) in enumerate(levels):
                assert r["hit"][0, l] == 1.0
                if k & (k - 1) == 0:
                    assert r["step_entropy"][0, l] == math.log2(k), (l, k)
        if kind == "above-2^24":
            assert got_parts["total"][0] == int(counts[0][0].sum()) > 1 << 24
    # (`used` above is exact with entry 1 of every row with k >= 3 just over CodeUsage's threshold and entry 2 just under it:
    #  tests/test_meter_ref.py checks that the tables are built so)
    for key, val in worst.items():
        record(f"step_meter/{name}/{key}", value=val, bar=BARS[key])
    print(name, {k: f"{v:.3e}" for k, v in worst.items()})
    for key, val in worst.items():
        assert val <= BARS[key], (name, key, val, BARS[key])


def test_optional_inputs_and_host_lr(dev):
    """Without gradient norm and learning rate the columns are NaN, without `skipped` 0; a host learning rate is recorded as given."""
    levels = C.LEVEL_SETS["2x3"]
    meter, _, _ = _meter(dev, levels)
    c = _flat(C.counts(levels, "random", 1), dev)
    meter.update(_f32(0.1, dev), c)
    meter.update(_f32(0.1, dev), c, lr=0.25)
    r = meter.read()
    assert np.isnan(r["grad_norm"]).all() and np.isnan(r["lr"][0]) and r["lr"][1] == 0.25 and (r["skipped"] == 0).all()
    assert r["first_bad_step"] == -1
    with pytest.raises(RuntimeError, match="HIP device"):
        meter.update(torch.tensor(0.1), c)
    with pytest.raises(ValueError):
        meter.update(_f32(0.1, dev), c[:-1])


def test_ring_and_checkpoint(dev):
    """Capacity 4, 6 updates: steps 2-5 in order, 2 dropped; nothing on a second read; a fresh meter loaded with the state continues at 6,
    with the shadow's bits."""
    levels = C.LEVEL_SETS["64+257"]
    meter, _, _ = _meter(dev, levels, capacity=4)
    c = _flat(C.counts(levels, "random", 1), dev)
    losses = C.losses(7, 9)
    for it in range(6):
        meter.update(_f32(losses[it], dev), c)
    r = meter.read()
    assert r["steps"].tolist() == [2, 3, 4, 5] and r["dropped"] == 2 and r["count"] == 6
    assert r["loss"].tobytes() == losses[2:6].tobytes()
    assert r["usage"].shape == (4, 2)
    again = meter.read()
    assert again["steps"].size == 0 and again["dropped"] == 0 and again["loss"].size == 0 and again["usage"].shape == (0, 2)
    fresh, _, _ = _meter(dev, levels, capacity=4)
    fresh.load_state_dict(meter.state_dict())
    fresh.update(_f32(losses[6], dev), c)
    meter.update(_f32(losses[6], dev), c)
    a, b = fresh.read(), meter.read()
    assert a["steps"].tolist() == b["steps"].tolist() == [6] and a["dropped"] == 0
    assert a["db_ema"].tobytes() == b["db_ema"].tobytes() and a["count"] == 7
    other, _, _ = _meter(dev, levels, capacity=5)
    with pytest.raises(RuntimeError):
        other.load_state_dict(meter.state_dict())


def test_warm_leaves_every_bit(dev):
    levels = C.LEVEL_SETS["2x3"]
    meter, _, _ = _meter(dev, levels, capacity=4)
    c = _flat(C.counts(levels, "random", 1), dev)
    for it in range(3):
        meter.update(_f32(0.2 + 0.1 * it, dev), c)
    before = meter._buf.clone()
    meter.warm()
    assert torch.equal(meter._buf, before)
    virgin, _, _ = _meter(dev, levels, capacity=4)
    before = virgin._buf.clone()
    virgin.prepare()
    virgin.warm()
    assert torch.equal(virgin._buf, before) and int(virgin.first_bad_step) == -1       # (NaN shadow: compared as words)


def test_watchdog(dev):
    levels = C.LEVEL_SETS["2x3"]
    c = _flat(C.counts(levels, "random", 1), dev)
    meter, _, _ = _meter(dev, levels)
    for it in range(6):
        meter.update(_f32(float("nan") if it == 3 else 0.1, dev), c, grad_norm=_f32(1.0, dev))
        assert int(meter.first_bad_step) == (-1 if it < 3 else 3)
        if it < 3:
            meter.check()
    with pytest.raises(RuntimeError, match="Loss becomes NAN. Train crashed."):
        meter.check()
    r = meter.read()
    assert np.isnan(r["db_ema"][3]) and np.isfinite(r["db_ema"][4:]).all()      # EMATracker starts over from a NaN shadow
    # a gradient norm that is not finite
    meter, _, _ = _meter(dev, levels)
    meter.update(_f32(0.1, dev), c, grad_norm=_f32(1.0, dev))
    meter.update(_f32(0.1, dev), c, grad_norm=_f32(float("inf"), dev))
    assert int(meter.first_bad_step) == 1
    # the shadow under the floor: loss 0.99 is 0.044 dB
    meter, _, _ = _meter(dev, levels)
    meter.update(_f32(0.99, dev), c)
    assert int(meter.first_bad_step) == 0
    meter, _, _ = _meter(dev, levels, floor=None)
    meter.update(_f32(0.99, dev), c)
    assert int(meter.first_bad_step) == -1
    meter.update(_f32(float("inf"), dev), c)
    assert int(meter.first_bad_step) == 1


def test_captured_update_reads_its_inputs_at_replay(dev):
    """`update` recorded once on a side stream, replayed three times with loss, counts and the learning-rate TENSOR changed in between:
    the rows of three eager updates.  A value baked in at capture would repeat the first row."""
    levels = C.LEVEL_SETS["various-m"]
    eager, _, _ = _meter(dev, levels)
    graphed, _, _ = _meter(dev, levels)
    losses = C.losses(3, 4)
    loss, lr = _f32(0.0, dev), _f32(0.0, dev)
    gn, skipped = _f32(2.0, dev), torch.zeros((), dtype=torch.int64, device=dev)
    counts = torch.zeros(graphed.entries, dtype=torch.int64, device=dev)
    graphed.prepare()
    graphed.warm()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        graphed.update(loss, counts, grad_norm=gn, lr=lr, skipped=skipped)
    assert int(graphed._count) == 0                            # (a capture runs nothing)
    for it in range(3):
        c = _flat(C.counts(levels, C.COUNT_KINDS[it], 30 + it), dev)
        loss.fill_(float(losses[it])); lr.fill_(1e-3 / (it + 1)); gn.fill_(2.0 + it); skipped.fill_(it); counts.copy_(c)
        g.replay()
        eager.update(loss, c, grad_norm=gn, lr=lr, skipped=skipped)
    a, b = graphed.read(), eager.read()
    assert a["steps"].tolist() == [0, 1, 2]
    for key in b:
        assert np.asarray(a[key]).tobytes() == np.asarray(b[key]).tobytes(), key
    assert len(set(a["lr"].tolist())) == 3 and len(set(a["bpp"].tolist())) == 3 and len(set(a["loss"].tolist())) == 3


def test_same_inputs_same_bits(dev):
    levels = C.LEVEL_SETS["product"]
    rows = []
    for _ in range(2):
        meter, _, _ = _meter(dev, levels)
        for it in range(2):
            meter.update(_f32(0.3, dev), _flat(C.counts(levels, "random", 5 + it), dev), grad_norm=_f32(1.5, dev), lr=3e-4)
        rows.append(meter._buf.clone())
    assert torch.equal(rows[0], rows[1])
