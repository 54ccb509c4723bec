"""tests/_meter_ref.py (the float64 restatement the StepMeter kernels are held to) against the code it restates -- `Compressor.CodeUsage`'s
torch formula, `validate.ideal_bpp`, the reference's three-line EMATracker -- plus the host-side contract of mcquic_amd.monitor: ABI number,
no CPU path.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import _meter_cases as C
import _meter_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tables(ms, ks, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for m, k in zip(ms, ks):
        f = torch.rand((m, k), generator=g)
        f = torch.where(torch.rand((m, k), generator=g) < 0.4, torch.zeros_like(f), f)
        f[:, 0] += 0.5
        out.append(f)
    return out


@pytest.mark.parametrize("ms,ks", [([2, 2, 2], [64, 32, 16]), ([4, 1], [65, 1023]), ([1], [1])])
def test_code_usage_is_the_compressors_formula(ms, ks):
    """compressor.py:211-212 over `NormalizedFreq` (entropyCoder.py: f / f.sum(-1)), in torch float32, on tables whose entries are 0 or far
    from the threshold."""
    from mcquic_amd.modules.entropyCoder import VariousMCoder
    coder = VariousMCoder(ms, ks)
    tables = _tables(ms, ks, 3)
    with torch.no_grad():
        for p, f in zip(coder._freqEMA, tables):
            p.copy_(f)
    want = torch.cat(list((freq > 1e-6).flatten() for freq in coder.NormalizedFreq)).float().mean()
    counts = [np.ones((m, k), dtype=np.int64) for m, k in zip(ms, ks)]
    got, _ = M.row([f.numpy() for f in tables], counts, 0.1, 1)
    assert 0 < float(want) < 1 or ks == [1]
    assert np.float32(got[6]) == np.float32(float(want))


def test_bpp_is_ideal_bpp():
    from mcquic_amd import validate
    levels = C.LEVEL_SETS["64+257"]
    for kind in C.COUNT_KINDS[:4]:                            # (ideal_bpp works in float32: not for counts above 2^24)
        counts = C.counts(levels, kind, 5)
        if kind == "zero-group":                              # (0 / 0 there: the reference's handler never sees an empty group)
            counts[0][0, 3] = 1
        want = validate.ideal_bpp([torch.from_numpy(c) for c in counts], 4096)
        got, _ = M.row(C.freqs(levels, 1), counts, 0.1, 4096)
        assert abs(got[7] - want) <= 1e-5 * abs(want), (kind, got[7], want)


@pytest.mark.parametrize("momentum", [0.99, 0.9])
def test_recurrence_is_the_references_ematracker(momentum):
    """validate/utils.py:15-28, restated in three lines of torch, NaN-initialised first call included: bit for bit."""
    shadow = torch.empty(()) * torch.nan
    decay = 1 - momentum
    ours = np.float32("nan")
    for x in torch.from_numpy(M.decibel(C.losses(60, 2)).astype(np.float32)):
        if torch.all(torch.isnan(shadow)):
            shadow.copy_(x)
        else:
            shadow -= decay * (shadow - x)
        ours = M.ema_f32(ours, x.numpy(), momentum)
        assert ours.tobytes() == shadow.numpy().tobytes()
    assert np.isnan(M.ema_f32(ours, np.float32("nan"), momentum))
    assert M.ema_f32(np.float32("nan"), np.float32(3.5), momentum) == np.float32(3.5)      # a NaN shadow starts over


def test_float32_restatement_is_within_rounding_of_float64():
    """What evaluating the same sums in float32 costs, over the GPU test's cases: the figure the kernel's error is read against.  Sums of at
    most 8192 non-negative terms of a few ulp each stay near 1e-5; the exception is x log2 x next to x = 1, conditioned like 1 / |ln x|:
    the 3-entry rows of "2x3" have p = 1 - 2e-6, so float32's 6e-8 on p becomes up to 6e-8 * 5e5 = 3e-2 of that term, which is most
    of the row's entropy.  (The kernel therefore forms these terms in double.)"""
    worst = {}
    for name, levels in C.LEVEL_SETS.items():
        f = C.freqs(levels, 11)
        for kind in C.COUNT_KINDS:
            c = C.counts(levels, kind, 12)
            a, _ = M.row(f, c, 0.1, 1000.0, dtype=np.float32)
            b, _ = M.row(f, c, 0.1, 1000.0)
            for i in range(6, len(b)):
                col = ("code_usage", "bpp")[i - 6] if i < 8 else ("usage", "ema_entropy", "hit", "step_entropy")[(i - 8) % 4]
                if b[i] == 0:
                    assert a[i] == 0, (name, kind, col)
                else:
                    worst[col] = max(worst.get(col, 0.0), abs(a[i] - b[i]) / abs(b[i]))
    print("float32 numpy against float64, worst relative error per column:", {k: f"{v:.2e}" for k, v in worst.items()})
    assert max(v for k, v in worst.items() if k != "ema_entropy") < 1e-4 and worst["ema_entropy"] < 3e-2


def test_threshold_entries_fall_on_their_sides():
    """The frequency tables of the GPU test hold what they claim: entry 1 of a row above CodeUsage's threshold, entry 2 below, in float64."""
    for levels in C.LEVEL_SETS.values():
        for f, (m, k) in zip(C.freqs(levels, 11), levels):
            if k >= 3:
                p = f.astype(np.float64) / f.astype(np.float64).sum(-1, keepdims=True)
                assert (p[:, 1] > 1e-6).all() and (p[:, 2] < 1e-6).all() and (p[:, 2] > 0.999999e-6).all()


def test_abi_version_of_header_and_binding():
    from mcquic_amd import _lib
    header = open(os.path.join(ROOT, "include", "mcquic_hip.h")).read()
    assert int(re.search(r"#define\s+MCQ_ABI_VERSION\s+(\d+)", header).group(1)) == _lib.ABI_VERSION
    assert "mcq_step_meter_update_f32" in _lib.SYMBOLS and "mcq_step_meter_update_f32" in header


def test_step_meter_has_no_cpu_path():
    from mcquic_amd import Compressor, monitor
    with pytest.raises(RuntimeError, match="HIP device"):
        monitor.StepMeter(Compressor(8, 2, [32, 16, 8]), capacity=4, pixels=64)


def test_workspace_query_rejects_bad_tables():
    import ctypes
    from mcquic_amd import _lib
    lib = _lib.load()
    arr = lambda *v: (ctypes.c_int32 * len(v))(*v)
    assert lib.mcq_step_meter_workspace_bytes(arr(2, 3), arr(8, 5), 2) == 5 * 24
    assert lib.mcq_step_meter_workspace_bytes(arr(2, 0), arr(8, 5), 2) == 0
    assert lib.mcq_step_meter_workspace_bytes(arr(2), arr(8), 0) == 0
    assert lib.mcq_step_meter_workspace_bytes(None, None, 1) == 0
    assert lib.mcq_step_meter_columns(3) == 20 and lib.mcq_step_meter_columns(0) == 0 and lib.mcq_step_meter_columns(33) == 0
    assert lib.mcq_step_meter_update_f32(None, None, None, 0, *([None] * 5), 0.0, None, 1.0, 0.99, 0.1, 1.0, None, None, None, 4, None) == _lib.MCQ_EINVAL
