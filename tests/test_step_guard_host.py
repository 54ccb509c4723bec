"""CPU: the step guard's float64 reference against hand-computed cases; the new entry points' binding, ABI number and argument checks
(every refusal below returns before anything is launched); the refusals of contradictory settings that need no device."""
import math
import os
import re

import numpy as np
import pytest
import torch

import _guard_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mcq_step_guard_chunks", "mcq_step_guard_list_f32", "mcq_step_guard_flat_f32", "mcq_step_guard_partials_f32", "mcq_step_guard_norm_f32",
       "mcq_clip_by_norm_skip_f32", "mcq_adam_step_skip_f32", "mcq_lamb_grad_partials_skip_f32", "mcq_lamb_step_skip_f32", "mcq_sgd_step_skip_f32",
       "mcq_ema_update_skip_f32", "mcq_freq_ema_update_skip_f32", "mcq_lr_schedule_step_skip"]


def test_reference_flag_norm_and_counters():
    assert R.norm([np.array([3.0]), np.array([[4.0]])]) == 5.0
    assert R.norm([np.full(7, 1e19, np.float32)]) == pytest.approx(1e19 * math.sqrt(7), rel=1e-7)      # no overflow of the squares
    for bad in (np.nan, np.inf, -np.inf):
        assert not math.isfinite(R.norm([np.ones(5), np.array([1.0, bad])]))
    clean, nan = [np.ones(4)], [np.array([np.nan])]
    recs = R.run([clean, nan, nan, clean, nan])
    assert [r["skip"] for r in recs] == [0, 1, 1, 0, 1]
    assert [r["skipped"] for r in recs] == [0, 1, 2, 2, 3]
    assert [r["consecutive"] for r in recs] == [0, 1, 2, 0, 1]
    assert recs[0]["grad_norm"] == np.float32(2.0) and np.isnan(recs[1]["grad_norm"])


def test_binding_and_abi_version():
    from mcquic_amd import _lib
    header = open(os.path.join(ROOT, "include", "mcquic_hip.h")).read()
    declared = int(re.search(r"#define\s+MCQ_ABI_VERSION\s+(\d+)", header).group(1))
    lib = _lib.load()
    assert lib.mcq_abi_version() == declared == _lib.ABI_VERSION >= 18
    for name in NEW:
        assert name in _lib.SYMBOLS and re.search(r"\b%s\s*\(" % name, header) and getattr(lib, name) is not None
    chunk = lib.mcq_adam_chunk()
    assert chunk == int(re.search(r"MCQ_LIST_CHUNK\s*=\s*(\d+)", open(os.path.join(ROOT, "mcquic_amd", "csrc", "tensor_list.h")).read()).group(1))
    assert [lib.mcq_step_guard_chunks(n) for n in (-1, 0, 1, chunk, chunk + 1, 2 * chunk + 1)] == [0, 0, 1, 1, 2, 3]


def test_entry_points_refuse_missing_arguments():
    """MCQ_EINVAL for what a caller can get wrong with the guard's own entry points (no launch happens: every pointer below is either
    NULL or never dereferenced before the check)."""
    from mcquic_amd import _lib
    lib = _lib.load()
    buf = torch.zeros(8, dtype=torch.float64)
    p = buf.data_ptr()
    E = _lib.MCQ_EINVAL
    assert lib.mcq_step_guard_flat_f32(None, 4, p, p, None) == E
    assert lib.mcq_step_guard_flat_f32(p, 0, p, p, None) == E
    assert lib.mcq_step_guard_flat_f32(p, 4, None, p, None) == E
    assert lib.mcq_step_guard_flat_f32(p, 4, p, None, None) == E
    assert lib.mcq_step_guard_partials_f32(None, 1, p, None) == E
    assert lib.mcq_step_guard_partials_f32(p, 0, p, None) == E
    assert lib.mcq_step_guard_partials_f32(p, 1, None, None) == E
    assert lib.mcq_step_guard_norm_f32(None, 0, p, None) == E
    assert lib.mcq_step_guard_norm_f32(p, 0, None, None) == E
    assert lib.mcq_step_guard_list_f32(None, 1, p, p, p, 1, p, p, 1, p, None) == E          # no tables
    assert lib.mcq_step_guard_list_f32(p, 1, p, p, p, 1, None, p, 1, p, None) == E          # no room for the partials
    assert lib.mcq_step_guard_list_f32(p, 1, p, p, p, 1, p, None, 0, p, None) == E          # a record, but nothing to sum
    assert lib.mcq_step_guard_flat_f32(p, (2 ** 31) * lib.mcq_adam_chunk() + 1, p, p, None) == _lib.MCQ_ETOOLARGE


def test_python_side_refusals():
    from mcquic_amd import guard, optim
    with pytest.raises(RuntimeError, match="HIP device only"):
        guard.StepGuard("cpu")
    for bad in (torch.zeros((), dtype=torch.int32), 1, torch.zeros(2)):
        with pytest.raises(TypeError, match="one int32 on the HIP device"):
            guard.skip_pointer(bad, "cuda:0", "test")
    assert guard.skip_pointer(None, "cuda:0", "test") is None
    params = [torch.nn.Parameter(torch.zeros(3))]
    for own in (optim.Adam(params, skip_nonfinite=True), optim.AdamW(params, skip_nonfinite=True), optim.Lamb(params, skip_nonfinite=True),
                optim.SGD(params, lr=0.1, skip_nonfinite=True)):
        with pytest.raises(ValueError, match="counted twice"):
            own.attach_guard(object())
        own.attach_guard(None)                                # (detaching is always fine)
    plain = optim.Adam(params)
    assert getattr(plain, "skipped", None) is None, "without the option nothing counts and the attribute is absent, as before"
    plain.attach_guard(None)
    with pytest.raises(RuntimeError, match="no CPU path"):
        from mcquic_amd.modules.entropyCoder import EntropyCoder
        EntropyCoder._emaUpdate(object(), [torch.zeros(1, 2)], skip=torch.zeros((), dtype=torch.int32))
