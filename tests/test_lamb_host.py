"""mcquic_amd.optim.Lamb without a GPU: constructor validation, the optimizer registry, argument checks of the entry points
(csrc/lamb.hip: they return before any launch), the workspace query and a fresh checkpoint's round trip."""
import ctypes

import pytest
import torch


def _p():
    return [torch.nn.Parameter(torch.zeros(4))]


def test_constructor_validation():
    from mcquic_amd import optim
    with pytest.raises(RuntimeError):
        optim.Lamb(_p(), amsgrad=True)
    for kw in (dict(lr=-1e-3), dict(eps=-1e-6), dict(weight_decay=-0.01), dict(betas=(1.0, 0.999)), dict(betas=(0.9, 1.0)),
               dict(betas=(-0.1, 0.999)), dict(betas=(0.9, -0.5))):
        with pytest.raises(ValueError):
            optim.Lamb(_p(), **kw)
    opt = optim.Lamb(_p())
    g = opt.param_groups[0]
    assert (g["lr"], g["betas"], g["eps"], g["weight_decay"], g["max_grad_norm"]) == (1e-3, (0.9, 0.999), 1e-6, 0.01, 1.0)
    assert g["bias_correction"] and g["adam_w_mode"] and g["grad_averaging"] and not g["use_nvlamb"]
    assert optim.FusedLAMB is optim.Lamb


def test_set_grad_none_is_the_default_of_zero_grad():
    from mcquic_amd import optim
    for flag in (True, False):
        p = _p()
        p[0].grad = torch.ones(4)
        optim.Lamb(p, set_grad_none=flag).zero_grad()
        assert (p[0].grad is None) == flag
        if not flag:
            assert float(p[0].grad.abs().sum()) == 0.0


def test_cpu_tensors_raise():
    from mcquic_amd import optim
    p = _p()
    p[0].grad = torch.ones(4)
    opt = optim.Lamb(p)
    with pytest.raises(RuntimeError):
        opt.step()
    with pytest.raises(RuntimeError):
        opt.prepare()
    with pytest.raises(NotImplementedError):
        opt.step(lambda: 0.0)


def test_registry_resolves_the_reference_keys():
    from mcquic_amd import optim
    assert optim.REGISTRY == {"FusedLAMB": optim.Lamb, "Adam": optim.AdamW, "SGD": torch.optim.SGD}


def test_entry_points_reject_null_tables_and_empty_lists():
    from mcquic_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    ok = ctypes.addressof(buf)                               # (never dereferenced: the argument check returns first)
    assert lib.mcq_lamb_grad_partials_f32(None, 1, ok, ok, ok, 1, ok, None) == _lib.MCQ_EINVAL
    assert lib.mcq_lamb_grad_partials_f32(ok, 0, ok, ok, ok, 1, ok, None) == _lib.MCQ_EINVAL
    assert lib.mcq_lamb_grad_partials_f32(ok, 1, ok, ok, ok, 1, None, None) == _lib.MCQ_EINVAL

    def step(tables=ok, ntensors=1, first=ok, nblocks=1, beta1=0.9, mgn=1.0):
        return lib.mcq_lamb_step_f32(tables, ntensors, ok, ok, ok, first, nblocks, ok, 1, ok, None, 1e-3, beta1, 0.999, 1e-6, 0.01, 1, 1, 1, 0, mgn,
                                     ok, ok, ok, ok, None)
    assert step(tables=None) == _lib.MCQ_EINVAL
    assert step(first=None) == _lib.MCQ_EINVAL
    assert step(ntensors=0) == _lib.MCQ_EINVAL
    assert step(ntensors=-3) == _lib.MCQ_EINVAL
    assert step(nblocks=0) == _lib.MCQ_EINVAL
    assert step(beta1=1.0) == _lib.MCQ_EINVAL
    assert step(mgn=-1.0) == _lib.MCQ_EINVAL


def test_workspace_query_runs_without_a_gpu():
    from mcquic_amd import _lib
    lib = _lib.load()
    assert lib.mcq_lamb_workspace_bytes(10, 300) >= 300 * 2 * 8 + 10 * 4
    assert lib.mcq_lamb_workspace_bytes(0, 300) == 0
    assert lib.mcq_lamb_workspace_bytes(10, 0) == 0
    assert lib.mcq_lamb_workspace_bytes(-1, -1) == 0


def test_fresh_state_dict_round_trips():
    from mcquic_amd import optim
    a = optim.Lamb(_p(), lr=3e-3, weight_decay=0.0, use_nvlamb=True, adam_w_mode=False)
    sd = a.state_dict()
    assert sd["state"] == {}
    b = optim.Lamb(_p())
    b.load_state_dict(sd)
    ga, gb = a.param_groups[0], b.param_groups[0]
    assert {k: v for k, v in ga.items() if k != "params"} == {k: v for k, v in gb.items() if k != "params"}
    assert b.state_dict() == sd
