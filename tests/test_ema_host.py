"""mcquic_amd.optim.EMA without a GPU: argument checks of the entry points (csrc/ema.hip: they return before any device call),
constructor validation, what is averaged, and that nothing runs on the CPU."""
import ctypes

import pytest
import torch


def test_entry_points_reject_bad_arguments_without_a_device():
    from mcquic_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64)()
    ok = ctypes.addressof(buf)                               # (never dereferenced: the argument check returns first)

    def update(tables=ok, ntensors=1, numel=ok, blk_t=ok, blk_f=ok, nblocks=1, count=ok, decay=0.9, scalars=ok):
        return lib.mcq_ema_update_f32(tables, ntensors, numel, blk_t, blk_f, nblocks, count, None, decay, 1, scalars, None)

    def swap(tables=ok, ntensors=1, numel=ok, blk_t=ok, blk_f=ok, nblocks=1):
        return lib.mcq_ema_swap_f32(tables, ntensors, numel, blk_t, blk_f, nblocks, None)
    for fn in (update, swap):
        for kw in (dict(tables=None), dict(numel=None), dict(blk_t=None), dict(blk_f=None), dict(ntensors=0), dict(ntensors=-3), dict(nblocks=0),
                   dict(nblocks=-1)):
            assert fn(**kw) == _lib.MCQ_EINVAL, (fn.__name__, kw)
    assert update(count=None) == _lib.MCQ_EINVAL
    assert update(scalars=None) == _lib.MCQ_EINVAL
    for decay in (-1e-9, 1.0 + 1e-9, 2.0, float("nan"), float("inf"), -float("inf")):
        assert update(decay=decay) == _lib.MCQ_EINVAL, decay


def _net():
    net = torch.nn.Module()
    net.a = torch.nn.Parameter(torch.arange(6.0).reshape(2, 3))
    net.frozen = torch.nn.Parameter(torch.ones(4), requires_grad=False)
    net.b = torch.nn.Parameter(torch.full((5,), -2.0))
    net.register_buffer("counts", torch.arange(3))
    return net


def test_constructor_validation_and_what_is_averaged():
    from mcquic_amd import optim
    assert "EMA" in optim.__all__ and "EMA" not in optim.REGISTRY
    for decay in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            optim.EMA(_net(), decay=decay)
    with pytest.raises(ValueError):
        optim.EMA(_net(), decay=torch.zeros(2))
    with pytest.raises(ValueError):
        optim.EMA([])
    with pytest.raises(RuntimeError):
        optim.EMA([torch.nn.Parameter(torch.zeros(3, dtype=torch.float64))])
    net = _net()
    ema = optim.EMA(net, decay=0.5, warmup=False)
    assert ema.names == ["a", "b"] and not ema.swapped
    assert all(torch.equal(v, p.detach()) and v.data_ptr() != p.data_ptr() for v, p in zip(ema.averages, ema.params))
    base = ema._flat.data_ptr()
    assert [v.data_ptr() - base for v in ema.averages] == [0, 32], "views of one flat buffer, 16-byte aligned slices"
    sd = ema.averaged_state_dict()
    assert list(sd) == list(net.state_dict())
    assert sd["frozen"].data_ptr() == net.frozen.data_ptr() and sd["counts"].data_ptr() == net.counts.data_ptr()
    assert sd["a"].data_ptr() == ema.averages[0].data_ptr()
    # an iterable of parameters: exactly those, no model to fill
    it = optim.EMA([net.frozen, net.b])
    assert it.names == ["0", "1"] and len(it.averages) == 2
    with pytest.raises(RuntimeError):
        it.averaged_state_dict()


def test_nothing_runs_on_the_cpu():
    from mcquic_amd import optim
    ema = optim.EMA(_net())
    for call in (ema.update, ema.swap, ema.prepare):
        with pytest.raises(RuntimeError):
            call()
    with pytest.raises(RuntimeError):
        with ema.applied():
            pass
    assert not ema.swapped


def test_state_dict_round_trips_on_the_host():
    from mcquic_amd import optim
    a, b = optim.EMA(_net(), decay=0.75, warmup=False), optim.EMA(_net(), decay=0.5, warmup=True)
    with torch.no_grad():
        a.averages[1].mul_(3.0)
    a._count.fill_(7)
    sd = a.state_dict()
    assert sorted(sd) == ["averages", "decay", "num_updates", "warmup"] and sd["num_updates"] == 7
    b.load_state_dict(sd)
    assert (b.decay, b.warmup, b.num_updates) == (0.75, False, 7)
    assert all(torch.equal(x, y) for x, y in zip(a.averages, b.averages))
    with pytest.raises(KeyError):
        optim.EMA([torch.nn.Parameter(torch.zeros(3))]).load_state_dict(sd)
