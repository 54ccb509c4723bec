"""mcquic_amd.optim.EMA (csrc/ema.hip: the whole model's average in one launch; live and averaged weights exchanged in place) against the
float64 restatement of tests/_ema_ref.py, started from the same float32 values.

The bar (`_bar` of tests/test_gpu_sgd.py): torch._foreach_lerp_ runs on the device on the same inputs -- what
torch.optim.swa_utils.get_ema_multi_avg_fn runs; its worst error against the restatement, relative to max|x| per tensor, is the measured
error of a float32 average.  Ours may be 4 x that far from the restatement, and never needs to be closer than one float32 ulp of max|x|.

The tensor set is that file's, with c = mcq_adam_chunk(): 1, 3, 4, 5, c - 1, c, c + 1, 2c + 5, [7, 3, 3, 3], a tensor without elements and
a parameter that is a view starting 4 bytes past a 16-byte boundary -- plus one parameter with requires_grad=False, which is left out."""
import pytest
import torch

from _ema_ref import RefEMA
from test_gpu_sgd import VIEW, _bar, _params, _shapes, _values

pytestmark = pytest.mark.gpu


def _model(dev, seed):
    net = torch.nn.Module()
    net.ps = torch.nn.ParameterList(_params(dev, seed))
    net.frozen = torch.nn.Parameter(torch.full((37,), 0.25, device=dev), requires_grad=False)
    assert net.ps[VIEW].data_ptr() % 16 == 4 and not net.ps[9].numel()
    return net


def _move(net, seed):
    """New values into the same addresses (a captured update reads them); returns them."""
    vals = _values(seed)
    with torch.no_grad():
        for p, v in zip(net.ps, vals):
            p.copy_(v)
    return vals


def _run(dev, decay, warmup, as_tensor, updates=5, seed=1):
    from mcquic_amd import optim
    net = _model(dev, seed)
    d = float(torch.tensor(decay, dtype=torch.float32)) if as_tensor else decay     # (a tensor decay IS a float32: all three sides take its value)
    ema = optim.EMA(net, decay=torch.tensor(decay, dtype=torch.float32, device=dev) if as_tensor else decay, warmup=warmup)
    theirs = [p.detach().clone() for p in net.ps]
    ref = RefEMA([p.detach() for p in net.ps], d, warmup)
    for it in range(updates):
        _move(net, 10 * seed + it + 1)
        ema.update()
        ref.update([p.detach() for p in net.ps])
        torch._foreach_lerp_(theirs, [p.detach() for p in net.ps], 1.0 - ref.decays[-1])
    return net, ema, theirs, ref


@pytest.mark.parametrize("as_tensor", [False, True], ids=["float", "tensor"])
@pytest.mark.parametrize("warmup", [False, True], ids=["plain", "warmup"])
@pytest.mark.parametrize("decay", [0.0, 0.9, 0.9999])
def test_ema_matches_the_restatement(dev, decay, warmup, as_tensor):
    net, ema, theirs, ref = _run(dev, decay, warmup, as_tensor)
    assert ema.names == [f"ps.{i}" for i in range(len(_shapes()))], "the frozen parameter is left out"
    assert torch.equal(net.frozen.detach(), torch.full((37,), 0.25, device=dev))
    assert ema.num_updates == ref.num_updates == 5
    if warmup and decay > 0.5:
        assert ref.decays == [1 / 10, 2 / 11, 3 / 12, 4 / 13, 5 / 14]
    _bar(f"ema[decay={decay},warmup={warmup},{'tensor' if as_tensor else 'float'}]", ema.averages, theirs, ref.averages)
    if decay == 0.0:
        for v, p in zip(ema.averages, net.ps):
            assert torch.equal(v.view(torch.int32), p.detach().view(torch.int32)), "decay 0: the average IS the parameter"
    else:
        assert not torch.equal(ema.averages[5], net.ps[5].detach())
    sd = ema.averaged_state_dict()
    assert torch.equal(sd["frozen"], net.frozen.detach()) and torch.equal(sd["ps.7"], ema.averages[7])


def test_ema_is_deterministic(dev):
    a = _run(dev, 0.9, True, False)[1]
    b = _run(dev, 0.9, True, False)[1]
    assert torch.equal(a._flat.view(torch.int32), b._flat.view(torch.int32)) and a.num_updates == b.num_updates == 5
    assert float(a._flat.abs().sum()) > 0.0


def test_ema_captured_update(dev):
    """Three replays of a captured `update()` (warm-up on, decay read from a device tensor) are the bits of three eager ones, and the
    device counter moves by three; an address that changed is refused under capture."""
    from mcquic_amd import optim
    nets = [_model(dev, 3), _model(dev, 3)]
    decay = torch.tensor(0.9, device=dev)
    emas = [optim.EMA(n, decay=decay, warmup=True) for n in nets]
    for e in emas:
        e.update()                                            # (the kernels' first launch, outside any capture)
    emas[0].prepare()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        emas[0].update()
    assert emas[0].num_updates == 1, "capturing runs nothing"
    for it in range(3):
        for n in nets:
            _move(n, 31 + it)
        if it == 2:
            decay.fill_(0.125)                                # (below the warm-up's 4/13: the tensor is read on every replay)
        graph.replay()
        emas[1].update()
        assert torch.equal(emas[0]._flat.view(torch.int32), emas[1]._flat.view(torch.int32)), it
    assert emas[0].num_updates == emas[1].num_updates == 4
    assert float(emas[0]._scalars[2]) == 0.125
    moved = torch.nn.Parameter(nets[0].ps[0].detach().clone())
    emas[0].params[0] = moved
    with pytest.raises(RuntimeError):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            emas[0].update()


def _bits(ts):
    return [t.detach().view(torch.int32).clone() for t in ts]


def test_ema_swap_exchanges_raw_words(dev):
    from mcquic_amd import optim
    net = _model(dev, 4)
    ema = optim.EMA(net, decay=0.9, warmup=False)
    _move(net, 41)
    ema.update()
    with torch.no_grad():
        net.ps[3][0], net.ps[3][1] = float("nan"), -0.0      # the dword path
        net.ps[7].view(-1)[4097], net.ps[7].view(-1)[-1] = -0.0, float("nan")      # a 16-byte lane of the second chunk; the tail
        net.ps[VIEW][5] = -0.0                                # the misaligned view
        ema.averages[5][17], ema.averages[5][18] = float("nan"), -0.0
    p0, a0 = _bits(net.ps), _bits(ema.averages)
    assert any(not torch.equal(x, y) for x, y in zip(p0, a0))
    assert int(p0[3][1]) == -2 ** 31 and int(p0[VIEW][5]) == -2 ** 31, "-0.0 is the sign bit alone"
    versions = [p._version for p in net.ps]
    frozen_version = net.frozen._version

    ema.swap()
    assert ema.swapped
    p1, a1 = _bits(net.ps), _bits(ema.averages)
    assert all(torch.equal(x, y) for x, y in zip(p1, a0)) and all(torch.equal(x, y) for x, y in zip(a1, p0)), "exchanged exactly"
    assert all(p._version > v for p, v in zip(net.ps, versions)) and net.frozen._version == frozen_version
    with pytest.raises(RuntimeError):
        ema.update()
    assert ema.num_updates == 1
    assert torch.equal(ema.averaged_state_dict()["ps.5"].view(torch.int32), a0[5]), "while swapped the averaged values are the model's"
    versions = [p._version for p in net.ps]

    ema.swap()
    assert not ema.swapped
    p2, a2 = _bits(net.ps), _bits(ema.averages)
    assert all(torch.equal(x, y) for x, y in zip(p2, p0)) and all(torch.equal(x, y) for x, y in zip(a2, a0)), "two swaps are the identity"
    assert all(p._version > v for p, v in zip(net.ps, versions))

    with ema.applied():
        assert ema.swapped and all(torch.equal(x, y) for x, y in zip(_bits(net.ps), a0))
    assert not ema.swapped and all(torch.equal(x, y) for x, y in zip(_bits(net.ps), p0))
    ema.update()
    assert ema.num_updates == 2
