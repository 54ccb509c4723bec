"""tests/_ema_ref.py (the float64 restatement the GPU tests of mcquic_amd.optim.EMA compare with) pinned to
torch.optim.swa_utils.AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(decay)) on float64 CPU parameters, and its warm-up schedule to
the fractions it is defined by.  No GPU."""
from fractions import Fraction

import pytest
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

from _ema_ref import RefEMA, decay_at


class _Net(torch.nn.Module):
    def __init__(self, seed):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(torch.randn(s, generator=g, dtype=torch.float64)) for s in [(1,), (5,), (7, 3), (2, 3, 3, 3)]])


@pytest.mark.parametrize("decay", [0.0, 0.5, 0.9, 0.9999])
def test_restatement_equals_averaged_model_over_five_updates(decay):
    """Both sides are float64; torch's lerp takes the form p - (p - avg) d once 1 - d >= 0.5, the restatement always avg + (1 - d)(p - avg):
    they agree to a few float64 roundings of max|x| per update -- 1e-14 relative over five."""
    net = _Net(3)
    theirs = AveragedModel(net, multi_avg_fn=get_ema_multi_avg_fn(decay))
    theirs.update_parameters(net)                             # (AveragedModel's first call COPIES the parameters: the initialisation)
    ref = RefEMA(list(net.parameters()), decay)
    g = torch.Generator().manual_seed(4)
    for _ in range(5):
        with torch.no_grad():
            for p in net.parameters():
                p.add_(torch.randn(p.shape, generator=g, dtype=torch.float64) * 0.3)
        theirs.update_parameters(net)
        ref.update(list(net.parameters()))
    assert ref.num_updates == 5 and ref.decays == [decay] * 5
    moved = False
    for a, t, p in zip(ref.averages, theirs.module.parameters(), net.parameters()):
        assert float((a - t.detach()).abs().max()) <= 1e-14 * float(t.detach().abs().max())
        moved = moved or not torch.equal(a, p.detach())
    assert moved or decay == 0.0, "an average that equals the parameters pins nothing"


def test_warmup_decays_are_the_fractions_until_decay_caps_them():
    for decay in (0.5, 0.9, 0.9999):
        ref = RefEMA([torch.zeros(3, dtype=torch.float64)], decay, warmup=True)
        for _ in range(120):
            ref.update([torch.ones(3, dtype=torch.float64)])
        assert ref.decays[:3] == [1 / 10, 2 / 11, 3 / 12]
        capped = False
        for n, d in enumerate(ref.decays):
            frac = Fraction(1 + n, 10 + n)
            if frac < Fraction(decay):
                assert not capped and d == (1.0 + n) / (10.0 + n) == float(frac), n     # (one correctly rounded division: the fraction's double)
            else:
                capped = True
                assert d == decay, n
        assert capped == (decay < 0.9999), "0.5 caps at n = 8, 0.9 at n = 80, 0.9999 not within 120 updates"
    assert decay_at(0.9, 7, False) == 0.9
    # with warm-up the first update moves the average 9/10 of the way
    ref = RefEMA([torch.zeros(1, dtype=torch.float64)], 0.9999, warmup=True)
    ref.update([torch.ones(1, dtype=torch.float64)])
    assert abs(float(ref.averages[0]) - 0.9) <= 1e-15
