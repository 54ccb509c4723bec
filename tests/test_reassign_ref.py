"""CPU: the numpy restatement of the reassignment rule (tests/_reassign_ref.py) against the eager torch method
`_multiCodebookQuantization.reAssignCodebook`, element for element -- on random cases in every group regime and on the inputs of the
reference fixture tests/test_reassign.py loads (oracle `reassign_case` + `reassign_priority`).  The kernels of csrc/vq_reassign.hip are
then held to two yardsticks that are pinned to each other and are neither of them the kernel (tests/test_gpu_reassign_leaf.py)."""
import os

import numpy as np
import pytest
import torch

import _reassign_ref as RR
from oracle import mcquic_ref as R

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def torch_reassign(codebook, raw_freq, priority):
    """The eager method on CPU, fed the normalised frequencies of the restatement's own row sum (the method takes them normalised)."""
    from mcquic_amd.modules import quantizer as MQ
    cb = torch.from_numpy(np.asarray(codebook, dtype=np.float32)).clone()
    q = MQ._multiCodebookQuantization(torch.nn.Parameter(cb), MQ._CodebookCache())
    changed = q.reAssignCodebook(torch.from_numpy(RR.normalised(raw_freq)), priority=torch.from_numpy(np.asarray(priority, dtype=np.float32)))
    return q._codebook.detach().numpy(), changed.view(cb.shape[0], cb.shape[1]).numpy()


def _assert_pinned(cb, raw, prio):
    new, source, changed = RR.reassign(cb, raw, prio)
    want, want_changed = torch_reassign(cb, raw, prio)
    np.testing.assert_array_equal(new, want)
    np.testing.assert_array_equal(changed, want_changed)
    m, k, _ = cb.shape
    assert source.dtype == np.int32 and source.min() >= 0 and source.max() < k
    return new, source, changed


@pytest.mark.parametrize("m,k,d,ties", [(1, 2, 1, False), (6, 5, 3, False), (6, 64, 16, False), (6, 64, 16, True), (12, 33, 4, True), (6, 512, 8, False)])
def test_restatement_equals_the_torch_method_in_every_regime(m, k, d, ties):
    regimes = RR.REGIMES[1:] if m == 1 else RR.REGIMES
    cb, raw, prio = RR.regime_case(m, k, d, seed=k + d + int(ties), regimes=regimes, ties=ties)
    new, source, changed = _assert_pinned(cb, raw, prio)
    dead = RR.normalised(raw) < 1e-6
    assert np.array_equal(new[~dead], cb[~dead])                      # live codewords never move
    assert (source[~dead] == np.nonzero(~dead)[1]).all()


def test_the_cases_cover_the_regimes():
    """The generator does put every regime the kernel test needs into one table: by count of dead codewords per group, with dead
    codewords at index 0 and k - 1, and with rows the read-before-write case shows on (a donor that is itself refilled)."""
    cb, raw, prio = RR.regime_case(6, 64, 16, seed=81)
    dead = RR.normalised(raw) < 1e-6
    assert dead.sum(-1).tolist() == [0, 1, 32, 33, 63, 64]
    assert dead[1, 0] and dead[2, 0] and dead[2, 63]
    assert float(raw[:5].astype(np.float64).sum(-1).max()) < 16 and np.all(raw[:5] * 2.0 ** 20 == np.round(raw[:5] * 2.0 ** 20))
    source, refill = RR.plan(raw, prio)
    chained = [bool((refill[g] & refill[g][source[g]] & (source[g] != np.arange(64))).any()) for g in range(6)]
    # 33 dead: 31 live donors for 32 refills, the last donor is a refilled row; all but one dead: 31 of them donate their OLD value
    assert chained == [False, False, False, True, True, False]
    assert (source[5] == np.arange(64)).all() and refill[5].sum() == 32      # all dead: every refilled row is its own donor
    new, _, changed = RR.reassign(cb, raw, prio)
    assert changed[4].sum() > 16 and not changed[5].any() and not changed[0].any()
    _, _, ptie = RR.regime_case(6, 64, 16, seed=81, ties=True)
    assert len(np.unique(ptie)) <= 3


@pytest.mark.parametrize("ci", range(len(R.REASSIGN_CASES)))
def test_restatement_equals_the_torch_method_on_the_reference_fixture(ci):
    """The fixture's inputs through its own helper; where re-normalising the (already normalised) frequencies keeps their order, the
    restatement also reproduces the reference's recorded output on every slot the reference defines."""
    z = np.load(os.path.join(G, "f9_reassign.npz"))
    m, k, d, dead_frac, seed = R.REASSIGN_CASES[ci]
    cb, freq, perms = R.reassign_case(m, k, d, dead_frac, seed)
    prio = R.reassign_priority(freq, perms)
    new, _, changed = _assert_pinned(cb.numpy(), freq.numpy(), prio.numpy())
    defined = R.reassign_defined_mask(freq, prio).numpy()
    np.testing.assert_array_equal(new[defined], z[f"new_codebook_{ci}"][defined])
    np.testing.assert_array_equal(changed[defined], z[f"changed_{ci}"].reshape(m, k)[defined])
