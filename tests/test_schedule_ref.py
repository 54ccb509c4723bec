"""CPU: tests/_schedule_ref.py -- the float64 restatement the schedule tests reason with -- against the REAL reference's schedulers as
recorded in tests/golden/f19_lr_schedules.npz (tests/golden/make_golden_schedules.py: mcquic/train/lrSchedulers.py imported unmodified).
Both sides are CPython float64 running the same operations in the same order on the same libm: the comparison is exact."""
import numpy as np
import pytest

import _schedule_ref as R

CASES, RATES, EPOCHS = R.load()


def test_fixture_holds_the_cases_the_schedules_are_pinned_on():
    names = [c["name"] for c in CASES]
    assert len(set(names)) == len(names)
    kinds = {c["scheduler"] for c in CASES}
    assert kinds == {"Placeholder", "MultiStepLRWithWarmUp", "CyclicLR", "CosineAnnealingWarmupRestarts"}
    assert {c["kwargs"]["mode"] for c in CASES if c["scheduler"] == "CyclicLR"} == {"triangular", "triangular2", "exp_range"}
    assert sorted(c["last_epoch"] for c in CASES if c["name"].startswith("cosine_resume")) == [0, 5, 9, 30]
    assert any(len(c["base_lrs"]) == 2 for c in CASES)
    for c in CASES:
        assert c["steps"] <= 64 and RATES[c["name"]].shape == (c["steps"] + 1, len(c["base_lrs"])) and RATES[c["name"]].dtype == np.float64
    # what the cases are there for: two restarts with a growing cycle; the zero floor, past the restart; the overshoot at the first
    # milestone and the milestone that never decays; a duplicated milestone that decays once
    r = RATES["cosine_restarts"][:, 0]
    assert np.allclose(r[[2, 6, 8, 14, 16]], [0.1, 0.005, 0.05, 0.0025, 0.025], rtol=1e-12, atol=0), r[:18]
    a = RATES["cosine_a800"][:, 0]
    assert a[0] == 0.0 and a[4] == 1e-4 and a[20] == 0.0 and a[24] == 1e-4 and 0 < a[19] < 1e-6
    m = RATES["multistep"][:, 0]
    assert m[3] == 0.05 * 4.0 / 3 and m[4] == m[3] and m[5] == m[3] * 0.1 and m[8] == m[5] * 0.1
    d = RATES["multistep_duplicate"][:, 0]
    assert d[4] == d[3] * 0.5 and d[7] == d[4] * 0.5


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_equals_the_reference_exactly(case):
    rates, epochs = R.sequence(case)
    assert epochs.tolist() == EPOCHS[case["name"]].tolist()
    assert rates.tobytes() == RATES[case["name"]].tobytes(), np.abs(rates - RATES[case["name"]]).max()


def test_resume_is_not_the_sequential_value_when_the_cycle_grows():
    """`last_epoch=k` is the reference's closed form; with cycle_mult != 1 it leaves a fractional cycle length behind (6 * 1.5 ** 3 = 20.25
    where the recurrence is in a cycle of 15 steps) and the sequences part -- which is why the resume constructors have cases of their own."""
    seq = RATES["cosine_restarts"][:, 0]
    res = RATES["cosine_resume_30"][:, 0]
    assert EPOCHS["cosine_resume_30"][0] == 31
    assert not np.array_equal(res[:9], seq[30:39])
    early = RATES["cosine_resume_5"][:, 0]                    # (inside the first cycle both agree)
    assert np.array_equal(early[:1], seq[5:6])
