"""mcquic_amd.schedule on the device, kernel by kernel: every case of tests/golden/f19_lr_schedules.npz (the REAL reference's sequences,
tests/golden/make_golden_schedules.py) stepped by `mcq_lr_schedule_step`, one launch per step.

  float32 store          the `lr` tensor is float32 of the device's own float64 rate, bit for bit, at every step
  arithmetic-only        Placeholder, MultiStep, every warm-up ramp, Cyclic triangular: the float64 rate is the fixture's, exactly
  cos / pow branches     |device - fixture| <= 2^-50 * (the case's largest rate).  Derived, not tuned: the device's cos / pow and the host's
                         are each within about an ulp (2^-53 relative) of a value of magnitude <= 1 -- (1 + cos) / 2, gamma ** n with
                         gamma <= 1 --, and a few roundings of that size follow (the sum, the product with the amplitude, the halving, the
                         sum with min_lr): about 2^-52 of the amplitude in all, and 2^-50 is four times that.  The bound is absolute
                         against the peak rate, not in ulps of the result: 1 + cos cancels near a cycle's end, and with lrScaleRatio 0 the
                         last steps of a cycle are tiny numbers.  Worst observed on an MI355X: 0 -- every recorded point
                         came out with the fixture's bits (docs/experiments.md section 21).
  resume constructors    the `cosine_resume_*` cases, under the same bars
  round trip, warm()     state_dict -> load_state_dict into a fresh scheduler continues bit for bit; warm() leaves every bit as it was
"""
import numpy as np
import pytest
import torch

import _schedule_ref as R

pytestmark = pytest.mark.gpu
CASES, RATES, EPOCHS = R.load()
BOUND = 2.0 ** -50


def _record(sched, steps):
    """(last_epoch [steps + 1], float64 state [steps + 1, groups, 8], float32 rates [steps + 1, groups]) with one copy at the end."""
    bufs, lrs = [sched._buf.clone()], [torch.stack([lr.reshape(()) for lr in sched._lrs])]
    for _ in range(steps):
        sched.step()
        bufs.append(sched._buf.clone())
        lrs.append(torch.stack([lr.reshape(()) for lr in sched._lrs]))
    host = torch.stack(bufs).cpu().numpy()
    return host[:, 0].copy(), host[:, 1:].copy().view(np.float64).reshape(steps + 1, len(sched._lrs), 8), torch.stack(lrs).cpu().numpy()


@pytest.fixture(scope="module")
def runs(dev):
    out = {}
    for case in CASES:
        opt, sched = R.make_scheduler(case, dev)
        out[case["name"]] = _record(sched, case["steps"]) + (opt, sched)
    return out


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_device_sequence_against_the_reference(runs, case):
    epochs, state, lr32, opt, sched = runs[case["name"]]
    want = RATES[case["name"]]
    rate = state[:, :, 0]
    assert epochs.tolist() == EPOCHS[case["name"]].tolist()
    assert sched.last_epoch == EPOCHS[case["name"]][-1] and sched.get_last_lr() == rate[-1].tolist()
    assert all(g["lr"] is lr for g, lr in zip(opt.param_groups, sched._lrs))
    assert lr32.dtype == np.float32 and lr32.tobytes() == rate.astype(np.float32).tobytes(), "the float32 store is not the rounding of the float64 rate"
    exact = R.exact_points(case)
    worst = float(np.abs(rate - want).max()) / float(np.abs(want).max())
    print(f"{case['name']}: worst |device - fixture| / peak = {worst:.3e} = 2^{np.log2(worst) if worst else -np.inf:.1f}; "
          f"points that differ {int((rate != want).sum())} of {rate.size}, exact points {int(exact.sum())}")
    bad = np.argwhere(exact & (rate != want))
    assert not len(bad), (bad[:4].tolist(), rate[tuple(bad[0])], want[tuple(bad[0])])
    assert worst <= BOUND, worst


def test_state_round_trip_continues_bit_for_bit(dev):
    case = next(c for c in CASES if c["name"] == "cosine_two_groups")
    _, a = R.make_scheduler(case, dev)
    for _ in range(9):                                        # (into the second cycle: bounds, cycle length and counters have all moved)
        a.step()
    sd = a.state_dict()
    assert sd["last_epoch"] == 9 and sd["state"][0, 1] == 1.0 and sd["state"][0, 3] == 8.0
    opt_b, b = R.make_scheduler(case, dev)
    b.step()
    addresses = (b._buf.data_ptr(), [lr.data_ptr() for lr in b._lrs])
    b.load_state_dict(sd)
    assert addresses == (b._buf.data_ptr(), [lr.data_ptr() for lr in b._lrs]), "loaded INTO the buffers a captured step may hold"
    assert torch.equal(a._buf, b._buf) and all(torch.equal(x, y) for x, y in zip(a._lrs, b._lrs))
    ra, rb = _record(a, 25), _record(b, 25)
    for x, y in zip(ra, rb):
        assert x.tobytes() == y.tobytes()
    want = RATES[case["name"]]
    assert np.abs(rb[1][:, :, 0] - want[9:35]).max() <= BOUND * np.abs(want).max()


@pytest.mark.parametrize("name", ["cosine_restarts", "multistep", "cyclic_exp_range"])
def test_warm_leaves_every_bit_as_it_was(dev, name):
    case = next(c for c in CASES if c["name"] == name)
    _, s = R.make_scheduler(case, dev)
    for _ in range(4):
        s.step()
    buf, lrs = s._buf.clone(), [lr.clone() for lr in s._lrs]
    s.warm()
    assert torch.equal(s._buf, buf) and all(torch.equal(x, y) for x, y in zip(s._lrs, lrs))
    assert s.last_epoch == 4
    s.step()
    assert not torch.equal(s._buf, buf)


def test_step_under_capture_replays_the_sequence(dev):
    """`step()` reads nothing on the host: one captured launch, replayed, walks the schedule; an adopted rate tensor keeps its address."""
    from mcquic_amd import optim, schedule
    lr = torch.tensor(0.1, dtype=torch.float32, device=dev)
    opt = optim.SGD([torch.nn.Parameter(torch.zeros(4, device=dev))], lr=lr)
    s = schedule.MultiStepLRWithWarmUp(opt, [3, 5, 8], gamma=0.1)
    assert opt.param_groups[0]["lr"] is lr
    eager_opt, eager = R.make_scheduler(dict(scheduler="MultiStepLRWithWarmUp", kwargs=dict(milestones=[3, 5, 8], gamma=0.1),
                                             base_lrs=[float(np.float32(0.1))], last_epoch=-1), dev)
    s.warm()
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        s.step()
    assert s.last_epoch == 0, "capturing is not stepping"
    for i in range(10):
        graph.replay()
        eager.step()
        assert torch.equal(s._buf, eager._buf) and torch.equal(lr.reshape(()), eager._lrs[0].reshape(())), i
    assert s.last_epoch == 10
