"""mcquic_amd.schedule without a GPU.  The rule of csrc/schedule_rule.h compiled for the host, twice -- inside the library
(`mcq_lr_schedule_host`, what the constructors run) and as a stand-alone program (tests/schedule_host_main.cpp, no HIP) -- against the
reference's sequences (tests/golden/f19_lr_schedules.npz): exactly, because the host's libm is CPython's.  Then the argument checks of the
entry points, the registry, the refused optimizers and arguments, and the shape of a checkpoint."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import _schedule_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES, RATES, EPOCHS = R.load()
CPU = torch.device("cpu")


def _rule_and_state(sched):
    """(rule with HOST milestones, last_epoch, state [groups, 8] float64 copy, keep-alive) of a scheduler built on CPU parameters."""
    sd = sched.state_dict()
    miles = sched._milestones_host
    rule = sched._rule(len(sched._lrs), miles.ctypes.data if len(miles) else None)
    return rule, sd["last_epoch"], sd["state"].numpy().copy(), miles


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_library_host_rule_equals_the_reference_exactly(case):
    from mcquic_amd import _lib
    opt, sched = R.make_scheduler(case, CPU)
    want, epochs = RATES[case["name"]], EPOCHS[case["name"]]
    assert sched.last_epoch == epochs[0] and sched.get_last_lr() == want[0].tolist(), "the constructor's initial step"
    assert [float(g["lr"]) for g in opt.param_groups] == want[0].astype(np.float32).astype(np.float64).tolist()
    rule, epoch, state, _keep = _rule_and_state(sched)
    e = ctypes.c_int64(epoch)
    lr32 = np.zeros(len(case["base_lrs"]), dtype=np.float32)
    for i in range(1, case["steps"] + 1):
        assert _lib.load().mcq_lr_schedule_host(ctypes.byref(rule), 1, ctypes.addressof(e), state.ctypes.data, lr32.ctypes.data) == _lib.MCQ_OK
        assert e.value == epochs[i]
        assert state[:, 0].tobytes() == want[i].tobytes(), (i, state[:, 0], want[i])
        assert lr32.tobytes() == want[i].astype(np.float32).tobytes()


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """tests/schedule_host_main.cpp built with the host compiler: -ffp-contract=off as the library's build has it."""
    cxx = next((c for c in (shutil.which("g++"), shutil.which("c++"), shutil.which("clang++"), "/opt/rocm/lib/llvm/bin/clang++") if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("schedule") / "schedule_host_main")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tests", "schedule_host_main.cpp"), "-lm"], check=True)
    return exe


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_stand_alone_host_build_equals_the_reference_exactly(program, case):
    _, sched = R.make_scheduler(case, CPU)
    rule, epoch, state, miles = _rule_and_state(sched)
    args = [rule.kind, rule.mode, rule.ngroups] + [float(v).hex() for v in (rule.gamma, rule.first_milestone, rule.total_size, rule.step_ratio,
                                                                           rule.warmup_steps, rule.cycle_mult)]
    args += [epoch, case["steps"], len(miles)] + miles.tolist() + [float(v).hex() for v in state.reshape(-1)]
    out = subprocess.run([program] + [str(a) for a in args], check=True, capture_output=True, text=True).stdout.split("\n")
    want, epochs = RATES[case["name"]], EPOCHS[case["name"]]
    for i in range(1, case["steps"] + 1):
        words = out[i - 1].split()
        assert int(words[0]) == epochs[i]
        got = np.array([float.fromhex(w) for w in words[1::2]])
        got32 = np.array([float.fromhex(w) for w in words[2::2]])
        assert got.tobytes() == want[i].tobytes(), (i, got, want[i])
        assert got32.tobytes() == want[i].astype(np.float32).astype(np.float64).tobytes()


def test_entry_points_reject_bad_arguments_without_a_device():
    from mcquic_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_double * 64 * 8)()
    ok = ctypes.addressof(buf)                               # (never dereferenced by the device entry: the argument check returns first)

    def rule(**kw):
        r = _lib.LrSchedule()
        r.kind, r.mode, r.ngroups, r.nmilestones, r.milestones = _lib.LR_COSINE, 0, 1, 0, None
        r.gamma, r.first_milestone, r.total_size, r.step_ratio, r.warmup_steps, r.cycle_mult = 1.0, 0.0, 0.0, 0.0, 2.0, 1.0
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    def step(r, epoch=ok, state=ok, lr=ok):
        return lib.mcq_lr_schedule_step(ctypes.byref(r) if r is not None else None, epoch, state, lr, None)

    def host(r, advance=1, epoch=ok, state=ok):
        return lib.mcq_lr_schedule_host(ctypes.byref(r) if r is not None else None, advance, epoch, state, None)
    for fn in (step, host):
        assert fn(None) == _lib.MCQ_EINVAL
        assert fn(rule(), epoch=None) == _lib.MCQ_EINVAL and fn(rule(), state=None) == _lib.MCQ_EINVAL
        bad = [dict(ngroups=0), dict(ngroups=-1), dict(ngroups=_lib.LR_MAX_GROUPS + 1), dict(kind=4), dict(kind=-1), dict(warmup_steps=-1.0),
               dict(warmup_steps=1.5), dict(cycle_mult=0.0), dict(cycle_mult=float("nan")), dict(gamma=float("nan")),
               dict(kind=_lib.LR_MULTISTEP, first_milestone=3.0), dict(kind=_lib.LR_MULTISTEP, nmilestones=1, milestones=ok, first_milestone=0.0),
               dict(kind=_lib.LR_CYCLIC, total_size=0.0, step_ratio=0.5), dict(kind=_lib.LR_CYCLIC, total_size=5.0, step_ratio=0.0),
               dict(kind=_lib.LR_CYCLIC, total_size=5.0, step_ratio=1.5), dict(kind=_lib.LR_CYCLIC, total_size=5.0, step_ratio=0.5, mode=3)]
        for kw in bad:
            assert fn(rule(**kw)) == _lib.MCQ_EINVAL, (fn.__name__, kw)
    assert step(rule(), lr=None) == _lib.MCQ_EINVAL
    assert host(rule(ngroups=_lib.LR_MAX_GROUPS)) == _lib.MCQ_OK, "the cap itself is taken"
    # a recurrence on the rate has nothing to re-evaluate
    miles = (ctypes.c_int64 * 1)(3)
    assert host(rule(kind=_lib.LR_MULTISTEP, nmilestones=1, milestones=ctypes.addressof(miles), first_milestone=3.0), advance=0) == _lib.MCQ_EINVAL
    assert (_lib.LR_MAX_GROUPS, _lib.LR_STATE_WORDS) == (64, 8)
    header = open(os.path.join(ROOT, "include", "mcquic_hip.h")).read()
    assert "#define MCQ_LR_MAX_GROUPS   64" in header and "#define MCQ_LR_STATE_WORDS  8" in header


def _sgd(n=1, **kw):
    from mcquic_amd import optim
    return optim.SGD([{"params": [torch.nn.Parameter(torch.zeros(3))], "lr": 0.1 / (i + 1)} for i in range(n)], lr=1.0, **kw)


def test_registry_holds_the_references_keys():
    from mcquic_amd import schedule
    assert list(schedule.REGISTRY) == ["Placeholder", "MultiStepLRWithWarmUp", "CyclicLR", "CosineAnnealingWarmupRestarts"]
    assert all(cls.__name__ == key for key, cls in schedule.REGISTRY.items())
    assert sorted(schedule.__all__) == sorted(list(schedule.REGISTRY) + ["REGISTRY"])


def test_optimizers_that_read_a_tensor_rate_on_the_host_are_refused():
    from mcquic_amd import optim, schedule
    p = [torch.nn.Parameter(torch.zeros(3))]
    for make in (lambda: torch.optim.SGD(p, lr=0.1), lambda: torch.optim.Adam(p, lr=0.1), lambda: torch.optim.AdamW(p, lr=0.1),
                 lambda: torch.optim.RMSprop(p, lr=0.1)):
        opt = make()
        for build in (lambda o: schedule.Placeholder(o), lambda o: schedule.MultiStepLRWithWarmUp(o, [3]), lambda o: schedule.CyclicLR(o, 0.01, 0.1),
                      lambda o: schedule.CosineAnnealingWarmupRestarts(o, 6)):
            with pytest.raises(ValueError, match="on the host"):
                build(opt)
        assert not torch.is_tensor(opt.param_groups[0]["lr"]) and opt.param_groups[0]["lr"] == 0.1, "a refused optimizer is left as it was"
    with pytest.raises(TypeError):
        schedule.Placeholder(object())
    for make in (lambda: optim.Adam(p, lr=0.1), lambda: optim.AdamW(p, lr=0.1), lambda: optim.Lamb(p, lr=0.1), lambda: optim.SGD(p, lr=0.1),
                 lambda: torch.optim.Adam(p, lr=0.1, capturable=True), lambda: torch.optim.AdamW(p, lr=0.1, capturable=True)):
        opt = make()
        s = schedule.Placeholder(opt)
        lr = opt.param_groups[0]["lr"]
        assert torch.is_tensor(lr) and lr.dtype == torch.float32 and lr.dim() == 0 and float(lr) == float(np.float32(0.1))
        assert s.get_last_lr() == [0.1] and s.last_epoch == 0 and opt.param_groups[0]["initial_lr"] == 0.1


def test_argument_checks():
    from mcquic_amd import schedule
    with pytest.raises(ValueError, match="scale_fn"):
        schedule.CyclicLR(_sgd(), 0.01, 0.1, scale_fn=lambda x: 1.0)
    with pytest.raises(NotImplementedError, match="cycle_momentum"):
        schedule.CyclicLR(_sgd(), 0.01, 0.1, cycle_momentum=True)
    assert schedule.CyclicLR(_sgd(), 0.01, 0.1).get_last_lr() == [0.01], "cycle_momentum defaults to False here"
    with pytest.raises(ValueError):
        schedule.CyclicLR(_sgd(), 0.01, 0.1, mode="sawtooth")
    with pytest.raises(ValueError):
        schedule.CyclicLR(_sgd(2), [0.01], 0.1)
    with pytest.raises(ValueError):
        schedule.CyclicLR(_sgd(), 0.01, 0.1, step_size_up=0)
    for bad in ([], [0, 3], [-1]):
        with pytest.raises(ValueError):
            schedule.MultiStepLRWithWarmUp(_sgd(), bad)
    for kw in (dict(first_cycle_steps=4, warmup_steps=4), dict(first_cycle_steps=4, warmup_steps=-1), dict(first_cycle_steps=4, cycle_mult=0.0)):
        with pytest.raises(ValueError):
            schedule.CosineAnnealingWarmupRestarts(_sgd(), **kw)
    with pytest.raises(KeyError, match="initial_lr"):
        schedule.CosineAnnealingWarmupRestarts(_sgd(), 6, last_epoch=3)
    with pytest.raises(ValueError):
        schedule.Placeholder(_sgd(65))
    assert len(schedule.Placeholder(_sgd(64)).get_last_lr()) == 64


def test_an_existing_rate_tensor_is_adopted():
    from mcquic_amd import optim, schedule
    lr = torch.tensor(0.25, dtype=torch.float32)
    opt = optim.SGD([torch.nn.Parameter(torch.zeros(3))], lr=lr)
    s = schedule.CosineAnnealingWarmupRestarts(opt, 6, warmup_steps=2, lrScaleRatio=0.5)
    assert opt.param_groups[0]["lr"] is lr and float(lr) == 0.125 and s.get_last_lr() == [0.125]


def test_nothing_steps_on_the_cpu():
    from mcquic_amd import schedule
    s = schedule.MultiStepLRWithWarmUp(_sgd(), [3, 5])
    for call in (s.step, s.prepare, s.warm):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    assert s.last_epoch == 0


def test_state_dict_shape_and_round_trip_on_the_host():
    from mcquic_amd import schedule
    a = schedule.CosineAnnealingWarmupRestarts(_sgd(2), 6, cycle_mult=1.5, lrScaleRatio=0.1, warmup_steps=2, gamma=0.5, last_epoch=-1)
    sd = a.state_dict()
    assert sorted(sd) == ["last_epoch", "params", "scheduler", "state"] and sd["scheduler"] == "CosineAnnealingWarmupRestarts" and sd["last_epoch"] == 0
    assert sd["state"].dtype == torch.float64 and tuple(sd["state"].shape) == (2, 8) and sd["state"].device.type == "cpu"
    assert sd["params"] == {"first_cycle_steps": 6, "cycle_mult": 1.5, "lrScaleRatio": 0.1, "warmup_steps": 2, "gamma": 0.5}
    # rate, cycle, step_in_cycle, cur_cycle_steps, max_lr, min_lr, base_lr, min_base_lr
    assert sd["state"][1].tolist() == [0.05 * 0.1, 0.0, 0.0, 6.0, 0.05, 0.05 * 0.1, 0.05, 0.05 * 0.1]
    groups = [{"params": [torch.nn.Parameter(torch.zeros(3))], "lr": 0.1 / (i + 1), "initial_lr": 0.1 / (i + 1)} for i in range(2)]
    from mcquic_amd import optim
    opt = optim.SGD(groups, lr=1.0)
    b = schedule.CosineAnnealingWarmupRestarts(opt, 6, cycle_mult=1.5, lrScaleRatio=0.1, warmup_steps=2, gamma=0.5, last_epoch=30)
    assert b.last_epoch == 31 and b.state_dict()["state"][0, 3] == 6 * 1.5 ** 3, "the resume path's fractional cycle length: 20.25"
    b.load_state_dict(sd)
    assert b.last_epoch == 0 and torch.equal(b.state_dict()["state"], sd["state"])
    assert [float(g["lr"]) for g in opt.param_groups] == [float(np.float32(v)) for v in a.get_last_lr()]
    with pytest.raises(ValueError):
        schedule.CosineAnnealingWarmupRestarts(_sgd(2), 7, warmup_steps=2).load_state_dict(sd)
    with pytest.raises(ValueError):
        schedule.Placeholder(_sgd(2)).load_state_dict(sd)
    with pytest.raises(ValueError):
        schedule.CosineAnnealingWarmupRestarts(_sgd(1), 6, cycle_mult=1.5, lrScaleRatio=0.1, warmup_steps=2, gamma=0.5).load_state_dict(sd)
