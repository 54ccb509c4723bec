"""Learning-rate schedules that step on the device (mcquic/train/lrSchedulers.py, the reference's `LrSchedulerRegistry`; its trainer
steps the scheduler after every batch, mcquic/train/trainer.py `_stepFinish`, and trains with `CosineAnnealingWarmupRestarts`,
configs/a800_8.yaml): `Placeholder`, `MultiStepLRWithWarmUp`, `CyclicLR`, `CosineAnnealingWarmupRestarts`, with the reference's
names, constructor arguments and arithmetic, quirks included.

`step()` is ONE launch of one workgroup (`mcq_lr_schedule_step`, csrc/schedule.hip; the rule: csrc/schedule_rule.h), one lane per
parameter group: it advances `last_epoch` (int64) and eight float64 words of state per group ON THE DEVICE and stores float32(rate)
into each group's `lr`, which the constructor turns into a 0-dim float32 device tensor (an existing one is adopted) -- what the
optimizers' kernels read on every call.  The host reads nothing, so `parallel.GraphedTrainStep(..., scheduler=s)` records the launch in
its post graph once and every replay moves the schedule.  The float64 state is the truth, the float32 tensor only its rounding:
`get_last_lr()` returns the float64 rates.

The constructor performs the reference's initial step with the same rule compiled for the host (`mcq_lr_schedule_host`) and uploads
the result; `last_epoch=k` reproduces the reference's resume path -- for Cosine its closed form in `step(epoch)`, which with
`cycle_mult != 1` is not the value the sequential steps reach (the cycle length it leaves behind is a float, `first * mult ** n`).
HIP device only: on CPU parameters a scheduler can be built and inspected, `step()` raises."""
from __future__ import annotations

import ctypes
import math

import numpy as np
import torch

from . import _lib
from . import optim as _optim
from .ops import _guard, _stream, check

__all__ = ["Placeholder", "MultiStepLRWithWarmUp", "CyclicLR", "CosineAnnealingWarmupRestarts", "REGISTRY"]

_RATE, _CYCLE, _SIC, _CUR, _MAX, _MIN, _BASE, _MIN_BASE = range(8)
_W = _lib.LR_STATE_WORDS


def _check_optimizer(optimizer) -> None:
    """The optimizers whose update reads a tensor rate ON THE DEVICE at every call."""
    if not isinstance(optimizer, torch.optim.Optimizer):
        raise TypeError(f"{type(optimizer).__name__} is not an Optimizer")
    if isinstance(optimizer, _optim._Planned):                # mcquic_amd.optim.Adam / AdamW / Lamb / SGD
        return
    if isinstance(optimizer, (torch.optim.Adam, torch.optim.AdamW)) and all(g.get("capturable") for g in optimizer.param_groups):
        return
    raise ValueError(f"mcquic_amd.schedule: {type(optimizer).__module__}.{type(optimizer).__name__} would read a tensor learning rate on the host "
                     "(a captured update bakes it in): use mcquic_amd.optim.Adam / AdamW / Lamb / SGD, or torch.optim.Adam / AdamW(capturable=True)")


class _DeviceScheduler:
    """What the four schedulers share: the device state, the launch, and the host side of a checkpoint.

        step()                      the launch; safe under capture after `prepare()` (the constructor has prepared)
        get_last_lr()               the float64 rates as Python floats (one device-to-host copy)
        last_epoch                  read from the device (a host synchronisation)
        state_dict() / load_state_dict()   a reloaded scheduler continues the sequence bit for bit; the state is loaded INTO the
                                    buffers this object has (the addresses a captured step holds)
        prepare() / warm()          as `optim.EMA`'s: `warm()` is one throw-away launch after which every bit of state is restored
    """
    _KIND = _lib.LR_PLACEHOLDER
    _NAME = "Placeholder"

    # ---- construction ----------------------------------------------------------------------------------------------------------
    def _attach(self, optimizer, last_epoch: int) -> None:
        _check_optimizer(optimizer)
        groups = optimizer.param_groups
        if not 1 <= len(groups) <= _lib.LR_MAX_GROUPS:
            raise ValueError(f"mcquic_amd.schedule: {len(groups)} parameter groups; one launch steps 1..{_lib.LR_MAX_GROUPS} (MCQ_LR_MAX_GROUPS)")
        last_epoch = int(last_epoch)
        if last_epoch < -1:
            raise ValueError(f"Invalid last_epoch: {last_epoch}")
        self.optimizer = optimizer
        dev = next((p.device for g in groups for p in g["params"]), torch.device("cpu"))
        current = [float(g["lr"]) for g in groups]            # (a tensor rate is read once, here)
        if last_epoch == -1:
            for g, lr in zip(groups, current):
                g.setdefault("initial_lr", lr)
        else:
            for i, g in enumerate(groups):
                if "initial_lr" not in g:
                    raise KeyError(f"param 'initial_lr' is not specified in param_groups[{i}] when resuming an optimizer")
        self.base_lrs = [float(g["initial_lr"]) for g in groups]
        self._lrs = []
        for g in groups:                                      # every group's rate: one float32 on the device, an existing one adopted
            lr = g["lr"]
            if not (torch.is_tensor(lr) and lr.dtype == torch.float32 and lr.numel() == 1 and lr.device == dev):
                lr = g["lr"] = torch.zeros((), dtype=torch.float32, device=dev)
            self._lrs.append(lr)
        n = len(groups)
        state = np.zeros((n, _W), dtype=np.float64)
        state[:, _RATE], state[:, _BASE] = current, self.base_lrs
        self._milestones_host = np.asarray(sorted(set(getattr(self, "_distinct", ()))), dtype=np.int64)
        epoch, advance = self._initial_state(state, current, last_epoch)
        rule = self._rule(n, self._milestones_host.ctypes.data if len(self._milestones_host) else None)
        host_epoch = ctypes.c_int64(epoch)
        rates32 = np.zeros(n, dtype=np.float32)
        check(_lib.load().mcq_lr_schedule_host(ctypes.byref(rule), 1 if advance else 0, ctypes.addressof(host_epoch), state.ctypes.data,
                                               rates32.ctypes.data), "mcq_lr_schedule_host")
        self._after_initial_step(state)
        # ONE buffer: [last_epoch (int64)] [n x 8 float64]
        words = np.empty(1 + n * _W, dtype=np.int64)
        words[0] = host_epoch.value
        words[1:] = state.reshape(-1).view(np.int64)
        self._buf = torch.from_numpy(words).to(dev)
        self._state = self._buf[1:].view(torch.float64).view(n, _W)
        with torch.no_grad():
            for lr, v in zip(self._lrs, rates32):
                lr.fill_(float(v))
        self._tables = None
        if dev.type == "cuda":
            self.prepare()

    def _initial_state(self, state, current, last_epoch):
        """Fill `state` for the reference's constructor; returns (last_epoch to start from, whether the initial step advances)."""
        return last_epoch, True

    def _after_initial_step(self, state) -> None:
        pass

    def _params(self) -> dict:
        """The constructor arguments, as a checkpoint names them."""
        return {}

    def _rule(self, ngroups: int, milestones):
        r = _lib.LrSchedule()
        r.kind, r.mode, r.ngroups = self._KIND, 0, ngroups
        r.nmilestones, r.milestones = len(self._milestones_host), milestones
        r.gamma = r.first_milestone = r.total_size = r.step_ratio = r.warmup_steps = r.cycle_mult = 0.0
        self._fill_rule(r)
        return r

    def _fill_rule(self, r) -> None:
        pass

    # ---- the device side -------------------------------------------------------------------------------------------------------
    def _no_cpu(self) -> None:
        if not self._buf.is_cuda:
            raise RuntimeError(f"mcquic_amd.schedule.{self._NAME}: the parameters must live on a HIP device; the schedule's kernel has no CPU fallback")

    @torch.no_grad()
    def prepare(self) -> None:
        """The device tables (the groups' `lr` addresses, the milestones) and the groups' `lr` entries themselves: an optimizer's
        `load_state_dict` replaces them by the checkpoint's values, and the schedule's own tensors -- whose addresses a captured update
        holds, and whose values are the schedule's -- go back in.  Host-to-device copies: not inside a capture."""
        self._no_cpu()
        for g, lr in zip(self.optimizer.param_groups, self._lrs):
            if g["lr"] is not lr:
                g["lr"] = lr
        if self._tables is None:
            dev = self._buf.device
            ptrs = torch.tensor([lr.data_ptr() for lr in self._lrs], dtype=torch.int64).to(dev)
            miles = torch.from_numpy(self._milestones_host).to(dev) if len(self._milestones_host) else None
            self._tables = (ptrs, miles, self._rule(len(self._lrs), miles.data_ptr() if miles is not None else None))

    @torch.no_grad()
    def step(self, skip=None) -> None:
        """One `scheduler.step()` on the device: last_epoch += 1, every group's state advanced, float32(rate) stored into its `lr`.
        `skip`: a step's guard flag (one int32 on the device, `guard.StepGuard.skip`): when it is set on the device the schedule stays
        where it is -- last_epoch, state and rates."""
        self._no_cpu()
        if self._tables is None or any(g["lr"] is not lr for g, lr in zip(self.optimizer.param_groups, self._lrs)):
            self.prepare()
        ptrs, _, rule = self._tables
        from .guard import skip_pointer
        flag = skip_pointer(skip, self._buf.device, "mcquic_amd.schedule: step")
        with _guard(self._buf.device):
            check(_lib.load().mcq_lr_schedule_step_skip(ctypes.byref(rule), self._buf.data_ptr(), self._buf.data_ptr() + 8, ptrs.data_ptr(), flag,
                                                        _stream()), "mcq_lr_schedule_step_skip")

    @torch.no_grad()
    def warm(self) -> None:
        """One throw-away step, so that the kernel's first launch happens outside any capture; state and rates keep their bits."""
        keep, lrs = self._buf.clone(), [lr.clone() for lr in self._lrs]
        self.step()
        self._buf.copy_(keep)
        for lr, v in zip(self._lrs, lrs):
            lr.copy_(v)

    # ---- the host side ---------------------------------------------------------------------------------------------------------
    def _host_state(self):
        host = self._buf.cpu().numpy()
        return int(host[0]), host[1:].view(np.float64).reshape(len(self._lrs), _W)

    def get_last_lr(self) -> list:
        """The float64 rates of the last step, one per parameter group (one device-to-host copy)."""
        return [float(v) for v in self._host_state()[1][:, _RATE]]

    @property
    def last_epoch(self) -> int:
        return int(self._buf[0])

    def state_dict(self) -> dict:
        """{"scheduler", "params", "last_epoch", "state"}: `state` is the [groups, 8] float64 table of include/mcquic_hip.h, on the host."""
        epoch, state = self._host_state()
        return {"scheduler": self._NAME, "params": self._params(), "last_epoch": epoch, "state": torch.from_numpy(state.copy())}

    @torch.no_grad()
    def load_state_dict(self, sd) -> None:
        """Into the buffers this scheduler has.  The checkpoint must come from a scheduler built with the same arguments: the rule's
        constants travel with the launch (a captured one has them recorded), only the state is loaded."""
        if sd["scheduler"] != self._NAME:
            raise ValueError(f"mcquic_amd.schedule.{self._NAME}: the checkpoint is a {sd['scheduler']}'s")
        if sd["params"] != self._params():
            raise ValueError(f"mcquic_amd.schedule.{self._NAME}: the checkpoint was written with {sd['params']}, this scheduler was built with {self._params()}")
        state = torch.as_tensor(sd["state"])
        if state.dtype != torch.float64 or tuple(state.shape) != (len(self._lrs), _W):
            raise ValueError(f"mcquic_amd.schedule.{self._NAME}: `state` must be float64 [{len(self._lrs)}, {_W}] (got {state.dtype}, {tuple(state.shape)})")
        self._buf[0].fill_(int(sd["last_epoch"]))
        self._state.copy_(state.to(self._buf.device))
        for lr, v in zip(self._lrs, state[:, _RATE].to(torch.float32)):
            lr.fill_(float(v))


class Placeholder(_DeviceScheduler):
    """The base rates, for ever (lrSchedulers.py:14-19; further arguments are ignored, as there)."""

    def __init__(self, optimizer, *_, **__):
        self._attach(optimizer, -1)


class MultiStepLRWithWarmUp(_DeviceScheduler):
    """lrSchedulers.py:22-68.  Linear warm-up `base_lr * (last_epoch + 1) / first` while `last_epoch <= first`, first = min(milestones)
    -- which overshoots to (first + 1) / first at the first milestone, and the first milestone itself never decays --, then the rate is
    multiplied by `gamma` at every later milestone (a duplicated one decays once) and kept in between.  The recurrence runs on the float64
    rate the device holds, never on its float32 rounding."""
    _KIND, _NAME = _lib.LR_MULTISTEP, "MultiStepLRWithWarmUp"

    def __init__(self, optimizer, milestones, gamma=0.1, last_epoch=-1, verbose=False):
        self.milestones = [int(m) for m in milestones]
        if not self.milestones or min(self.milestones) < 1:
            raise ValueError(f"Invalid milestones: {milestones} (at least one, all >= 1: the warm-up divides by the first)")
        self.gamma = float(gamma)
        if self.gamma != self.gamma:
            raise ValueError("Invalid gamma: nan")
        self._distinct = self.milestones
        self._attach(optimizer, last_epoch)

    def _fill_rule(self, r) -> None:
        r.gamma, r.first_milestone = self.gamma, float(min(self.milestones))

    def _params(self) -> dict:
        return {"milestones": sorted(self.milestones), "gamma": self.gamma}


class CyclicLR(_DeviceScheduler):
    """lrSchedulers.py:72-302 (torch's CyclicLR): `base_lr`, `max_lr` (numbers, or one per parameter group), `step_size_up`,
    `step_size_down`, `mode` in {triangular, triangular2, exp_range}, `gamma` for exp_range.

    Two arguments are refused because the optimizers' updates read them on the HOST when the step is captured: a custom `scale_fn` is a
    Python callable and cannot run inside the graph (ValueError), and `cycle_momentum` would have to rewrite `momentum` / `betas`, which
    the optimizers read as host numbers at capture -- so it defaults to False here (the reference: True) and True raises
    NotImplementedError."""
    _KIND, _NAME = _lib.LR_CYCLIC, "CyclicLR"
    _MODES = {"triangular": _lib.LR_TRIANGULAR, "triangular2": _lib.LR_TRIANGULAR2, "exp_range": _lib.LR_EXP_RANGE}

    def __init__(self, optimizer, base_lr, max_lr, step_size_up=2000, step_size_down=None, mode="triangular", gamma=1., scale_fn=None,
                 scale_mode="cycle", cycle_momentum=False, base_momentum=0.8, max_momentum=0.9, last_epoch=-1, verbose=False):
        if not isinstance(optimizer, torch.optim.Optimizer):
            raise TypeError(f"{type(optimizer).__name__} is not an Optimizer")
        if scale_fn is not None:
            raise ValueError("mcquic_amd.schedule.CyclicLR: a custom scale_fn is a Python callable and cannot run inside a captured step; use `mode`")
        if cycle_momentum:
            raise NotImplementedError("mcquic_amd.schedule.CyclicLR: cycle_momentum is not supported (the optimizers read momentum / betas as host "
                                      "numbers when the step is captured)")
        if mode not in self._MODES:
            raise ValueError("mode is invalid and scale_fn is None")
        self._cyclic_base = [float(v) for v in self._format_param("base_lr", optimizer, base_lr)]
        self.max_lrs = [float(v) for v in self._format_param("max_lr", optimizer, max_lr)]
        up = float(step_size_up)
        down = float(step_size_down) if step_size_down is not None else up
        if not up > 0 or not down >= 0:
            raise ValueError(f"Invalid step sizes: up {step_size_up}, down {step_size_down}")
        self.total_size = up + down
        self.step_ratio = up / self.total_size
        self.mode, self.gamma = mode, float(gamma)
        if int(last_epoch) == -1:
            _check_optimizer(optimizer)
            for lr, group in zip(self._cyclic_base, optimizer.param_groups):
                if torch.is_tensor(group["lr"]):
                    group["lr"].fill_(lr)
                else:
                    group["lr"] = lr
        self._attach(optimizer, last_epoch)
        self.base_lrs = list(self._cyclic_base)

    @staticmethod
    def _format_param(name, optimizer, param):
        if isinstance(param, (list, tuple)):
            if len(param) != len(optimizer.param_groups):
                raise ValueError(f"expected {len(optimizer.param_groups)} values for {name}, got {len(param)}")
            return list(param)
        return [param] * len(optimizer.param_groups)

    def _initial_state(self, state, current, last_epoch):
        state[:, _MAX] = self.max_lrs                         # (the initial step runs on the groups' `initial_lr`, as the reference's does)
        return last_epoch, True

    def _after_initial_step(self, state) -> None:
        state[:, _BASE] = self._cyclic_base

    def _fill_rule(self, r) -> None:
        r.mode, r.gamma, r.total_size, r.step_ratio = self._MODES[self.mode], self.gamma, self.total_size, self.step_ratio

    def _params(self) -> dict:
        return {"base_lr": list(self._cyclic_base), "max_lr": list(self.max_lrs), "total_size": self.total_size, "step_ratio": self.step_ratio,
                "mode": self.mode, "gamma": self.gamma}


class CosineAnnealingWarmupRestarts(_DeviceScheduler):
    """lrSchedulers.py:306-481, what the reference trains with: linear warm-up over `warmup_steps` from min_lr = lr * lrScaleRatio to
    max_lr = lr, cosine down to min_lr at the end of the cycle, restart; each restart multiplies both bounds by `gamma` (gamma ** cycle
    on the base values) and stretches the cycle to `int((cur - warmup_steps) * cycle_mult) + warmup_steps`.  The sequential recurrence
    of `step(None)` runs on the device; `last_epoch=k` starts from the reference's closed form of `step(k)`.  The momentum arguments are
    dead in the reference too."""
    _KIND, _NAME = _lib.LR_COSINE, "CosineAnnealingWarmupRestarts"

    def __init__(self, optimizer, first_cycle_steps, cycle_mult=1., lrScaleRatio=0.001, warmup_steps=0, gamma=1., last_epoch=-1,
                 cycle_momentum=False, max_momentum=0.9, base_momentum=0.8, verbose=False):
        self.first_cycle_steps, self.warmup_steps = int(first_cycle_steps), int(warmup_steps)
        if not 0 <= self.warmup_steps < self.first_cycle_steps:
            raise ValueError(f"warmup_steps ({warmup_steps}) must be non-negative and smaller than first_cycle_steps ({first_cycle_steps})")
        self.cycle_mult, self.lrScaleRatio, self.gamma = float(cycle_mult), float(lrScaleRatio), float(gamma)
        if not self.cycle_mult > 0 or self.gamma != self.gamma:
            raise ValueError(f"Invalid cycle_mult / gamma: {cycle_mult}, {gamma}")
        self._attach(optimizer, last_epoch)

    def _initial_state(self, state, current, last_epoch):
        first, mult, gamma = self.first_cycle_steps, self.cycle_mult, self.gamma
        state[:, _MAX] = current
        state[:, _MIN] = state[:, _MIN_BASE] = [lr * self.lrScaleRatio for lr in current]
        cycle, cur, sic = 0, first, last_epoch
        if last_epoch == -1:
            state[:, _CYCLE], state[:, _SIC], state[:, _CUR] = cycle, sic, cur
            return -1, True                                    # `step(None)`: the device's rule, on the host
        epoch = last_epoch                                    # `step(epoch)`, lrSchedulers.py:465-479, as written
        if epoch >= first:
            if mult == 1.:
                sic = epoch % first
                cycle = epoch // first
            else:
                n = int(math.log((epoch / first * (mult - 1) + 1), mult))
                cycle = n
                sic = epoch - int(first * (mult ** n - 1) / (mult - 1))
                cur = first * mult ** (n)
            state[:, _MAX] = [lr * (gamma ** cycle) for lr in self.base_lrs]
            state[:, _MIN] = [lr * (gamma ** cycle) for lr in state[:, _MIN_BASE].tolist()]
        else:
            cur, sic = first, epoch
        state[:, _CYCLE], state[:, _SIC], state[:, _CUR] = cycle, sic, cur
        return last_epoch + 1, False                          # (`super().step()` counts the epoch once more; the rate is the state's)

    def _fill_rule(self, r) -> None:
        r.gamma, r.warmup_steps, r.cycle_mult = self.gamma, float(self.warmup_steps), self.cycle_mult

    def _params(self) -> dict:
        return {"first_cycle_steps": self.first_cycle_steps, "cycle_mult": self.cycle_mult, "lrScaleRatio": self.lrScaleRatio,
                "warmup_steps": self.warmup_steps, "gamma": self.gamma}


# the reference's scheduler registry (`LrSchedulerRegistry`, keys as mcquic/train/lrSchedulers.py registers them)
REGISTRY = {"Placeholder": Placeholder, "MultiStepLRWithWarmUp": MultiStepLRWithWarmUp, "CyclicLR": CyclicLR,
            "CosineAnnealingWarmupRestarts": CosineAnnealingWarmupRestarts}
