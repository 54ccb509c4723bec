"""The optimizer update of the training step (mcquic/train/trainer.py:283 `self._optimizer.step()`; the reference trains with
`Adam`, lr 1e-4, configs/a800_8.yaml:20-25) as ONE launch over the whole model: `mcq_adam_step_f32` (csrc/adam.hip; the device tables: csrc/tensor_list.h).

torch.optim.Adam(fused=True) hands its tensor lists to the GPU through kernel arguments, 4 KB at a time: 19 launches of ~91 us for
the qp=2 model's 666 tensors, 1.7 ms per step at 0.8 TB/s (docs/experiments.md section 9.11).  Here the lists are device arrays
(pointer tables + a chunk table), built once and rebuilt only when an address changes, and both moments live in two flat buffers
this object owns; the update is a one-thread kernel (step count, bias corrections, on the device) plus one pass over 28 bytes per
element.  Arithmetic and state layout are torch.optim.Adam's / AdamW's: `state_dict()` / `load_state_dict()` exchange checkpoints with
them (per-parameter `step`, `exp_avg`, `exp_avg_sq`), a learning rate given as a device tensor is read by the kernel on every
call (`mcquic_amd.schedule` fills it, on the device; a captured step needs no re-capture), and nothing is read back by the host, so
`parallel.GraphedTrainStep` captures it like any capturable optimizer.  float32 parameters on a HIP device only: there is no CPU path.

`Lamb` (alias `FusedLAMB`) is the reference's third optimizer (mcquic/train/ddp.py:53-69, apex FusedLAMB's arithmetic) on the same tables
and flat moment buffers: csrc/lamb.hip, five launches; `REGISTRY` maps the reference's `optim.key` names to these classes.

`SGD` is torch.optim.SGD's arithmetic and checkpoint layout on the same tables with one flat momentum buffer (none without momentum):
csrc/sgd.hip, the scalar kernel plus one pass; `max_grad_norm=` (clip_grad_norm_'s arithmetic) and `skip_nonfinite=` (a call whose
gradient norm is inf or NaN changes nothing and is counted in `skipped`) add one pass over the gradients.  `REGISTRY["SGD"]` stays
torch.optim.SGD, as the reference's registry has it: opt in by building `mcquic_amd.optim.SGD(model.parameters(), ...)` yourself.

`EMA` is not an optimizer: the exponential moving average of the weights on the same tables (row 1: the averages, one flat buffer),
csrc/ema.hip, the scalar kernel plus one pass, and a second kernel that exchanges live and averaged weights in place to evaluate the
average.  The reference has no such entry, so `REGISTRY` has none.

The non-finite guard (`mcquic_amd.guard`, csrc/step_guard.hip).  `Adam / AdamW / Lamb(..., skip_nonfinite=True)`: `step()` first forms the
global norm of its own gradients on the device (Adam: one pass over its gradient table; Lamb: the partials it computes anyway), and a
call whose norm is inf or NaN changes no parameter, no moment and no step count and is counted in `skipped` (a 0-dim int64 device
tensor), as `SGD(skip_nonfinite=True)` has always done inside its own kernel.  A clean call produces the bits it produces without the
option.  `attach_guard()` is how `parallel.GraphedTrainStep(..., skip_nonfinite=True)` drives all four with the step's ONE flag instead;
`EMA.update(skip=...)` takes the same flag."""
from __future__ import annotations

import torch

from . import _lib
from .ops import check, _guard, _stream
from .tensor_list import TensorList, chunk_tables, flat_layout  # noqa: F401  (`optim.chunk_tables` stays importable)

__all__ = ["Adam", "AdamW", "Lamb", "FusedLAMB", "SGD", "EMA", "REGISTRY"]


class _Planned(torch.optim.Optimizer):
    """What the optimizers of this module share: the per-parameter state (`_state_names`: both moments, or SGD's momentum buffer, or
    nothing) in flat buffers the object owns, one per name, and the device tables (pointers, sizes, chunks) the kernels walk, built once
    per parameter group and refilled only when an address changes."""
    _NAME = "?"

    def _state_names(self, group) -> tuple:
        """The per-parameter state tensors of `group`, by their names in `state_dict()`: one flat buffer each (at most two)."""
        return ("exp_avg", "exp_avg_sq")

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._plans = {}                                      # group index -> _Plan
        self._norm = None                                     # (see `_planned`)
        self._guard_own = False                               # Adam / Lamb(skip_nonfinite=True): `_guard` is this object's own
        self._guard = None                                    # a guard.StepGuard: own, or the step's (`attach_guard`)
        self._guard_decided = False                           # the step's guard has run before `step()` is called

    # ---- state in flat buffers -------------------------------------------------------------------------------------------------
    class _Plan:
        __slots__ = ("table", "flat_m", "flat_v", "views", "step", "scalars", "ids", "adopted", "names")
        ntensors = property(lambda self: self.table.ntensors)
        nblocks = property(lambda self: self.table.nblocks)

    def _flat_state(self, gi: int, params):
        """The plan of group `gi` for `params`: `flat_m` / `flat_v` (the flat buffers of the group's first / second state name, None where
        there is none), `views` [one tuple of views per parameter], `step`; state found in `self.state` that does not live in the flat
        buffers (loaded from a checkpoint, or set by hand) is copied in and replaced by views."""
        plan = self._plans.get(gi)
        ids = [id(p) for p in params]
        names = tuple(self._state_names(self.param_groups[gi]))
        same = plan is not None and plan.ids == ids and plan.names == names and plan.step.device == params[0].device
        if same and plan.adopted:
            return plan
        sizes = [p.numel() for p in params]
        if not same:
            # (also when the set of parameters that carry a gradient changed: fresh buffers, the old state is copied over below)
            plan = self._plans[gi] = type(self)._Plan()
            dev = params[0].device
            plan.ids, plan.names = ids, names
            offs, total = flat_layout(sizes)
            flats = [torch.zeros(total, dtype=torch.float32, device=dev) for _ in names]
            plan.flat_m, plan.flat_v = (flats + [None, None])[:2]
            plan.views = [tuple(f[o: o + n].view_as(p) for f in flats) for o, n, p in zip(offs, sizes, params)]
            plan.step = torch.zeros((), dtype=torch.float32, device=dev)
            plan.scalars = torch.zeros(4, dtype=torch.float32, device=dev)
            plan.table = TensorList(sizes, dev, moved=f"mcquic_amd.optim.{self._NAME}: parameter / gradient addresses changed since the last step")
            # (rows 2 and 3, the state, are the plan's own and filled once; rows of a state the group does not have stay 0: no kernel reads them)
            plan.table.fill(params, [p.grad for p in params], *([views[k] for views in plan.views] for k in range(len(names))))
            self._extend_plan(plan, dev)
        for p, views in zip(params, plan.views):
            st = self.state[p]
            for name, view in zip(names, views):
                old = st.get(name)
                if old is not None and old.data_ptr() != view.data_ptr():
                    view.copy_(old.to(view.device, torch.float32))
                st[name] = view
            old_s = st.get("step")
            if old_s is not None and old_s is not plan.step:  # (torch keeps one count per parameter; they move together)
                plan.step.copy_(torch.as_tensor(old_s, dtype=torch.float32).to(plan.step.device))
            st["step"] = plan.step
        plan.adopted = True
        return plan

    def _extend_plan(self, plan, dev) -> None:
        """What a subclass adds to a new plan."""

    def _checked(self, group):
        params = [p for p in group["params"] if p.grad is not None]
        for p in params:
            g = p.grad
            if not (p.is_cuda and g.is_cuda and p.dtype == torch.float32 and g.dtype == torch.float32 and p.is_contiguous() and g.is_contiguous()
                    and not g.is_sparse):
                raise RuntimeError(f"mcquic_amd.optim.{self._NAME}: contiguous float32 parameters and gradients on a HIP device only "
                                   "(there is no CPU path)")
            if p.device != params[0].device:
                raise RuntimeError(f"mcquic_amd.optim.{self._NAME}: the parameters of one group must live on one device (one launch per group)")
        return params

    @torch.no_grad()
    def prepare(self) -> None:
        """Build the state buffers and the device tables for the gradients the parameters hold NOW, without updating anything: what
        `parallel.GraphedTrainStep` calls before it captures `step()` (table uploads are host-to-device copies)."""
        self._planned()

    # ---- what a training step asks (parallel.GraphedTrainStep) ---------------------------------------------------------------------
    guards_itself = property(lambda self: self._guard_own, doc="Its own `skip_nonfinite` is on: a step's guard beside it is refused.")
    lends_norm = False                                        # it computes the norm of all gradients: a guard borrows the partials

    def last_grad_norm(self):
        """The device tensor that holds G of the last step, or None (no step yet, or an optimizer that computes none)."""
        return self._norm[2] if self.lends_norm and self._norm is not None else None

    def skip_count(self):
        """`skipped` where the optimizer has the counter (its own `skip_nonfinite`; SGD always), else None."""
        return self.skipped if self._guard_own else None

    # ---- the non-finite guard ----------------------------------------------------------------------------------------------------
    def attach_guard(self, guard, decided: bool = False) -> None:
        """Obey a step's guard (`guard.StepGuard`; None detaches): every launch of `step()` takes its flag.  `decided`: the caller runs
        the guard itself before each `step()` (over the flat gradient buffer, or from its clipping's norm); otherwise `step()` runs it --
        from the partials of the gradient norm where this optimizer computes them (Lamb; SGD with `max_grad_norm`), else over its own
        gradient tables.  Refused beside the optimizer's own `skip_nonfinite`: two guards would count one step twice."""
        if guard is not None and self.guards_itself:
            raise ValueError(f"mcquic_amd.optim.{self._NAME}: both the step and the optimizer guard against a non-finite gradient "
                             "(`skip_nonfinite`): one step would be counted twice; set one of them")
        self._guard, self._guard_decided = guard, bool(decided) and guard is not None

    def _own_guard(self, todo) -> None:
        """(from `_planned`, outside any capture) the optimizer's own guard and the scratch its reduction needs."""
        if self._guard_own and todo:
            from .guard import StepGuard
            dev = todo[0][1].step.device
            if self._guard is None or self._guard.device != dev:
                old, self._guard = self._guard, StepGuard(dev)
                if old is not None:
                    self._guard.record.copy_(old.record)
        if self._guard is not None and todo and not self._guard_decided:
            self._guard._room(sum(plan.nblocks for _, plan in todo))

    def _flag(self, todo, partials=None, total: int = 0):
        """The address of the flag this call's launches obey (None: no guard), after running the guard where that is this call's job."""
        guard = self._guard
        if guard is None:
            return None
        if not self._guard_decided:
            if partials is not None:
                guard.from_partials(partials, total)          # (the norm's partials exist already: no second pass over the gradients)
            else:
                guard.run_list([plan.table for _, plan in todo])
        return guard.skip.data_ptr()

    @property
    def skipped(self) -> torch.Tensor:
        """How many calls this optimizer's own guard has skipped (0-dim int64 on the device).  Adam / AdamW / Lamb have the counter with
        `skip_nonfinite=True` only: without it nothing counts, and the attribute is absent as it always was."""
        if not self._guard_own:
            raise AttributeError(f"mcquic_amd.optim.{self._NAME}: `skipped` exists with skip_nonfinite=True only")
        if self._guard is None:
            from .guard import StepGuard
            self._guard = StepGuard(next(p.device for g in self.param_groups for p in g["params"]))
        return self._guard.skipped

    def _planned(self):
        """[(group, plan)] of the groups that hold gradients, tables current, and -- for an optimizer that `lends_norm` -- the buffers
        of the gradient norm they share: `self._norm` = (key, double partials of sum g^2 for all groups, G)."""
        live = []
        for gi, group in enumerate(self.param_groups):
            params = self._checked(group)
            if params:
                if live and self.lends_norm and params[0].device != live[0][2][0].device:
                    raise RuntimeError(f"mcquic_amd.optim.{self._NAME}: all param groups must live on one device (the gradient norm spans them)")
                live.append((gi, group, params))
        out = []
        for gi, group, params in live:
            plan = self._flat_state(gi, params)
            plan.table.fill(params, [p.grad for p in params])
            out.append((group, plan))
        key = tuple((id(plan), plan.nblocks) for _, plan in out)
        if out and self.lends_norm and (self._norm is None or self._norm[0] != key):
            dev = out[0][1].step.device
            gnorm = self._norm[2] if self._norm is not None and self._norm[2].device == dev else torch.zeros((), dtype=torch.float32, device=dev)
            self._norm = (key, torch.zeros(max(sum(plan.nblocks for _, plan in out), 1), dtype=torch.float64, device=dev), gnorm)
        self._own_guard([(g, plan) for g, plan in out if plan.nblocks > 0])
        return out

    def _grad_partials(self, todo, skip=None):
        """(partials, total, G) for an optimizer that `lends_norm`, (None, 0, None) otherwise: the per-chunk sums of g^2 of every plan of
        `todo`, one launch each into one array of `total` doubles, from which every group's update derives the same norm G."""
        if not self.lends_norm:
            return None, 0, None
        _, partials, gnorm = self._norm
        total = 0
        with _guard(gnorm.device):
            for _, plan in todo:
                check(_lib.load().mcq_lamb_grad_partials_skip_f32(*plan.table.args(), partials.data_ptr() + 8 * total, skip, _stream()),
                      "mcq_lamb_grad_partials_skip_f32")
                total += plan.nblocks
        return partials, total, gnorm

    def _begin(self, closure):
        """The opening every `step()` shares: (todo, partials, total, G, flag) -- the non-empty plans (none: nothing to launch), the norm
        of ALL gradients first where the optimizer forms one, then ONE decision for all groups before any is updated.  With a guard that
        has not decided yet the flag comes from those partials (Lamb, SGD: no second pass), else from a pass over the gradient tables."""
        if closure is not None:
            raise NotImplementedError(f"mcquic_amd.optim.{self._NAME}: closures are not supported (the reference's trainer passes none)")
        todo = [(group, plan) for group, plan in self._planned() if plan.nblocks > 0]
        if not todo:
            return todo, None, 0, None, None
        decided = self._guard.skip.data_ptr() if self._guard is not None and self._guard_decided else None
        partials, total, gnorm = self._grad_partials(todo, decided)
        return todo, partials, total, gnorm, self._flag(todo, partials, total)

    def load_state_dict(self, state_dict):
        """The loaded tensors are copied INTO the existing flat buffers on the next step (same parameters: same addresses, which a
        captured update may hold); only a plan whose parameter set changed is rebuilt."""
        super().load_state_dict(state_dict)
        for plan in self._plans.values():
            plan.adopted = False

    @staticmethod
    def _check_adam_args(lr, betas, eps, weight_decay) -> None:
        if not torch.is_tensor(lr) and not lr >= 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid betas: {betas}")
        if not eps >= 0.0 or not weight_decay >= 0.0:
            raise ValueError("eps and weight_decay must be non-negative")

    def state_dict(self):
        """Every parameter gets a `step` tensor of ITS OWN (here a group shares one): torch's optimizers increment each entry they are
        handed, so a shared one would be advanced once per parameter after loading there."""
        sd = super().state_dict()
        sd["state"] = {k: {n: (v.clone() if n == "step" and torch.is_tensor(v) else v) for n, v in st.items()} for k, st in sd["state"].items()}
        return sd

    def _rate(self, group):
        """(device tensor or None, host value) of a group's learning rate."""
        lr = group["lr"]
        if torch.is_tensor(lr):
            if lr.is_cuda:
                if lr.dtype != torch.float32 or lr.numel() != 1:
                    raise TypeError(f"mcquic_amd.optim.{self._NAME}: a device learning rate must be one float32")
                return lr, 0.0
        return None, float(lr)


class Adam(_Planned):
    _NAME = "Adam"
    """torch.optim.Adam(params, lr, betas, eps, weight_decay, maximize=...) without `amsgrad` / `foreach` / `differentiable`;
    `decoupled=True` makes the decay AdamW's (`AdamW` below sets it and AdamW's default of 1e-2)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, *, decoupled: bool = False,
                 maximize: bool = False, skip_nonfinite: bool = False):
        self._check_adam_args(lr, betas, eps, weight_decay)
        # (capturable=True is what torch's load_state_dict looks at to keep `step` a float32 device tensor)
        super().__init__(params, dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, decoupled=bool(decoupled),
                                      maximize=bool(maximize), capturable=True))
        self._guard_own = bool(skip_nonfinite)

    @torch.no_grad()
    def step(self, closure=None):
        todo, _, _, _, flag = self._begin(closure)            # (no norm of its own: a guard looks at the gradient tables)
        lib = _lib.load()
        for group, plan in todo:
            lr_dev, lr_host = self._rate(group)
            b1, b2 = group["betas"]
            with _guard(plan.step.device):
                check(lib.mcq_adam_step_skip_f32(*plan.table.args(), plan.step.data_ptr(), None if lr_dev is None else lr_dev.data_ptr(),
                                                 float(lr_host), float(b1), float(b2), float(group["eps"]), float(group["weight_decay"]),
                                                 1 if group["decoupled"] else 0, 1 if group["maximize"] else 0, plan.scalars.data_ptr(), flag,
                                                 _stream()), "mcq_adam_step_skip_f32")
        return None

    def state_dict(self):
        """torch.optim.Adam's layout."""
        sd = super().state_dict()
        # torch spells the decoupled decay `decoupled_weight_decay` (torch.optim.AdamW sets it): both names travel
        sd["param_groups"] = [dict(g, decoupled_weight_decay=bool(g.get("decoupled", False))) for g in sd["param_groups"]]
        return sd

    def load_state_dict(self, state_dict):
        """torch.optim.Adam / AdamW checkpoints load as they are (per-parameter `step`, `exp_avg`, `exp_avg_sq`); the tensors move
        into the flat buffers on the next `step()`."""
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            # (torch replaces the groups by the saved ones: a torch.optim.AdamW checkpoint carries `decoupled_weight_decay: True` and
            #  no `decoupled` -- dropping it would turn the decay into Adam's L2 term silently)
            group["decoupled"] = bool(group.get("decoupled", group.get("decoupled_weight_decay", isinstance(self, AdamW))))
            group["decoupled_weight_decay"] = group["decoupled"]
            group.setdefault("maximize", False)
            group["capturable"] = True
            for k in ("amsgrad", "foreach", "fused", "differentiable"):
                if group.get(k):
                    raise NotImplementedError(f"mcquic_amd.optim.Adam: `{k}` checkpoints are not supported")


class AdamW(Adam):
    """torch.optim.AdamW: decoupled weight decay (param *= 1 - lr * weight_decay before the update), default 1e-2."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2, *, maximize: bool = False,
                 skip_nonfinite: bool = False):
        super().__init__(params, lr, betas, eps, weight_decay, decoupled=True, maximize=maximize, skip_nonfinite=skip_nonfinite)


class Lamb(_Planned):
    """LAMB with apex `FusedLAMB`'s arithmetic and constructor (the reference's `"FusedLAMB"` registry entry, mcquic/train/ddp.py:53-69;
    apex is not available on this platform and torch ships no LAMB): csrc/lamb.hip, five launches per parameter group whatever the
    number of tensors, nothing read back by the host.  One `step()`:

      1. G = sqrt(sum g^2) over every parameter that has a gradient, in EVERY group, before any group is updated;
      2. c = G / max_grad_norm if G > max_grad_norm else 1 (a NaN G compares false);
      3. per group t += 1; beta3 = 1 - beta1 if grad_averaging else 1; bc1 = 1 - beta1^t, bc2 = 1 - beta2^t (1 without bias_correction);
      4. g^ = g / c.  L2 mode (adam_w_mode=False): g^ += wd p; m = beta1 m + beta3 g^; v = beta2 v + (1 - beta2) g^2;
         u = (m / bc1) / (sqrt(v / bc2) + eps).  AdamW mode: m, v from the plain g^ and u += wd p;
      5. per tensor ||p|| (before the update) and ||u||;
      6. r = lr; if use_nvlamb or wd != 0: r = lr ||p|| / ||u|| where both norms are non-zero.  p -= r u.

    Gradients are left as they were (apex overwrites them with u).  `amsgrad` is not supported; `set_grad_none` only sets the default
    of `zero_grad`.  State layout is Adam's (per-parameter `step`, `exp_avg`, `exp_avg_sq`); `load_state_dict` also takes apex's
    (an integer `step` in the param group, none per parameter).  All groups live on one device: the gradient norm spans them.
    After a step, without any host synchronisation: `grad_norm` (G, a 0-dim device tensor) and `trust_ratios(group)`."""
    _NAME = "Lamb"

    class _Plan(_Planned._Plan):
        __slots__ = ("workspace", "ratios")

    def __init__(self, params, lr=1e-3, bias_correction=True, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, amsgrad=False,
                 adam_w_mode=True, grad_averaging=True, set_grad_none=True, max_grad_norm=1.0, use_nvlamb=False, skip_nonfinite=False):
        if amsgrad:
            raise RuntimeError("mcquic_amd.optim.Lamb does not support the AMSGrad variant.")
        self._check_adam_args(lr, betas, eps, weight_decay)
        if not max_grad_norm >= 0.0:
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm}")
        super().__init__(params, dict(lr=lr, bias_correction=bool(bias_correction), betas=tuple(betas), eps=eps, weight_decay=weight_decay,
                                      grad_averaging=bool(grad_averaging), max_grad_norm=max_grad_norm, adam_w_mode=bool(adam_w_mode),
                                      use_nvlamb=bool(use_nvlamb), capturable=True))
        self.set_grad_none = bool(set_grad_none)
        self._guard_own = bool(skip_nonfinite)

    def zero_grad(self, set_to_none=None):
        super().zero_grad(self.set_grad_none if set_to_none is None else set_to_none)

    lends_norm = True

    def _extend_plan(self, plan, dev) -> None:
        plan.table.tensor_first_blk                           # (uploaded now: the first `step()` after `prepare()` may be a captured one)
        nbytes = _lib.load().mcq_lamb_workspace_bytes(plan.ntensors, max(plan.nblocks, 1))
        plan.workspace = torch.zeros((nbytes + 7) // 8, dtype=torch.float64, device=dev)
        plan.ratios = torch.zeros(plan.ntensors, dtype=torch.float32, device=dev)

    @property
    def grad_norm(self) -> torch.Tensor:
        """G of the last step: the norm of all gradients before clipping (0-dim float32 on the device)."""
        if self._norm is None:
            raise RuntimeError("mcquic_amd.optim.Lamb: no step has run yet")
        return self._norm[2]

    def trust_ratios(self, group: int = 0) -> torch.Tensor:
        """||p|| / ||u|| of the last step for every tensor of `group` that had a gradient, in the group's order ([ntensors] float32 on the
        device; inf / 0 / NaN where a norm is zero -- the update uses the plain learning rate there)."""
        plan = self._plans.get(group)
        if plan is None:
            raise RuntimeError("mcquic_amd.optim.Lamb: no step has run yet for this group")
        return plan.ratios

    @torch.no_grad()
    def step(self, closure=None):
        todo, partials, total, gnorm, flag = self._begin(closure)       # (with a guard: the flag from the partials of LAMB's own G)
        if not todo:
            return None
        lib = _lib.load()
        with _guard(gnorm.device):
            for group, plan in todo:                          # every group's update reads the same partials
                lr_dev, lr_host = self._rate(group)
                b1, b2 = group["betas"]
                check(lib.mcq_lamb_step_skip_f32(*plan.table.args(first_blk=True), partials.data_ptr(), total, plan.step.data_ptr(),
                                                 None if lr_dev is None else lr_dev.data_ptr(), float(lr_host), float(b1),
                                                 float(b2), float(group["eps"]), float(group["weight_decay"]), 1 if group["bias_correction"] else 0,
                                                 1 if group["adam_w_mode"] else 0, 1 if group["grad_averaging"] else 0,
                                                 1 if group["use_nvlamb"] else 0, float(group["max_grad_norm"]), gnorm.data_ptr(),
                                                 plan.ratios.data_ptr(), plan.workspace.data_ptr(), plan.scalars.data_ptr(), flag, _stream()),
                      "mcq_lamb_step_skip_f32")
        return None

    def load_state_dict(self, state_dict):
        """Our own checkpoints, and apex FusedLAMB's: there the count is an integer `step` of the param group and the per-parameter
        state holds the two moments only.  The tensors move into the flat buffers on the next `step()`, at the same addresses."""
        groups = [dict(g) for g in state_dict["param_groups"]]
        state = {k: dict(v) for k, v in state_dict["state"].items()}
        for g in groups:
            if "step" in g:
                count = g.pop("step")
                for pid in g["params"]:
                    if pid in state and "step" not in state[pid]:
                        state[pid]["step"] = torch.tensor(float(count), dtype=torch.float32)
        super().load_state_dict({"state": state, "param_groups": groups})
        for group in self.param_groups:
            if group.get("amsgrad"):
                raise NotImplementedError("mcquic_amd.optim.Lamb: `amsgrad` checkpoints are not supported")
            for k in ("bias_correction", "grad_averaging", "max_grad_norm", "adam_w_mode", "use_nvlamb"):
                group.setdefault(k, self.defaults[k])         # (apex keeps adam_w_mode / use_nvlamb on the object, not in the groups)
            group["capturable"] = True


class SGD(_Planned):
    """torch.optim.SGD(params, lr, momentum, dampening, weight_decay, nesterov, maximize=...) without `foreach` / `fused` /
    `differentiable`: csrc/sgd.hip, the whole parameter group in one launch behind a one-thread kernel.  Per element, in float32:

      g = -grad if maximize else grad;  g += weight_decay p;
      with momentum: buf = g on the first update, else buf = momentum buf + (1 - dampening) g;  g = g + momentum buf if nesterov else buf;
      p -= lr g.

    The momentum buffers are views of ONE flat buffer (none is allocated without momentum).  Two options add one pass over the gradients,
    the per-chunk sums of g^2 over every parameter that has a gradient, in EVERY group, summed on the device to the norm G:
      max_grad_norm   every gradient enters as grad * min(1, max_grad_norm / (G + 1e-6)): torch.nn.utils.clip_grad_norm_ in front of the
                      step, without touching the gradients;
      skip_nonfinite  a call whose G is inf or NaN changes no parameter, no buffer and no step count; `skipped` counts such calls.
    Nothing is read by the host: `grad_norm()` and `skipped` are device tensors.  `state_dict()` / `load_state_dict()` exchange checkpoints
    with torch.optim.SGD (`momentum_buffer` per parameter, nothing without momentum).  torch keeps no step count: a loaded buffer means
    "not the first update"; a group loaded without any buffer starts with one (parameters that lack a buffer while others of their
    group have one start from zeros)."""
    _NAME = "SGD"

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, *, maximize: bool = False,
                 max_grad_norm=None, skip_nonfinite: bool = False):
        if torch.is_tensor(lr) and lr.numel() != 1:
            raise ValueError("Tensor lr must be 1-element")
        if not torch.is_tensor(lr) and not lr >= 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not momentum >= 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if not weight_decay >= 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        if max_grad_norm is not None and not max_grad_norm > 0.0:
            raise ValueError(f"Invalid max_grad_norm: {max_grad_norm} (positive, or None: no clipping)")
        # (the keys torch.optim.SGD's step reads from a loaded group travel with ours)
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=bool(nesterov),
                                      maximize=bool(maximize), foreach=None, differentiable=False, fused=None))
        self.max_grad_norm, self.skip_nonfinite = max_grad_norm, bool(skip_nonfinite)
        self._bound = self._skipped = None                    # device tensors: the clip bound, the count of skipped calls

    def _state_names(self, group) -> tuple:
        return ("momentum_buffer",) if group["momentum"] != 0 else ()

    guards_itself = property(lambda self: self.skip_nonfinite)          # (inside its scalar kernel, with a counter of its own)
    lends_norm = property(lambda self: self.max_grad_norm is not None or self.skip_nonfinite)

    def skip_count(self):
        return self.skipped

    def _planned(self):
        out = super()._planned()
        if out:                                               # (created here, outside any capture: `prepare()` comes through)
            dev = out[0][1].step.device
            if self.max_grad_norm is not None and (self._bound is None or self._bound.device != dev):
                self._bound = torch.tensor(float(self.max_grad_norm), dtype=torch.float32).to(dev)
            if self._skipped is None or self._skipped.device != dev:
                self._skipped = torch.zeros((), dtype=torch.int64, device=dev) if self._skipped is None else self._skipped.to(dev)
        return out

    def grad_norm(self) -> torch.Tensor:
        """G of the last call, skipped or not: the norm of all gradients before clipping (0-dim float32 on the device)."""
        if not self.lends_norm:
            raise RuntimeError("mcquic_amd.optim.SGD: the gradient norm is computed only with `max_grad_norm` or `skip_nonfinite`")
        if self._norm is None:
            raise RuntimeError("mcquic_amd.optim.SGD: no step has run yet")
        return self._norm[2]

    @property
    def skipped(self) -> torch.Tensor:
        """How many calls the non-finite guard has skipped (0-dim int64 on the device; stays 0 without `skip_nonfinite`)."""
        if self._skipped is None:
            dev = next((p.device for g in self.param_groups for p in g["params"]), None)
            self._skipped = torch.zeros((), dtype=torch.int64, device=dev)
        return self._skipped

    @torch.no_grad()
    def step(self, closure=None):
        # (the norm with clipping or a guard only; the flag is a step's guard's, `attach_guard`: SGD's own lives in its scalar kernel)
        todo, partials, total, gnorm, flag = self._begin(closure)
        lib = _lib.load()
        for i, (group, plan) in enumerate(todo):              # (every group derives the same factor and flag; the first one counts a skip)
            lr_dev, lr_host = self._rate(group)
            with _guard(plan.step.device):
                check(lib.mcq_sgd_step_skip_f32(*plan.table.args(), plan.step.data_ptr(),
                                           None if lr_dev is None else lr_dev.data_ptr(), float(lr_host), float(group["momentum"]),
                                           float(group["dampening"]), float(group["weight_decay"]), 1 if group["nesterov"] else 0,
                                           1 if group["maximize"] else 0, None if partials is None else partials.data_ptr(), total,
                                           None if self.max_grad_norm is None else self._bound.data_ptr(),
                                           None if gnorm is None else gnorm.data_ptr(), 1 if self.skip_nonfinite else 0,
                                           self._skipped.data_ptr() if self.skip_nonfinite and i == 0 else None, plan.scalars.data_ptr(), flag,
                                           _stream()), "mcq_sgd_step_skip_f32")
        return None

    def state_dict(self):
        """torch.optim.SGD's layout: `momentum_buffer` per parameter and nothing else (the step count every plan keeps is ours)."""
        sd = super().state_dict()
        state = {k: {n: v for n, v in st.items() if n != "step"} for k, st in sd["state"].items()}
        sd["state"] = {k: st for k, st in state.items() if st}
        return sd

    def load_state_dict(self, state_dict):
        """torch.optim.SGD checkpoints load as they are; the buffers move into the flat buffer on the next `step()`, at the same
        addresses.  A group that comes with a buffer continues (its next update is not a first one); one without starts over."""
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            for k in ("foreach", "fused", "differentiable"):
                if group.get(k):
                    raise NotImplementedError(f"mcquic_amd.optim.SGD: `{k}` checkpoints are not supported")
            group.update(foreach=None, differentiable=False, fused=None)
            for k in ("nesterov", "maximize"):
                group.setdefault(k, False)
            held = [p for p in group["params"] if p in self.state]
            for p in held:
                if self.state[p].get("momentum_buffer", 0) is None:
                    del self.state[p]["momentum_buffer"]
            count = 1.0 if any("momentum_buffer" in self.state[p] for p in held) else 0.0
            for p in group["params"]:
                self.state[p]["step"] = torch.tensor(count, dtype=torch.float32)


class EMA:
    """Exponential moving average of a model's weights, the whole model in one launch (csrc/ema.hip), and the model evaluated under
    its average without a second module or a third copy of the weights:

        ema = EMA(model, decay=0.9999, warmup=True)      # model: an nn.Module, or an iterable of parameters
        ema.update()                                     # after optimizer.step(): one scalar kernel + one pass; capturable after prepare()
        with ema.applied(): model.eval(); ...            # the model runs under the averaged weights; the live ones come back on exit
        ema.averaged_state_dict()                        # the model's state_dict with the averaged parameters in place of the live ones

    Averaged are the floating-point parameters with `requires_grad` (float32 on a HIP device: there is no CPU path); every other entry
    of the model's `state_dict` -- frozen parameters, buffers such as the frequency EMA -- is the live model's.  Built from an iterable
    of parameters, exactly those are averaged.  The averages are views of ONE flat float32 buffer, initialised as a copy of the
    parameters.  Per element, in float32, avg = lerp(avg, p, 1 - d_t) with torch's lerp (what `torch.optim.swa_utils.AveragedModel`
    runs with `get_ema_multi_avg_fn(decay)`): avg + (1 - d_t) (p - avg), in the form p - (p - avg) d_t once 1 - d_t >= 0.5, so decay 0
    tracks the parameters bit for bit.  d_t = decay, with `warmup` min(decay, (1 + n) / (10 + n)) after n updates: 1/10, 2/11, 3/12, ...
    `decay` may be a 0-dim float32 device tensor, read by the kernel on every call (a schedule under capture).  The update count lives
    on the device and is advanced there, so captured replays count; `num_updates` reads it back.

    `swap()` exchanges the live and the averaged weights in place, as raw words (one launch; two swaps are the identity on bits), and
    bumps the version counter of every swapped parameter, so eager code re-packs its operand streams and `enableGraphs` captures are
    dropped by the weight stamp.  (`GraphedTrainStep.invalidate()`'s `_foreach_add_(params, 0.0)` would do that too but turns -0.0
    into +0.0; the bump alone changes no value.)  While swapped, `update()` raises."""

    def __init__(self, model, decay=0.9999, warmup: bool = True):
        if isinstance(model, torch.nn.Module):
            self.model = model
            named = [(n, p) for n, p in model.named_parameters() if p.requires_grad and p.is_floating_point()]
        else:
            self.model = None
            named = [(str(i), p) for i, p in enumerate(model)]
        if torch.is_tensor(decay):
            if decay.numel() != 1:
                raise ValueError("Tensor decay must be 1-element")
        elif not 0.0 <= decay <= 1.0:
            raise ValueError(f"Invalid decay: {decay}")
        if not named or not any(p.numel() for _, p in named):
            raise ValueError("mcquic_amd.optim.EMA: nothing to average")
        for n, p in named:
            if p.dtype != torch.float32:
                raise RuntimeError(f"mcquic_amd.optim.EMA: float32 parameters only ({n} is {p.dtype})")
            if p.device != named[0][1].device:
                raise RuntimeError("mcquic_amd.optim.EMA: the parameters must live on one device (one launch)")
        self.decay, self.warmup = decay, bool(warmup)
        self.names, self.params = [n for n, _ in named], [p for _, p in named]
        self.sizes = [p.numel() for p in self.params]
        dev = self.params[0].device
        self._layout(torch.zeros(flat_layout(self.sizes)[1], dtype=torch.float32, device=dev))
        with torch.no_grad():
            for v, p in zip(self.averages, self.params):
                v.copy_(p)
        self._count = torch.zeros((), dtype=torch.int64, device=dev)
        self._scalars = torch.zeros(4, dtype=torch.float32, device=dev)
        self.swapped = False

    def _layout(self, flat) -> None:
        self._flat = flat
        self.averages = [flat[o: o + n].view(p.shape) for o, n, p in zip(flat_layout(self.sizes)[0], self.sizes, self.params)]
        self._table = None                                    # (a TensorList on the buffer's device; row 1 holds the views' addresses)

    # ---- device tables ---------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def prepare(self) -> None:
        """Build the device tables for the addresses the parameters have NOW, without updating anything: what
        `parallel.GraphedTrainStep` calls before it captures `update()` (table uploads are host-to-device copies).  Rebuilt when a
        parameter's storage address changes."""
        dev = self.params[0].device
        for p in self.params:
            if not (p.is_cuda and p.is_contiguous() and p.device == dev):
                raise RuntimeError("mcquic_amd.optim.EMA: contiguous float32 parameters on one HIP device only (there is no CPU path)")
        if self._flat.device != dev:                          # (the model moved since construction)
            self._count, self._scalars = self._count.to(dev), self._scalars.to(dev)
            self._layout(self._flat.to(dev))
        if self._table is None:                               # (the kernels read rows 0 and 1 only; the averages' row is filled once)
            self._table = TensorList(self.sizes, dev, rows=2, moved="mcquic_amd.optim.EMA: parameter addresses changed since the last call")
            self._table.fill(self.params, self.averages)
        self._table.fill(self.params)

    # ---- the average -----------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def update(self, skip=None) -> None:
        """`skip`: a step's guard flag (one int32 on the device, `guard.StepGuard.skip`): when it is set on the device, neither an
        average nor the update count moves.  None: the launches are the ones they have always been."""
        if self.swapped:
            raise RuntimeError("mcquic_amd.optim.EMA: the averaged weights are swapped in (`swap()` / `applied()`): the model holds the average, "
                               "not the iterate; swap back before `update()`")
        self.prepare()
        decay = self.decay
        if torch.is_tensor(decay) and (not decay.is_cuda or decay.dtype != torch.float32 or decay.numel() != 1):
            raise TypeError("mcquic_amd.optim.EMA: a tensor decay must be one float32 on the device")
        dev = torch.is_tensor(decay)
        from .guard import skip_pointer
        flag = skip_pointer(skip, self._flat.device, "mcquic_amd.optim.EMA.update")
        with _guard(self._flat.device):
            check(_lib.load().mcq_ema_update_skip_f32(*self._table.args(), self._count.data_ptr(), decay.data_ptr() if dev else None,
                                                      0.0 if dev else float(decay), 1 if self.warmup else 0, self._scalars.data_ptr(), flag,
                                                      _stream()), "mcq_ema_update_skip_f32")

    @torch.no_grad()
    def warm(self) -> None:
        """One throw-away update, so that the kernels' first launch happens outside any capture; averages and count keep their bits."""
        flat, count = self._flat.clone(), self._count.clone()
        self.update()
        self._flat.copy_(flat)
        self._count.copy_(count)

    @property
    def num_updates(self) -> int:
        """How many updates have run, captured replays included (reads the device counter: a host synchronisation)."""
        return int(self._count)

    # ---- evaluating under the average ------------------------------------------------------------------------------------------
    @torch.no_grad()
    def swap(self) -> None:
        """Exchange the live and the averaged weights in place (one launch) and mark every swapped parameter changed."""
        self.prepare()
        with _guard(self._flat.device):
            check(_lib.load().mcq_ema_swap_f32(*self._table.args(), _stream()), "mcq_ema_swap_f32")
        self.swapped = not self.swapped
        for p in self.params:
            torch.autograd.graph.increment_version(p)

    def applied(self):
        """Context manager: swap, run the body under the averaged weights, swap back (the same bits as before)."""
        import contextlib

        @contextlib.contextmanager
        def ctx():
            self.swap()
            try:
                yield self
            finally:
                self.swap()
        return ctx()

    def _averaged(self):
        """The averaged values, wherever they are right now."""
        return [p.detach() for p in self.params] if self.swapped else self.averages

    def averaged_state_dict(self) -> dict:
        """The model's `state_dict()` with the averaged parameters in place of the live ones (references, as `state_dict()` returns
        them; every other entry is the live model's): what `Compressor.load_state_dict` takes."""
        if self.model is None:
            raise RuntimeError("mcquic_amd.optim.EMA: built from an iterable of parameters: there is no model whose state_dict to fill")
        sd = self.model.state_dict()
        for n, v in zip(self.names, self._averaged()):
            sd[n] = v
        return sd

    def state_dict(self) -> dict:
        return {"averages": {n: v.clone() for n, v in zip(self.names, self._averaged())}, "num_updates": self.num_updates,
                "decay": float(self.decay), "warmup": self.warmup}

    @torch.no_grad()
    def load_state_dict(self, sd) -> None:
        """Averages (by name, into the flat buffer: the same addresses, which a captured update may hold), update count, decay (a
        tensor decay is refilled) and warmup."""
        if self.swapped:
            raise RuntimeError("mcquic_amd.optim.EMA: swap back before loading")
        if set(sd["averages"]) != set(self.names):
            raise KeyError("mcquic_amd.optim.EMA: the checkpoint averages other parameters than this object")
        for n, v in zip(self.names, self.averages):
            src = sd["averages"][n]
            if tuple(src.shape) != tuple(v.shape):
                raise RuntimeError(f"mcquic_amd.optim.EMA: {n} has shape {tuple(v.shape)}, the checkpoint {tuple(src.shape)}")
            v.copy_(src.to(v.device, torch.float32))
        self._count.fill_(int(sd["num_updates"]))
        if torch.is_tensor(self.decay):
            self.decay.fill_(float(sd["decay"]))
        else:
            self.decay = float(sd["decay"])
        self.warmup = bool(sd["warmup"])


FusedLAMB = Lamb
# the reference's optimizer registry (mcquic/train/ddp.py:53-69), with its meanings: `"Adam"` is AdamW there
REGISTRY = {"FusedLAMB": Lamb, "Adam": AdamW, "SGD": torch.optim.SGD}
