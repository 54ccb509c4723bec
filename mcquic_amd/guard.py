"""The non-finite guard of a training step (csrc/step_guard.hip): ONE flag per step, decided on the device from the global norm of the
gradient, that every kernel of the update obeys -- `optim.Adam / AdamW / Lamb / SGD`, `optim.EMA.update`, the scheduler's `step`,
`ops.freq_ema_update_` and `ops.clip_by_norm_` take it as `skip=`.  The reference's only defence is the host's, after the fact
(mcquic/train/trainer.py:435-437 `Loss becomes NAN. Train crashed.`); inside captured graphs nobody reads anything between replays, and
one inf in one gradient would go through moments, parameters, weight average, frequency EMA and schedule before anyone looks.

The contract: a skipped step leaves every tensor the update owns bit for bit as it was (parameters, optimizer state and step counts, the
EMA shadow and its count, every `_freqEMA`, scheduler state and rates); only the guard's record moves.  A clean step with the guard on
produces the bits it produces with the guard off.  HIP device only: there is no CPU path."""
from __future__ import annotations

import torch

from . import _lib
from .ops import _guard, _stream, check

__all__ = ["StepGuard", "skip_pointer"]


def skip_pointer(skip, device, who: str):
    """The address an entry point's `skip` argument takes: None, or the flag tensor's (one int32 on `device`; a `StepGuard` gives its own)."""
    if skip is None:
        return None
    if isinstance(skip, StepGuard):
        skip = skip.skip
    if not (torch.is_tensor(skip) and skip.is_cuda and skip.dtype == torch.int32 and skip.numel() == 1):
        raise TypeError(f"{who}: `skip` must be one int32 on the HIP device (a StepGuard's `skip`), or None")
    if skip.device != torch.device(device):
        raise RuntimeError(f"{who}: `skip` lives on {skip.device}, the tensors it guards on {device}")
    return skip.data_ptr()


class StepGuard:
    """The device record {int32 skip; float grad_norm; int64 skipped; int64 consecutive} and the launches that fill it.

        guard = StepGuard(device)
        guard.run_flat(flat)              # G over one flat float32 buffer: per-chunk double partials, a fixed tree (two launches)
        guard.run_list(tables)            # ... over the gradients (row 1) of one or more `tensor_list.TensorList`
        guard.from_partials(p, n)         # from the partials an optimizer computed for itself (LAMB, SGD): no second pass
        guard.from_norm(t, squared=...)   # from a float32 norm / sum of squares that exists already (the step's clipping)
        guard.skip, guard.grad_norm, guard.skipped, guard.consecutive     # 0-dim device tensors, views of the record
        guard.check(max_consecutive=8)    # the ONE host read: raises `Loss becomes NAN. Train crashed.` after a run of skipped steps

    Every launch writes skip = !isfinite(G), grad_norm = G, skipped += skip, consecutive = skip ? consecutive + 1 : 0.  The sums are
    doubles in fixed orders: equal gradients give equal bits, and a finite gradient of 1e19 per element is not an overflow.  With a
    borrowed float32 value the flag is the lender's arithmetic (a float32 sum of squares that overflowed is skipped)."""

    def __init__(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("mcquic_amd.guard.StepGuard: a HIP device only (the flag is read by HIP kernels; there is no CPU path)")
        _lib.load()
        self.record = torch.zeros(3, dtype=torch.int64, device=device)
        self.skip = self.record.view(torch.int32)[0]
        self.grad_norm = self.record.view(torch.float32)[1]
        self.skipped = self.record[1]
        self.consecutive = self.record[2]
        self._partials = None

    device = property(lambda self: self.record.device)

    def _room(self, n: int) -> torch.Tensor:
        """`n` doubles of scratch for the partials (kept: a captured launch holds the address)."""
        if self._partials is None or self._partials.numel() < n:
            self._partials = torch.zeros(max(int(n), 1), dtype=torch.float64, device=self.device)
        return self._partials

    def prepare_flat(self, flat: torch.Tensor) -> None:
        """Allocate the scratch of `run_flat(flat)` now (outside a capture)."""
        self._room(int(_lib.load().mcq_step_guard_chunks(flat.numel())))

    @torch.no_grad()
    def run_flat(self, flat: torch.Tensor) -> "StepGuard":
        if not (torch.is_tensor(flat) and flat.is_cuda and flat.dtype == torch.float32 and flat.is_contiguous() and flat.numel() > 0):
            raise TypeError("mcquic_amd.guard.StepGuard.run_flat: a non-empty contiguous float32 buffer on the HIP device")
        if flat.device != self.device:
            raise RuntimeError(f"mcquic_amd.guard.StepGuard: the gradients live on {flat.device}, the record on {self.device}")
        lib = _lib.load()
        part = self._room(int(lib.mcq_step_guard_chunks(flat.numel())))
        with _guard(self.device):
            check(lib.mcq_step_guard_flat_f32(flat.data_ptr(), flat.numel(), part.data_ptr(), self.record.data_ptr(), _stream()),
                  "mcq_step_guard_flat_f32")
        return self

    @torch.no_grad()
    def run_list(self, tables) -> "StepGuard":
        """`tables`: a `TensorList` whose row 1 holds the gradients, or a sequence of them (parameter groups: ONE norm spans them)."""
        tables = [tables] if hasattr(tables, "args") else list(tables)
        tables = [t for t in tables if t.nblocks > 0]
        if not tables:
            raise ValueError("mcquic_amd.guard.StepGuard.run_list: no gradient to look at")
        lib = _lib.load()
        total = sum(t.nblocks for t in tables)
        part = self._room(total)
        done = 0
        with _guard(self.device):
            for i, t in enumerate(tables):
                last = i == len(tables) - 1
                check(lib.mcq_step_guard_list_f32(*t.args(), part.data_ptr() + 8 * done, part.data_ptr() if last else None, total if last else 0,
                                                  self.record.data_ptr() if last else None, _stream()), "mcq_step_guard_list_f32")
                done += t.nblocks
        return self

    @torch.no_grad()
    def from_partials(self, partials: torch.Tensor, n: int) -> "StepGuard":
        if not (torch.is_tensor(partials) and partials.is_cuda and partials.dtype == torch.float64 and partials.is_contiguous()
                and 0 < n <= partials.numel() and partials.device == self.device):
            raise TypeError("mcquic_amd.guard.StepGuard.from_partials: `n` float64 partial sums on the record's device")
        with _guard(self.device):
            check(_lib.load().mcq_step_guard_partials_f32(partials.data_ptr(), int(n), self.record.data_ptr(), _stream()),
                  "mcq_step_guard_partials_f32")
        return self

    @torch.no_grad()
    def from_norm(self, value: torch.Tensor, squared: bool = False) -> "StepGuard":
        if not (torch.is_tensor(value) and value.is_cuda and value.dtype == torch.float32 and value.numel() == 1 and value.device == self.device):
            raise TypeError("mcquic_amd.guard.StepGuard.from_norm: one float32 on the record's device")
        with _guard(self.device):
            check(_lib.load().mcq_step_guard_norm_f32(value.data_ptr(), 1 if squared else 0, self.record.data_ptr(), _stream()),
                  "mcq_step_guard_norm_f32")
        return self

    def check(self, max_consecutive: int = 8) -> None:
        """The one host read (a device-to-host copy of the record): raise as the reference's trainer does (trainer.py:435-437) once
        `max_consecutive` steps IN A ROW have been skipped -- single bad batches are what the guard is there to survive."""
        if not max_consecutive >= 1:
            raise ValueError("mcquic_amd.guard.StepGuard.check: max_consecutive must be at least 1")
        _, skipped, run = self.record.tolist()
        if run >= max_consecutive:
            raise RuntimeError(f"Loss becomes NAN. Train crashed. ({run} steps in a row had a non-finite gradient; {skipped} skipped in all)")

    def state_dict(self) -> dict:
        return {"record": self.record.clone()}

    @torch.no_grad()
    def load_state_dict(self, sd) -> None:
        self.record.copy_(sd["record"].to(self.device, torch.int64))
