"""Training telemetry that stays on the device: what the reference's trainer reports after every update
(mcquic/train/trainer.py:423-441 `_stepFinishHook`: the distortion in dB, its `EMATracker((), 0.99)` shadow, gradient norm, learning
rate, the `Loss becomes NAN. Train crashed.` guard; trainer.py:463-491 `log`: `CodeUsage` and the per-level code statistics), recorded as
one float32 row per step in a ring buffer by two HIP launches (csrc/step_meter.hip) that read every value through a device pointer.
The host copies the buffer back when it likes, with one copy; nothing else here synchronises, so the launches sit in the captured
post graph of `parallel.GraphedTrainStep(..., meter=...)` and a replay stays free of host reads.

`StepSnapshot` is the periodic payload of that `log` (the LogDistance histogram, the frequency and code-map pictures, the batch and its
reconstruction as images), made by the kernels of csrc/step_snapshot.hip into one buffer when the host asks for it.

`ParamStats` is what neither says: per parameter tensor, the norms of weights, gradient and update and the count of non-finite gradient
elements (csrc/param_stats.hip), recorded around the optimizer's update of `parallel.GraphedTrainStep(..., stats=...)`.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch

from . import _lib, ops
from .ops import _guard, _stream, check

HEAD = ("loss", "db", "db_ema", "grad_norm", "lr", "skipped", "code_usage", "bpp")
PER_LEVEL = ("usage", "ema_entropy", "hit", "step_entropy")
_STATE = 4                                                    # int64 words in front of `steps`: count, first_bad_step, shadow, reserved


class StepMeter:
    """One row per training step, kept on the device:

        meter = StepMeter(model, capacity=1024, pixels=n * H * W, upper_bound=1.0, momentum=0.99, floor=0.1)
        step = parallel.GraphedTrainStep(model, opt, example_x, ..., meter=meter)       # or, by hand: meter.update(loss, counts, ...)
        rows = meter.read()          # ONE device-to-host copy: the rows recorded since the last read(), as numpy arrays
        meter.check()                # raises `Loss becomes NAN. Train crashed.` once the watchdog has tripped (reads one word)

    `model`: anything whose modules include the entropy coder(s) (`EntropyCoder` / `VariousMCoder`: what has `deferCounts`); their
    frequency EMAs give the levels (m_l, k_l).  Columns of a row (`read()` keys; the per-level ones are [rows, levels] arrays):

        loss, db, db_ema     the loss given to `update`, -10 log10(loss / upper_bound^2) (`Decibel`: upper_bound 1.0 for MsSSIM, 2.0 for
                             PSNR) and its EMATracker shadow with `momentum`, float32 op by op as the reference computes them
        grad_norm, lr        as given (NaN when not given);  skipped: the optimizer's skip count (0 when not given)
        code_usage           the reference's `CodeUsage` of the frequency EMA: entries with f / sum f > 1e-6 over all entries of all levels
        bpp                  `validate.ideal_bpp` of THIS step's code histograms over `pixels` (the image pixels behind `counts`: all ranks')
        usage, ema_entropy   per level: used entries / all entries; entropy of the normalised EMA rows in bits per code, mean over groups
        hit, step_entropy    per level: codewords this step used / all entries; entropy of this step's codes in bits per code

    `first_bad_step` (0-dim int64 device tensor, -1 = none) is set, and stays set, the first time the loss or the gradient norm is inf / NaN
    or the shadow is NaN or below `floor` (the reference's 0.1; None switches that test off).  The ring holds the last `capacity` rows;
    `read()` reports how many were overwritten unread as `dropped`.  HIP device and float32 only: there is no CPU path."""

    def __init__(self, model, capacity: int = 1024, pixels: int = 1, upper_bound: float = 1.0, momentum: float = 0.99,
                 floor: Optional[float] = 0.1):
        coders = [m for m in model.modules() if hasattr(m, "deferCounts")]
        if not coders:
            raise ValueError("mcquic_amd.monitor.StepMeter: the model has no entropy coder (no module with `deferCounts`)")
        self.freqs = [f for c in coders for f in c._freqEMA]
        for f in self.freqs:
            if not f.is_cuda:
                raise RuntimeError(f"mcquic_amd: the model's frequency tables must live on a HIP device (got {f.device}); "
                                   "the HIP kernels have no CPU fallback")
            if f.dtype != torch.float32:
                raise TypeError(f"mcquic_amd: the model's frequency tables must be torch.float32 (got {f.dtype})")
            if f.device != self.freqs[0].device:
                raise RuntimeError("mcquic_amd.monitor.StepMeter: the coders must live on one device")
        if capacity < 1 or not pixels > 0 or not upper_bound > 0 or not 0.0 <= momentum <= 1.0:
            raise ValueError("mcquic_amd.monitor.StepMeter: capacity >= 1, pixels > 0, upper_bound > 0 and 0 <= momentum <= 1 are required")
        self.ms, self.ks = [int(f.shape[0]) for f in self.freqs], [int(f.shape[1]) for f in self.freqs]
        self.levels = len(self.freqs)
        lib = _lib.load()
        if self.levels > int(lib.mcq_vq_max_levels()):
            raise ValueError(f"mcquic_amd.monitor.StepMeter: {self.levels} levels, the kernels' tables hold {int(lib.mcq_vq_max_levels())}")
        self.capacity, self.pixels = int(capacity), float(pixels)
        self.upper_bound, self.momentum, self.floor = float(upper_bound), float(momentum), floor
        self.columns = int(lib.mcq_step_meter_columns(self.levels))
        self.entries = sum(m * k for m, k in zip(self.ms, self.ks))
        dev = self.freqs[0].device
        # ONE buffer, so that read() is one copy: [count, first_bad_step, shadow (float32 in the low word), -] [steps] [ring]
        words = _STATE + self.capacity + (self.capacity * self.columns + 1) // 2
        self._buf = torch.zeros(words, dtype=torch.int64, device=dev)
        self._count, self.first_bad_step = self._buf[0], self._buf[1]
        self._shadow = self._buf[2:3].view(torch.float32)[0]
        self._steps = self._buf[_STATE: _STATE + self.capacity]
        self._ring = self._buf[_STATE + self.capacity:].view(torch.float32)[: self.capacity * self.columns].view(self.capacity, self.columns)
        self.first_bad_step.fill_(-1)
        self._shadow.fill_(float("nan"))
        self._last_read = 0
        self._tables = self._key = self._ws = None

    # ---- launch tables -------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def prepare(self) -> None:
        """The level tables and the workspace for the addresses the frequency tables have NOW; `parallel.GraphedTrainStep` calls it
        before it captures `update()`.  Rebuilt when a table's storage address changes (not inside a capture)."""
        key = tuple(f.data_ptr() for f in self.freqs)
        if key == self._key:
            return
        for f in self.freqs:
            if not (f.is_cuda and f.is_contiguous() and f.device == self._buf.device):
                raise RuntimeError("mcquic_amd.monitor.StepMeter: contiguous frequency tables on the meter's HIP device only (there is no CPU path)")
        if torch.cuda.is_current_stream_capturing() and self._ws is None:
            raise RuntimeError("mcquic_amd.monitor.StepMeter: call `prepare()` before capturing (the workspace cannot be allocated inside a graph)")
        n = self.levels
        ms, ks = (ctypes.c_int32 * n)(*self.ms), (ctypes.c_int32 * n)(*self.ks)
        if self._ws is None:
            nbytes = int(_lib.load().mcq_step_meter_workspace_bytes(ms, ks, n))
            if nbytes <= 0:
                raise ValueError("mcquic_amd.monitor.StepMeter: the level table is not one the kernels take")
            self._ws = torch.zeros((nbytes + 7) // 8, dtype=torch.int64, device=self._buf.device)
        self._tables = ((ctypes.c_void_p * n)(*key), ms, ks)
        self._key = key

    def partials(self) -> dict:
        """The five per-(level, group) partials of the last `update` (device views of the workspace, rows in level-then-group order)."""
        rows = sum(self.ms)
        w32 = self._ws[rows:].view(torch.int32)
        return {"total": self._ws[:rows], "used": w32[:rows], "hit": w32[rows: 2 * rows],
                "ema_entropy": w32[2 * rows: 3 * rows].view(torch.float32), "step_bits": w32[3 * rows: 4 * rows].view(torch.float32)}

    # ---- one step ------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _scalar(t, name: str, dtype, dev):
        if t is None:
            return None
        if not torch.is_tensor(t) or not t.is_cuda or t.device != dev:
            raise RuntimeError(f"mcquic_amd: `{name}` must live on the meter's HIP device; the HIP kernels have no CPU fallback")
        if t.dtype != dtype or t.numel() != 1:
            raise TypeError(f"mcquic_amd: `{name}` must be one {dtype} value (got {t.dtype}, {tuple(t.shape)})")
        return t.data_ptr()

    @torch.no_grad()
    def update(self, loss: torch.Tensor, counts: torch.Tensor, grad_norm: Optional[torch.Tensor] = None, lr=None,
               skipped: Optional[torch.Tensor] = None) -> None:
        """Record one step: two launches on the current stream, capturable after `prepare()`.  `loss`, `grad_norm`: 0-dim float32 device
        tensors; `counts`: this step's global code histograms, all levels back to back (int64, what `applyCounts` takes); `lr`: a 0-dim
        float32 device tensor (read on the device at every launch or replay) or a host number (recorded as it is now); `skipped`: 0-dim int64."""
        self.prepare()
        dev = self._buf.device
        if not (torch.is_tensor(counts) and counts.is_cuda and counts.device == dev):
            raise RuntimeError("mcquic_amd: `counts` must live on the meter's HIP device; the HIP kernels have no CPU fallback")
        if counts.dtype != torch.int64 or counts.numel() != self.entries or not counts.is_contiguous():
            raise ValueError(f"mcquic_amd.monitor.StepMeter: `counts` must be {self.entries} contiguous int64 entries (sum of m_l * k_l)")
        lr_ptr, lr_val = None, float("nan")
        if torch.is_tensor(lr) and lr.is_cuda:
            lr_ptr = self._scalar(lr, "lr", torch.float32, dev)
        elif lr is not None:
            lr_val = float(lr)
        ptrs, ms, ks = self._tables
        with _guard(dev):
            check(_lib.load().mcq_step_meter_update_f32(
                ptrs, ms, ks, self.levels, counts.data_ptr(), self._ws.data_ptr(), self._scalar(loss, "loss", torch.float32, dev),
                self._scalar(grad_norm, "grad_norm", torch.float32, dev), lr_ptr, lr_val, self._scalar(skipped, "skipped", torch.int64, dev),
                self.upper_bound, self.momentum, float("nan") if self.floor is None else float(self.floor), self.pixels,
                self._buf.data_ptr(), self._steps.data_ptr(), self._ring.data_ptr(), self.capacity, _stream()), "mcq_step_meter_update_f32")

    @torch.no_grad()
    def warm(self) -> None:
        """One throw-away update, so that the kernels' first launch happens outside any capture; count, shadow, watchdog and ring keep
        their bits."""
        self.prepare()
        dev = self._buf.device
        keep = self._buf.clone()
        self.update(torch.ones((), dtype=torch.float32, device=dev), torch.zeros(self.entries, dtype=torch.int64, device=dev))
        self._buf.copy_(keep)

    # ---- the host side ---------------------------------------------------------------------------------------------------------
    def read(self) -> dict:
        """The rows recorded since the last `read()` (at most the last `capacity`), in step order: numpy arrays keyed by column name, per-level
        columns as [rows, levels], plus `steps`; `dropped` rows were overwritten before they were read; `count` and `first_bad_step` as
        of this copy.  One device-to-host copy of the buffer (a host synchronisation: call it when you want to look, not every step)."""
        host = self._buf.cpu().numpy()
        count, bad = int(host[0]), int(host[1])
        first = max(self._last_read, count - self.capacity)
        dropped = max(0, first - self._last_read)
        slots = np.arange(first, max(first, count)) % self.capacity
        ring = host[_STATE + self.capacity:].view(np.float32)[: self.capacity * self.columns].reshape(self.capacity, self.columns)[slots]
        out = {"steps": host[_STATE: _STATE + self.capacity][slots].copy(), "dropped": dropped, "count": count, "first_bad_step": bad}
        for i, name in enumerate(HEAD):
            out[name] = ring[:, i].copy()
        per = ring[:, len(HEAD):].reshape(len(slots), self.levels, len(PER_LEVEL))
        for i, name in enumerate(PER_LEVEL):
            out[name] = per[:, :, i].copy()
        self._last_read = max(self._last_read, count)
        return out

    def check(self) -> None:
        """Raise as the reference's trainer does (trainer.py:435-437) if the watchdog has tripped (reads `first_bad_step` back)."""
        bad = int(self.first_bad_step)
        if bad >= 0:
            raise RuntimeError(f"Loss becomes NAN. Train crashed. (first bad step: {bad})")

    def state_dict(self) -> dict:
        """Count, shadow, watchdog, ring and step numbers (device copies: nothing is read back), and the host's read position."""
        return {"count": self._count.clone(), "shadow": self._shadow.clone(), "first_bad_step": self.first_bad_step.clone(),
                "ring": self._ring.clone(), "steps": self._steps.clone(), "last_read": self._last_read}

    @torch.no_grad()
    def load_state_dict(self, sd) -> None:
        """Into the buffer this meter already has (the addresses a captured `update` holds): a resumed run continues its numbering."""
        if tuple(sd["ring"].shape) != tuple(self._ring.shape):
            raise RuntimeError(f"mcquic_amd.monitor.StepMeter: the checkpoint's ring is {tuple(sd['ring'].shape)}, this meter's "
                               f"{tuple(self._ring.shape)} (capacity, 8 + 4 levels)")
        dev = self._buf.device
        self._count.copy_(sd["count"].to(dev, torch.int64))
        self._shadow.copy_(sd["shadow"].to(dev, torch.float32))
        self.first_bad_step.copy_(sd["first_bad_step"].to(dev, torch.int64))
        self._ring.copy_(sd["ring"].to(dev, torch.float32))
        self._steps.copy_(sd["steps"].to(dev, torch.int64))
        self._last_read = int(sd.get("last_read", 0))


class StepSnapshot:
    """The reference trainer's periodic log payload (`MainTrainer.log`, mcquic/train/trainer.py:463-491) made on the device and read with
    one copy, where the reference moves the whole level-0 slab of logits to the host and bins it there:

        snap = StepSnapshot(model, batch_shape=(n, 3, H, W), bins=64, images=4)
        snap.prepare()                                  # tables + ONE device buffer; nothing is allocated afterwards
        snap.capture(images, restored, codes, logits)   # launches only, on the current stream, capturable; no host read
        payload = snap.read()                           # ONE device-to-host copy

    or, behind a `parallel.GraphedTrainStep(..., keep_outputs=True)`: `payload = step.snapshot(snap)`.  `read()` keys are the reference's
    wandb keys (there is no wandb import here: wrap them yourself):

        Hist/LogDistance     (counts int64 [bins], edges float64 [bins + 1]) of log10(clamp(-logits[0][0, 0], 1e-6)) in np.histogram's
                             form (`wandb.Histogram(np_histogram=...)`): level 0, image 0, group 0.  Non-finite values are left out and
                             counted: `snap.stats` = (finite, non-finite) of the last read.  The edges and the bin index are numpy's
                             evaluated in float64 (numpy >= 2 keeps float32 edges for a float32 array)
        Hist/FreqLvNN        (group 0 of the level's normalised frequency EMA float32 [k], np.arange(0.5, k + 1.5)), as the reference pairs them
        Hist/CodeLvNN        uint8 [images, 1, 4h, 4w]: `Validator.visualizeIntermediate` of the level's codes (group 0, scaled by the maximum of
                             the WHOLE batch's codes, enlarged 4x); an all-zero code tensor gives 0
        Train/Raw, Train/Res uint8 [images, 3, H, W]: `ops.detransform` of the batch and of its reconstruction
        Stat/CodeUsage       float: `Compressor.CodeUsage` of the frequency EMA

    `images`: only the first `images` images of the batch are kept (None, or more than the batch has: all, as the reference logs them).  `code_shapes`: (h, w) of every
    level's code map, in the order of the model's `codes`; by default the 16x stem and a halving per level, (H / 16 >> l, W / 16 >> l).
    HIP device and float32 only: there is no CPU path.  Inside a captured graph the kernels' first launch must have happened before:
    run one eager `capture` first."""

    EPS = 1e-6                                                # Consts.Eps

    def __init__(self, model, batch_shape, bins: int = 64, images: Optional[int] = 4, code_shapes=None):
        coders = [m for m in model.modules() if hasattr(m, "deferCounts")]
        if not coders:
            raise ValueError("mcquic_amd.monitor.StepSnapshot: the model has no entropy coder (no module with `deferCounts`)")
        self.freqs = [f for c in coders for f in c._freqEMA]
        for f in self.freqs:
            if not f.is_cuda:
                raise RuntimeError(f"mcquic_amd: the model's frequency tables must live on a HIP device (got {f.device}); "
                                   "the HIP kernels have no CPU fallback")
            if f.dtype != torch.float32:
                raise TypeError(f"mcquic_amd: the model's frequency tables must be torch.float32 (got {f.dtype})")
            if f.device != self.freqs[0].device:
                raise RuntimeError("mcquic_amd.monitor.StepSnapshot: the coders must live on one device")
        if len(batch_shape) != 4 or int(batch_shape[1]) != 3 or min(int(s) for s in batch_shape) < 1:
            raise ValueError(f"mcquic_amd.monitor.StepSnapshot: batch_shape (n, 3, H, W) is required (got {tuple(batch_shape)})")
        self.batch_shape = tuple(int(s) for s in batch_shape)
        n, _, H, W = self.batch_shape
        self.keep = n if images is None else min(int(images), n)
        if self.keep < 1 or not 1 <= int(bins) <= ops.HIST_MAX_BINS:
            raise ValueError(f"mcquic_amd.monitor.StepSnapshot: images >= 1 and 1 <= bins <= {ops.HIST_MAX_BINS} are required")
        self.bins = int(bins)
        self.ms, self.ks = [int(f.shape[0]) for f in self.freqs], [int(f.shape[1]) for f in self.freqs]
        self.levels = len(self.freqs)
        lib = _lib.load()
        if self.levels > int(lib.mcq_vq_max_levels()):
            raise ValueError(f"mcquic_amd.monitor.StepSnapshot: {self.levels} levels, the kernels' tables hold {int(lib.mcq_vq_max_levels())}")
        if code_shapes is None:
            code_shapes = [((H // 16) >> l, (W // 16) >> l) for l in range(self.levels)]
        self.code_shapes = [(int(h), int(w)) for h, w in code_shapes]
        if len(self.code_shapes) != self.levels or min(min(s) for s in self.code_shapes) < 1:
            raise ValueError(f"mcquic_amd.monitor.StepSnapshot: one positive (h, w) per level is required (got {self.code_shapes})")
        self.slab = self.code_shapes[0][0] * self.code_shapes[0][1] * self.ks[0]        # logits[0][0, 0]: [h, w, k]
        self.stats = None
        self._buf = self._tables = self._key = None

    # ---- the buffer: [counts] [edges] [stats] [usage] [code maxima] [freq] [code images] [raw] [res] | workspaces (not read back) ----
    def _layout(self):
        n, _, H, W = self.batch_shape
        words = lambda nbytes: (int(nbytes) + 7) // 8
        at, off = {}, 0
        for name, size in [("counts", self.bins), ("edges", self.bins + 1), ("stats", 2), ("usage", 1), ("max", self.levels),
                           ("freq", words(4 * sum(self.ks)))] + \
                          [(f"code{l}", words(self.keep * 16 * h * w)) for l, (h, w) in enumerate(self.code_shapes)] + \
                          [("raw", words(self.keep * 3 * H * W)), ("res", words(self.keep * 3 * H * W))]:
            at[name] = (off, size)
            off += size
        return at, off

    @torch.no_grad()
    def prepare(self) -> None:
        """The level tables, the buffer and the workspaces for the addresses the frequency tables have NOW.  Rebuilt when a table's
        storage address changes (not inside a capture)."""
        key = tuple(f.data_ptr() for f in self.freqs)
        if key == self._key:
            return
        for f in self.freqs:
            if not (f.is_cuda and f.is_contiguous() and f.device == self.freqs[0].device):
                raise RuntimeError("mcquic_amd.monitor.StepSnapshot: contiguous frequency tables on one HIP device only (there is no CPU path)")
        if torch.cuda.is_current_stream_capturing() and self._buf is None:
            raise RuntimeError("mcquic_amd.monitor.StepSnapshot: call `prepare()` before capturing (the buffer cannot be allocated inside a graph)")
        n = self.levels
        ms, ks = (ctypes.c_int32 * n)(*self.ms), (ctypes.c_int32 * n)(*self.ks)
        if self._buf is None:
            lib = _lib.load()
            hist_ws, freq_ws = int(lib.mcq_histogram_workspace_bytes(self.slab, self.bins)), int(lib.mcq_snapshot_freq_workspace_bytes(ms, ks, n))
            if hist_ws <= 0 or freq_ws <= 0:
                raise ValueError("mcquic_amd.monitor.StepSnapshot: the level table or the slab is not one the kernels take")
            self._at, self._payload = self._layout()
            w1, w2 = (hist_ws + 7) // 8, (freq_ws + 7) // 8
            self._buf = torch.zeros(self._payload + w1 + w2, dtype=torch.int64, device=self.freqs[0].device)
            self._hist_ws, self._freq_ws = self._buf[self._payload: self._payload + w1], self._buf[self._payload + w1:]
        self._tables = ((ctypes.c_void_p * n)(*key), ms, ks)
        self._key = key

    def _view(self, name: str) -> torch.Tensor:
        off, size = self._at[name]
        return self._buf[off: off + size]

    def _tensor(self, t, name: str, dtype, shape):
        dev = self.freqs[0].device
        if not torch.is_tensor(t) or not t.is_cuda or t.device != dev:
            raise RuntimeError(f"mcquic_amd: `{name}` must live on the snapshot's HIP device; the HIP kernels have no CPU fallback")
        if t.dtype != dtype:
            raise TypeError(f"mcquic_amd: `{name}` must be {dtype} (got {t.dtype})")
        if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise ValueError(f"mcquic_amd.monitor.StepSnapshot: `{name}` must be contiguous {tuple(shape)} (got {tuple(t.shape)})")
        return t

    # ---- one snapshot ----------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def capture(self, images: torch.Tensor, restored: torch.Tensor, codes, logits) -> None:
        """Make the payload of one step in the buffer: thirteen launches at three levels, on the current stream, nothing read by the host.
        `images`, `restored`: the batch and its reconstruction, float32 [n, 3, H, W]; `codes`: the int64 [n, m_l, h_l, w_l] code maps of
        all levels; `logits`: the levels' logits ([n, m, h, w, k] float32; only `logits[0][0, 0]` is read), or that level-0 tensor itself."""
        self.prepare()
        dev = self.freqs[0].device
        images = self._tensor(images, "images", torch.float32, self.batch_shape)
        restored = self._tensor(restored, "restored", torch.float32, self.batch_shape)
        if len(codes) != self.levels:
            raise ValueError(f"mcquic_amd.monitor.StepSnapshot: {self.levels} code levels are required (got {len(codes)})")
        codes = [self._tensor(c, f"codes[{l}]", torch.int64, (self.batch_shape[0], self.ms[l]) + self.code_shapes[l]) for l, c in enumerate(codes)]
        lg = logits if torch.is_tensor(logits) else logits[0]
        h0, w0 = self.code_shapes[0]
        lg = self._tensor(lg, "logits[0]", torch.float32, (self.batch_shape[0], self.ms[0], h0, w0, self.ks[0]))
        lib = _lib.load()
        ptrs, ms, ks = self._tables
        with _guard(dev):
            stream = _stream()
            check(lib.mcq_histogram_f32(lg.data_ptr(), self.slab, ops.HIST_LOG_DISTANCE, self.EPS, self.bins, self._view("counts").data_ptr(),
                                        self._view("edges").data_ptr(), self._view("stats").data_ptr(), self._hist_ws.data_ptr(), stream),
                  "mcq_histogram_f32")
            check(lib.mcq_snapshot_freq_f32(ptrs, ms, ks, self.levels, self._view("freq").data_ptr(), self._view("usage").data_ptr(),
                                            self._freq_ws.data_ptr(), stream), "mcq_snapshot_freq_f32")
        for l, c in enumerate(codes):
            ops.code_image(c, keep=self.keep, out=self._view(f"code{l}").view(torch.uint8)[: self.keep * 16 * c.shape[2] * c.shape[3]],
                           maxbuf=self._view("max")[l: l + 1])
        pixels = self.keep * 3 * self.batch_shape[2] * self.batch_shape[3]
        ops.detransform(images[: self.keep], out=self._view("raw").view(torch.uint8)[:pixels])
        ops.detransform(restored[: self.keep], out=self._view("res").view(torch.uint8)[:pixels])

    def read(self) -> dict:
        """The payload of the last `capture`, keyed as the reference's `wandb.log` payload.  One device-to-host copy of the buffer (a host
        synchronisation: call it when you want to look)."""
        if self._buf is None:
            raise RuntimeError("mcquic_amd.monitor.StepSnapshot: nothing was captured yet (`prepare()`, then `capture(...)`)")
        host = self._buf[: self._payload].cpu().numpy()
        part = lambda name: host[self._at[name][0]: self._at[name][0] + self._at[name][1]]
        _, _, H, W = self.batch_shape
        self.stats = tuple(int(v) for v in part("stats"))
        out = {"Hist/LogDistance": (part("counts").copy(), part("edges").view(np.float64).copy())}
        freq, off = part("freq").view(np.float32), 0
        for l, (k, (h, w)) in enumerate(zip(self.ks, self.code_shapes)):
            out[f"Hist/FreqLv{l:02d}"] = (freq[off: off + k].copy(), np.arange(0.5, k + 1.5, 1.0))
            out[f"Hist/CodeLv{l:02d}"] = part(f"code{l}").view(np.uint8)[: self.keep * 16 * h * w].reshape(self.keep, 1, 4 * h, 4 * w).copy()
            off += k
        for name, key in (("raw", "Train/Raw"), ("res", "Train/Res")):
            out[key] = part(name).view(np.uint8)[: self.keep * 3 * H * W].reshape(self.keep, 3, H, W).copy()
        out["Stat/CodeUsage"] = float(part("usage").view(np.float32)[0])
        return out


STAT_COLUMNS = ("weight_norm", "grad_norm", "grad_absmax", "grad_nonfinite", "update_norm")


class ParamStats:
    """Per-parameter gradient, weight and update norms of every step that is looked at, kept on the device (csrc/param_stats.hip):

        stats = ParamStats(model, capacity=64, every=1, updates=True)       # trainable parameters, in model.named_parameters() order
        step = parallel.GraphedTrainStep(model, opt, example_x, ..., stats=stats)
        rows = stats.read()          # ONE device-to-host copy: the rows recorded since the last read(), as numpy arrays
        stats.blame()                # None, or (step, parameter name): the first recorded non-finite gradient (reads two words)
        # by hand, in an eager loop: stats.before(); opt.step(); stats.after(skip=None)

    `model`: an nn.Module (its parameters with `requires_grad`), or an iterable of tensors (named "0", "1", ...); a tensor's gradient is
    its `.grad` at the time of the call (None: a gradient of zeros).  One recorded row holds five float32 columns per tensor t, every
    reduction over the whole tensor, sums of squares formed in double and rounded once (`read()` keys, [rows, T] arrays):

        weight_norm      ||w||_2 after the update (the weights as `after()` finds them)
        grad_norm        ||g||_2 of the gradient the optimizer consumed -- averaged over ranks and micro-batches, after the step's own
                         clipping if it clips -- over the FINITE elements only
        grad_absmax      max |g| over the finite elements; 0 when there are none
        grad_nonfinite   number of inf / NaN elements of g (exact up to 2^24, as a float32)
        update_norm      ||w_after - w_before||_2: `before()` copies the weights into a shadow (one flat float32 buffer of the model's
                         size, allocated once in `prepare()`); NaN in every row when `updates=False` (no shadow, no `before` launch)

    plus `update_ratio` = update_norm / weight_norm, formed on the host.  Sampling is decided on the device: `count` advances on every
    `after()`; a step is recorded when count % every == 0, or when `skip` (a guard's flag) is set for it -- a skipped step always leaves a
    row; `steps` holds the count at which each row was made.  On any other step the three launches read the decision and return.  A row
    made ONLY because the step was skipped does not read the shadow (no `before` refreshed it): its update_norm is 0, as a skipped update
    moves no weight.  `first_bad_step` / `first_bad_tensor` (-1 = none) are set, and stay set, by the first recorded row in which some
    tensor has grad_nonfinite > 0: the lowest such tensor.  The ring holds the last `capacity` rows; `read()` reports how many were
    overwritten unread as `dropped`.  HIP device and float32 only: there is no CPU path."""

    def __init__(self, model, capacity: int = 64, every: int = 1, updates: bool = True):
        if isinstance(model, torch.nn.Module):
            named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        else:
            named = [(str(i), p) for i, p in enumerate(model)]
        if not named or not any(p.numel() for _, p in named):
            raise ValueError("mcquic_amd.monitor.ParamStats: nothing to watch (no trainable parameter with elements)")
        for n, p in named:
            if not p.is_cuda:
                raise RuntimeError(f"mcquic_amd: the watched parameters must live on a HIP device (got {p.device} for {n}); "
                                   "the HIP kernels have no CPU fallback")
            if p.dtype != torch.float32:
                raise TypeError(f"mcquic_amd: the watched parameters must be torch.float32 (got {p.dtype} for {n})")
            if p.device != named[0][1].device:
                raise RuntimeError("mcquic_amd.monitor.ParamStats: the parameters must live on one device")
        if capacity < 1 or every < 1:
            raise ValueError("mcquic_amd.monitor.ParamStats: capacity >= 1 and every >= 1 are required")
        self.names, self.params = [n for n, _ in named], [p for _, p in named]
        self.sizes = [p.numel() for p in self.params]
        self.capacity, self.every, self.updates = int(capacity), int(every), bool(updates)
        self.tensors, self.columns = len(self.params), int(_lib.load().mcq_param_stats_columns())
        dev = self.params[0].device
        # ONE buffer, so that read() is one copy: [count, first_bad_step, first_bad_tensor, rows] [steps] [ring]
        cells = self.capacity * self.tensors * self.columns
        self._buf = torch.zeros(_STATE + self.capacity + (cells + 1) // 2, dtype=torch.int64, device=dev)
        self._count, self.first_bad_step, self.first_bad_tensor, self._rows = self._buf[0], self._buf[1], self._buf[2], self._buf[3]
        self._steps = self._buf[_STATE: _STATE + self.capacity]
        self._ring = self._buf[_STATE + self.capacity:].view(torch.float32)[:cells].view(self.capacity, self.tensors, self.columns)
        self._buf[1:3].fill_(-1)
        self._last_read = 0
        self._table = self._ws = self._shadow = None
        self._none = torch.empty(0, dtype=torch.float32)      # (data_ptr() 0: the table entry of a parameter without a gradient)

    # ---- launch tables -------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def prepare(self) -> None:
        """The device tables for the addresses the parameters and their gradients have NOW, the workspace and (with `updates`) the
        shadow; `parallel.GraphedTrainStep` calls it before it captures.  Refilled when an address changes (not inside a capture)."""
        dev = self._buf.device
        for p in self.params:
            g = p.grad
            if not (p.is_cuda and p.is_contiguous() and p.device == dev):
                raise RuntimeError("mcquic_amd.monitor.ParamStats: contiguous parameters on the statistics' HIP device only (there is no CPU path)")
            if g is not None and not (g.is_cuda and g.is_contiguous() and g.device == dev and g.dtype == torch.float32 and g.numel() == p.numel()):
                raise RuntimeError("mcquic_amd.monitor.ParamStats: contiguous float32 gradients of the parameters' sizes on their HIP device only")
        if self._table is None:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("mcquic_amd.monitor.ParamStats: call `prepare()` before capturing (the workspace cannot be allocated inside a graph)")
            from .tensor_list import TensorList, flat_layout
            self._table = TensorList(self.sizes, dev, rows=3, moved="mcquic_amd.monitor.ParamStats: parameter or gradient addresses changed "
                                                                     "since the last call")
            nbytes = int(_lib.load().mcq_param_stats_workspace_bytes(self._table.nblocks, self.tensors))
            self._ws = torch.zeros(nbytes // 8, dtype=torch.int64, device=dev)
            shadows = None
            if self.updates:                                  # (the rows a caller owns are filled once: the shadows never move)
                offsets, total = flat_layout(self.sizes)
                self._shadow = torch.zeros(total, dtype=torch.float32, device=dev)
                shadows = [self._shadow[o: o + n] for o, n in zip(offsets, self.sizes)]
            self._table.fill(self.params, None, shadows)
        self._table.fill(self.params, [self._none if p.grad is None else p.grad for p in self.params])

    # ---- one step ------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def before(self) -> None:
        """In front of the optimizer's step: on a sampled step the weights go into the shadow (one launch, capturable after `prepare()`);
        nothing is launched with `updates=False`."""
        self.prepare()
        if not self.updates:
            return
        with _guard(self._buf.device):
            check(_lib.load().mcq_param_stats_before_f32(*self._table.args(), self._buf.data_ptr(), self.every, _stream()),
                  "mcq_param_stats_before_f32")

    @torch.no_grad()
    def after(self, skip=None) -> None:
        """Behind the optimizer's step: the row of this step, if it is recorded, and count + 1 (two launches, capturable after
        `prepare()`).  `skip`: the step's guard flag (one int32 on the device, `guard.StepGuard.skip`) or None."""
        self.prepare()
        from .guard import skip_pointer
        dev = self._buf.device
        flag = skip_pointer(skip, dev, "mcquic_amd.monitor.ParamStats.after")
        lib, t = _lib.load(), self._table
        with _guard(dev):
            check(lib.mcq_param_stats_after_f32(*t.args(), self._buf.data_ptr(), self.every, self.capacity, int(self.updates), flag,
                                                self._ws.data_ptr(), _stream()), "mcq_param_stats_after_f32")
            check(lib.mcq_param_stats_finish_f32(t.tensor_first_blk.data_ptr(), t.blk_tensor.data_ptr(), self.tensors, t.nblocks,
                                                 self._ws.data_ptr(), int(self.updates), self._buf.data_ptr(), self._steps.data_ptr(),
                                                 self._ring.data_ptr(), _stream()), "mcq_param_stats_finish_f32")

    @torch.no_grad()
    def warm(self) -> None:
        """One throw-away pass, so that the kernels' first launch happens outside any capture; count, blame words, ring and shadow keep
        their bits."""
        self.prepare()
        self._table.tensor_first_blk                          # (uploaded on first use: not inside a capture)
        keep = self._buf.clone()
        shadow = None if self._shadow is None else self._shadow.clone()
        self.before()
        self.after()
        self._buf.copy_(keep)
        if shadow is not None:
            self._shadow.copy_(shadow)

    # ---- the host side ---------------------------------------------------------------------------------------------------------
    def read(self) -> dict:
        """The rows recorded since the last `read()` (at most the last `capacity`), in step order: `steps` [rows], `names`, one [rows, T]
        numpy array per column, `update_ratio`; `dropped` rows were overwritten before they were read; `count`, `first_bad_step` and
        `first_bad_tensor` as of this copy.  One device-to-host copy of the buffer (a host synchronisation: call it when you want to look)."""
        host = self._buf.cpu().numpy()
        count, bad_step, bad_tensor, made = (int(v) for v in host[:_STATE])
        first = max(self._last_read, made - self.capacity)
        dropped = max(0, first - self._last_read)
        slots = np.arange(first, max(first, made)) % self.capacity
        cells = self.capacity * self.tensors * self.columns
        ring = host[_STATE + self.capacity:].view(np.float32)[:cells].reshape(self.capacity, self.tensors, self.columns)[slots]
        out = {"steps": host[_STATE: _STATE + self.capacity][slots].copy(), "names": list(self.names), "dropped": dropped, "count": count,
               "first_bad_step": bad_step, "first_bad_tensor": bad_tensor}
        for i, name in enumerate(STAT_COLUMNS):
            out[name] = ring[:, :, i].copy()
        with np.errstate(divide="ignore", invalid="ignore"):
            out["update_ratio"] = out["update_norm"] / out["weight_norm"]
        self._last_read = max(self._last_read, made)
        return out

    def blame(self):
        """None, or (step, parameter name) of the first recorded non-finite gradient (reads the two blame words back)."""
        step, tensor = (int(v) for v in self._buf[1:3].cpu())
        return None if step < 0 else (step, self.names[tensor])

    def state_dict(self) -> dict:
        """Count, rows, blame words, ring and step numbers (device copies: nothing is read back), and the host's read position.  The shadow
        is not part of it: every sampled step rewrites it."""
        return {"count": self._count.clone(), "rows": self._rows.clone(), "first_bad_step": self.first_bad_step.clone(),
                "first_bad_tensor": self.first_bad_tensor.clone(), "ring": self._ring.clone(), "steps": self._steps.clone(),
                "last_read": self._last_read}

    @torch.no_grad()
    def load_state_dict(self, sd) -> None:
        """Into the buffer this object already has (the addresses a captured step holds): a resumed run continues its numbering."""
        if tuple(sd["ring"].shape) != tuple(self._ring.shape):
            raise RuntimeError(f"mcquic_amd.monitor.ParamStats: the checkpoint's ring is {tuple(sd['ring'].shape)}, this object's "
                               f"{tuple(self._ring.shape)} (capacity, tensors, 5)")
        dev = self._buf.device
        for name, word in (("count", self._count), ("rows", self._rows), ("first_bad_step", self.first_bad_step),
                           ("first_bad_tensor", self.first_bad_tensor), ("steps", self._steps)):
            word.copy_(sd[name].to(dev, torch.int64))
        self._ring.copy_(sd["ring"].to(dev, torch.float32))
        self._last_read = int(sd.get("last_read", 0))
