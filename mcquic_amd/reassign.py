"""Codebook reassignment inside the training step (csrc/vq_reassign.hip): the reference trainer's one hook, `CodebookReassign(freq)`
(mcquic/train/hooks.py:100-121; `freq: 20000` in configs/a800_8.yaml and configs/neon.yaml).  Every `freq` steps the reference calls
`Compound.refresh`: dead codewords (normalised frequency < 1e-6) are overwritten by the most used ones on rank 0 and `syncCodebook`
broadcasts the result.  Here the whole of it is two launches that take the step's device-side decision words, so it runs inside
`parallel.GraphedTrainStep`'s post graph (`reassign=`) with no host in between, obeys the step's non-finite guard, and needs no
broadcast: every rank holds the same all-reduced frequencies and draws the same priorities.  HIP device only: there is no CPU path
(the eager `reAssignCodebook` of the quantizer modules is unchanged and remains the CPU form)."""
from __future__ import annotations

import torch

from . import _lib, ops

__all__ = ["CodebookReassign"]

_COUNT, _SEEN, _FIRED, _MOVED, _PROPORTION, _SEED, _OFFSET = range(ops.REASSIGN_STATE_WORDS)


class CodebookReassign:
    """`CodebookReassign(model, freq, seed=0, start=0)`: the reference's hook name and its `freq` argument.

        reassign = CodebookReassign(model, freq=20000)
        step = GraphedTrainStep(model, optimizer, x, reassign=reassign)      # two more launches in the post graph
        reassign.step(skip=None)                                             # ... or eagerly, after the frequency EMA of an update
        reassign.read()["Stat/ReAssignProportion"]                           # one host copy

    `step()` is one completed update.  The step fires when the completed count s AFTER this update satisfies s >= start and
    (s + 1) % freq == 0 -- NOT s % freq: the reference increments `_step` and then tests (step + 1) % freq (trainer.py:211-213,
    hooks.py:107), so with freq = 20000 the first reassignment follows update 19 999; that off-by-one is kept.  On a firing step, for every
    level and group, by the rule of `_multiCodebookQuantization.reAssignCodebook` (one arithmetic, `ops.vq_reassign_plan`): the i-th
    refilled dead codeword in index order takes the i-th most used codeword; a group with more than k // 2 dead codewords refills the
    k // 2 of lowest priority.  The frequencies consulted are the RAW `_freqEMA` rows as the update's frequency EMA left them, normalised by
    a row sum formed in double in a fixed order and rounded once to float32; `NormalizedFreq`'s ATen sum can differ from it in the last
    place, which matters only for a codeword within one rounding of 1e-6.  On any other step the two launches read the decision and
    return; with `skip` (a step's guard flag, `guard.StepGuard.skip`) set on the device nothing moves and the count does not advance, as
    for the scheduler.

    The priorities come from a generator state of this object's own ({seed, offset} on the device, as `data.transforms.TrainingInput`
    keeps one): NOT the process generator, which ranks seed differently.  Level l of the n-th firing step draws
    `ops.hash_uniform({seed, offset + l}, ops.REASSIGN_STREAM, (m, k_l))`, and the offset advances by the level count on a firing step
    only.  Equal seeds, equal frequencies (the all-reduced counts) and equal codebooks give equal moves on every rank, so no broadcast
    and no barrier is added; under an initialised process group the constructor takes rank 0's `seed`.

    Device scalars (0-dim views of one int64 record): `count`, `fired`, `moved` (codewords that moved by more than 1e-4 in squared
    distance on the last firing step), `proportion` (float32: moved / all codewords, the reference's return value).  `read()` is one
    device-to-host copy of the record.

    Left as they are, as in the reference: the optimizer's moments and the EMA shadow of a moved codeword, and `_freqEMA` (a refilled
    codeword stays "dead" in the table until it is used; with freq = 20000 the EMA of 0.998 has long forgotten by the next firing step).
    After a move the packed-codebook cache of every touched quantizer is dropped and the Parameters' version counters are bumped, so eager
    `encode` follows the new codebook; a captured step re-packs its codebooks at the head of every replay anyway.  Only `UMGMQuantizer`
    (`Compressor`) is supported."""

    def __init__(self, model, freq: int, seed: int = 0, start: int = 0):
        from .modules.quantizer import UMGMQuantizer
        quantizer = getattr(model, "_quantizer", None)
        if not isinstance(quantizer, UMGMQuantizer):
            raise NotImplementedError(f"CodebookReassign refills the per-level codebooks of a UMGMQuantizer (Compressor); "
                                      f"{type(quantizer).__name__} keeps its codebook / frequency pairs elsewhere and is out of scope")
        if not isinstance(freq, int) or isinstance(freq, bool) or freq < 1:
            raise ValueError(f"CodebookReassign: freq must be an int >= 1 (updates between reassignments), got {freq!r}")
        if not isinstance(start, int) or isinstance(start, bool) or start < 0:
            raise ValueError(f"CodebookReassign: start must be an int >= 0 (no reassignment below that many updates), got {start!r}")
        self.freq, self.start = freq, start
        self._quantizers = [encoder._quantizer for encoder in quantizer._encoders]
        self._coder = quantizer._entropyCoder
        self.codebooks = [q._codebook for q in self._quantizers]
        self.freqs = list(self._coder._freqEMA)
        if len(self.freqs) != len(self.codebooks) or any(tuple(f.shape) != tuple(c.shape[:2]) for f, c in zip(self.freqs, self.codebooks)):
            raise NotImplementedError("CodebookReassign: the quantizer's levels do not pair one [m, k, d] codebook with one [m, k] `_freqEMA`")
        dev = self.codebooks[0].device
        for t in self.codebooks + self.freqs:
            if not t.is_cuda or t.device != dev:
                raise RuntimeError(f"mcquic_amd: CodebookReassign needs the model on one HIP device (got {t.device}); the HIP kernels have "
                                   "no CPU fallback")
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise TypeError("mcquic_amd: CodebookReassign needs contiguous float32 codebooks and frequency tables")
        kmax = int(_lib.load().mcq_vq_reassign_max_k())
        if max(int(c.shape[1]) for c in self.codebooks) > kmax:
            raise ValueError(f"CodebookReassign: a codebook of {max(int(c.shape[1]) for c in self.codebooks)} codewords per group does not "
                             f"fit the plan kernel's LDS arrays (at most {kmax})")
        seed = self._agreed_seed(int(seed), dev)
        # ONE record, so that read() is one copy (include/mcquic_hip.h: count, seen, fired, moved, proportion, seed, offset)
        words = [0] * ops.REASSIGN_STATE_WORDS
        words[_SEED] = seed & 0x7fffffffffffffff
        self._state = torch.tensor(words, dtype=torch.int64).to(dev)
        self.count, self.fired, self.moved = self._state[_COUNT], self._state[_FIRED], self._state[_MOVED]
        self.proportion = self._state.view(torch.float32)[2 * _PROPORTION]
        self.rng_state = self._state[_SEED: _OFFSET + 1]                 # {seed, offset}: what `ops.hash_uniform` takes (+ the level)
        shapes = [tuple(f.shape) for f in self.freqs]
        self.source = [torch.zeros(s, dtype=torch.int32, device=dev) for s in shapes]
        self.refill = [torch.zeros(s, dtype=torch.bool, device=dev) for s in shapes]
        self.changed = [torch.zeros(s, dtype=torch.bool, device=dev) for s in shapes]
        self._scratch = torch.zeros(ops.vq_reassign_scratch_floats(self.codebooks), dtype=torch.float32, device=dev)

    device = property(lambda self: self._state.device)

    @staticmethod
    def _agreed_seed(seed: int, dev) -> int:
        """Rank 0's seed under an initialised process group (all ranks must draw the same priorities); the caller's otherwise."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
            return seed
        from .parallel import _staged
        word = torch.tensor([seed], dtype=torch.int64, device=dev)
        buf = _staged(word)
        dist.broadcast(buf, 0)
        return int(buf[0])

    # ---- one step ------------------------------------------------------------------------------------------------------------
    def prepare(self) -> None:
        """Nothing to build: the buffers exist since the constructor (`parallel.GraphedTrainStep` calls it before it captures)."""

    @torch.no_grad()
    def step(self, skip=None) -> None:
        """One completed update: the two launches (capturable).  `skip`: the step's guard flag (one int32 on the device) or None."""
        ops.vq_reassign_plan(self.freqs, self._state, self.freq, self.start, skip=skip, source=self.source, refill=self.refill)
        ops.vq_reassign_apply(self.codebooks, self.source, self.refill, self._state, self.freq, self.start, skip=skip,
                              changed=self.changed, scratch=self._scratch)
        self._moved()

    def _moved(self) -> None:
        """What `_store` does for the eager method, without a launch: whether the step fired is known on the device only, so the host
        side treats every step as one that may have moved a codeword."""
        for q, cb in zip(self._quantizers, self.codebooks):
            q._cache[0].invalidate()
            torch.autograd.graph.increment_version(cb)

    @torch.no_grad()
    def warm(self) -> None:
        """One throw-away step, so that the kernels' first launch happens outside any capture, under a flag that is SET: a skipped
        launch writes nothing, so the count, the generator state, the scalars and the codebooks keep their bits."""
        flag = torch.ones(1, dtype=torch.int32, device=self.device)
        self.step(skip=flag)
        torch.cuda.synchronize(self.device)

    # ---- the host side ---------------------------------------------------------------------------------------------------------
    def read(self) -> dict:
        """One device-to-host copy of the record: `count`, `fired`, `moved`, `Stat/ReAssignProportion` (of the last firing step; 0.0
        before the first), `seed`, `offset`."""
        host = self._state.cpu()
        return {"count": int(host[_COUNT]), "fired": int(host[_FIRED]), "moved": int(host[_MOVED]),
                "Stat/ReAssignProportion": float(host.view(torch.float32)[2 * _PROPORTION]), "seed": int(host[_SEED]), "offset": int(host[_OFFSET])}

    def state_dict(self) -> dict:
        """The record -- count, generator state and scalars (a device copy: nothing is read back) -- and the two constructor arguments
        the decision depends on."""
        return {"state": self._state.clone(), "freq": self.freq, "start": self.start}

    @torch.no_grad()
    def load_state_dict(self, sd) -> None:
        """Into the record this object already has (the address a captured step holds): a resumed run fires on the same steps and draws
        the same priorities."""
        if int(sd["freq"]) != self.freq or int(sd["start"]) != self.start:
            raise ValueError(f"CodebookReassign: the checkpoint was written with freq={sd['freq']}, start={sd['start']}; this object was "
                             f"built with freq={self.freq}, start={self.start} (a captured step has them recorded)")
        state = torch.as_tensor(sd["state"])
        if state.dtype != torch.int64 or state.numel() != ops.REASSIGN_STATE_WORDS:
            raise ValueError(f"CodebookReassign: `state` must be int64 [{ops.REASSIGN_STATE_WORDS}]")
        self._state.copy_(state.to(self.device))
