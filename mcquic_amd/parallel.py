"""Multi-GPU layer of the Compressor path: one process per GPU, images sharded, no data-path collective.

Every image is independent in encode / decode, so a batch is cut into contiguous per-rank
slices and each rank runs the whole model on its slice.  Collectives (RCCL over xGMI with backend "nccl", gloo
in the CPU tests) appear only where validation statistics are combined:
  * all_gather of per-image statistics rows (e.g. [psnr, ms_ssim, bits]) -- what the reference's validator
    accumulates on rank 0 only (mcquic/validate/validator.py:40-58);
  * all_reduce(sum) of per-level code histograms [m, k_l] -- what `IdealBPP` counts
    (mcquic/validate/handlers.py:110-187) and what EntropyCoder.forward all-reduces in training
    (mcquic/modules/entropyCoder.py:28-44).  The three levels travel in ONE flat buffer (86 KB for qp=2): the
    message is latency-bound, so one collective instead of three.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple

import torch
import torch.distributed as dist


def shard_range(n: int, rank: int, world: int) -> Tuple[int, int]:
    """Contiguous [start, stop) slice of `n` images for `rank`; the first n % world ranks get one extra."""
    if world <= 0 or not 0 <= rank < world:
        raise ValueError(f"bad rank/world {rank}/{world}")
    base, extra = divmod(n, world)
    start = rank * base + min(rank, extra)
    return start, start + base + (1 if rank < extra else 0)


def prefetch(batches, device: torch.device):
    """Host-resident batches -> device tensors, the copy of batch i + 1 in flight while the caller computes on batch i (what the
    reference's validator gets from a pinned DataLoader + `.to(device, non_blocking=True)`, mcquic/validate/validator.py:40-58).
    The copies run on a side stream (SDMA engines, no CU is taken from the kernels); the caller's stream waits on each batch's
    event and the tensor is tied to it with `record_stream`, so the allocator cannot hand its memory to the next copy early.
    Give PINNED host tensors -- a pageable source makes the copy synchronous.  On a CPU device: the batches as they are."""
    device = torch.device(device)
    if device.type != "cuda":
        yield from batches
        return
    side = torch.cuda.Stream(device)

    def load(host):
        with torch.cuda.stream(side):
            t = host.to(device, non_blocking=True)
            done = torch.cuda.Event()
            done.record(side)
        return t, done
    it = iter(batches)
    try:
        ahead = load(next(it))
    except StopIteration:
        return
    while ahead is not None:
        t, done = ahead
        try:
            ahead = load(next(it))                            # issued BEFORE the caller launches anything on batch i
        except StopIteration:
            ahead = None
        here = torch.cuda.current_stream(device)
        here.wait_event(done)
        t.record_stream(here)
        yield t


def _staged(t: torch.Tensor, group=None) -> torch.Tensor:
    """The tensor a collective of `group` should run on: device tensors as they are under RCCL ("nccl"); under gloo (the CPU
    tests, and the two-processes-on-one-GPU test: RCCL refuses two ranks on one device) a host copy."""
    if t.is_cuda and dist.get_backend(group) == "gloo":
        return t.cpu()
    return t


def gather_image_stats(local: torch.Tensor, group=None) -> torch.Tensor:
    """all_gather of per-image rows [n_local, f] -> [n_total, f] in rank order (ragged shards allowed)."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) == 1:
        return local
    world = dist.get_world_size(group)
    home = local.device
    local = _staged(local, group)
    counts = torch.zeros(world, dtype=torch.int64, device=local.device)
    counts[dist.get_rank(group)] = local.shape[0]
    dist.all_reduce(counts, group=group)
    cap = int(counts.max())
    padded = torch.zeros((cap,) + tuple(local.shape[1:]), dtype=local.dtype, device=local.device)
    padded[: local.shape[0]] = local
    out = [torch.empty_like(padded) for _ in range(world)]
    dist.all_gather(out, padded, group=group)
    return torch.cat([o[: int(c)] for o, c in zip(out, counts)], 0).to(home)


def local_code_counts(codes: Sequence[torch.Tensor], ks: Sequence[int]) -> torch.Tensor:
    """This rank's per-level code counts, all levels in ONE flat int64 buffer (level l: m_l * k_l entries, [m, k] row-major)."""
    flat = []
    for code, k in zip(codes, ks):
        n, m = code.shape[0], code.shape[1]
        idx = code.permute(1, 0, 2, 3).reshape(m, -1) + (torch.arange(m, device=code.device) * k)[:, None]
        # scatter_add instead of torch.bincount: bincount reads its maximum back to the host (a sync, and illegal
        # inside a captured hipGraph)
        idx = idx.reshape(-1)
        flat.append(torch.zeros(m * k, dtype=torch.int64, device=code.device).scatter_add_(0, idx, torch.ones_like(idx)))
    return torch.cat(flat)


def split_code_counts(buf: torch.Tensor, ms: Sequence[int], ks: Sequence[int]) -> List[torch.Tensor]:
    """The [m_l, k_l] views of a flat count buffer (local_code_counts' layout)."""
    out, off = [], 0
    for m, k in zip(ms, ks):
        out.append(buf[off: off + m * k].reshape(m, k))
        off += m * k
    return out


def all_reduce_(buf: torch.Tensor, group=None) -> torch.Tensor:
    """In-place sum of `buf` over the ranks of `group` (RCCL on device tensors; staged through the host under gloo)."""
    if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
        staged = _staged(buf, group)
        dist.all_reduce(staged, group=group)
        if staged is not buf:
            buf.copy_(staged)
    return buf


def code_histograms(codes: Sequence[torch.Tensor], ks: Sequence[int], group=None) -> List[torch.Tensor]:
    """Per-level code counts [m, k_l] (int64) summed over all images of all ranks with ONE all_reduce."""
    buf = all_reduce_(local_code_counts(codes, ks), group)
    return split_code_counts(buf, [code.shape[1] for code in codes], ks)


def data_parallel(model: torch.nn.Module, device: torch.device, group=None, **kwargs):
    """torch DistributedDataParallel around the training-mode Compressor: gradients produced by the HIP kernels
    (mcquic_amd.autograd) are all-reduced bucket by bucket -- over RCCL / xGMI with backend "nccl" (the reference's
    `torchrun` + DDP set-up, mcquic/train/ddp.py:79-95).  Under gloo with device parameters (tests: two ranks sharing one GPU)
    nothing relies on gloo's device support: the initial state broadcast and the gradient buckets are staged through the host
    (a communication hook), buffers are constants of the layers and are not re-broadcast."""
    from torch.nn.parallel import DistributedDataParallel
    staged = kwargs.pop("stage_through_host", None)
    if staged is None:
        staged = device.type == "cuda" and dist.get_backend(group) == "gloo"
    if staged:
        with torch.no_grad():                                  # rank 0's parameters and buffers, like DDP's own init sync
            for t in list(model.parameters()) + list(model.buffers()):
                host = t.detach().cpu()
                dist.broadcast(host, dist.get_global_rank(group, 0) if group is not None else 0, group=group)
                if dist.get_rank(group) != 0:
                    t.copy_(host)
        kwargs.setdefault("init_sync", False)
        kwargs.setdefault("broadcast_buffers", False)
    ddp = DistributedDataParallel(model, device_ids=[device.index] if device.type == "cuda" else None, process_group=group, **kwargs)
    if staged:
        world = dist.get_world_size(group)

        def staged_allreduce(state, bucket):
            buf = bucket.buffer()
            host = buf.detach().cpu()
            dist.all_reduce(host, group=group)
            buf.copy_(host.div_(world))
            fut = torch.futures.Future()
            fut.set_result(buf)
            return fut
        ddp.register_comm_hook(None, staged_allreduce)
    return ddp


def _backward(loss):
    from .autograd import backward
    backward(loss)


def _default_loss(out, x):
    """The distortion term alone, mean((xHat - x)^2) (mcquic/loss/__init__.py:62), through this library's own reduction."""
    from .autograd import mse_loss
    return mse_loss(out[0], x)


_MEMSET_NODES_OK = {}


def memset_nodes_replay_correctly(device=None, refresh: bool = False) -> bool:
    """Does THIS process replay the memset nodes of a captured hipGraph correctly?  (ROCm 7.2 does not once eager blit work has
    run between replays, unless DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 was in the environment when the HIP runtime started -- see
    mcquic_amd/__init__.py.)  The check is the defect's own reproducer at small scale: a captured ATen reduction large enough for
    its two-stage path (whose semaphores are zeroed by a memset node), replayed over a changing input with 700 small eager
    reductions + device-to-host copies in between; ~0.1 s, once per process and device.  GraphedTrainStep consults it for a caller-supplied
    loss function -- the default loss and every kernel of this package are free of memset nodes either way."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.index in _MEMSET_NODES_OK and not refresh:
        return _MEMSET_NODES_OK[dev.index]
    with torch.no_grad():
        big = torch.rand(1 << 21, device=dev)
        small = [torch.ones(1000 + 37 * i, device=dev) for i in range(700)]
        side = torch.cuda.Stream(dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            big.sum()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        g = torch.cuda.CUDAGraph()
        mode = dict(capture_error_mode="thread_local") if (dist.is_available() and dist.is_initialized()) else {}
        with torch.cuda.graph(g, **mode):
            out = big.sum()
        ok = True
        for _ in range(3):
            big.add_(1.0)
            g.replay()
            sum(int(torch.isfinite(t).all()) for t in small)
            torch.cuda.synchronize(dev)
            want = float(big.sum())
            ok = ok and abs(float(out) - want) <= 1e-4 * abs(want)
    _MEMSET_NODES_OK[dev.index] = ok
    return ok


class GraphedTrainStep:
    """One rank's data-parallel training step (BASELINE configs[4]: `torchrun` + DDP in the reference, mcquic/train/ddp.py:79-95;
    its gradient exchange is overlapped with the backward pass bucket by bucket, mcquic/train/trainer.py:94,105) with the host out
    of the loop.  DDP's eager step is bound by the host here -- ~1 000 launches of ~20 us each per step, with two host cores per
    rank on an 8-GPU node -- and a step captured WITH DDP's hooks replays slower than eager (the bucket all-reduces live on RCCL's
    stream: a multi-stream graph, docs/experiments.md).  So the step is cut where the exchange is:

        segment graphs  forward + backward of the local shard on a static input, captured as `segments` hipGraphs in BACKWARD
                        order -- [forward, loss, decoder backward] -> [quantizer backward] -> [encoder backward] -- each ending
                        with the copy of its parameters' gradients into ITS slice of ONE flat float32 buffer; this rank's code
                        counts of the frequency-EMA update go into one int64 buffer (known after the forward)
        exchange        outside any graph: as soon as a segment's replay is enqueued, the all-reduce of its slice is started
                        (async on RCCL's stream, which waits for exactly that segment) while the next segment replays --
                        the slices are 21.5 / 166.3 / 14.4 MB for the qp=2 model (decoder / quantizer / encoder; 202.2 MB =
                        50 558 738 float32 gradients in all), so only the encoder's 14 MB are exchanged after the last kernel;
                        one message per segment is what a point-to-point xGMI ring wants, not 25 MB buckets
        post graph      gradients / world size, the optimizer's update, the frequency EMA from the GLOBAL counts
                        (mcquic/modules/entropyCoder.py:28-44 all-reduces them inside forward; here that collective is deferred)

    `segments=1` is the whole step as one graph followed by one all-reduce (what a single rank runs: nothing to overlap with);
    the default is 3 under a process group of more than one rank, when the model has the Compressor's three stages and the
    loss is the default one (a custom `loss_fn` sees (xHat, yHat, codes, logits) with yHat / logits as LEAVES of the decoder's
    segment: its gradients on them are carried into the quantizer's segment).
    Link time of the exchange at 8 ranks: a ring all-reduce moves 2 x 7/8 x 202 MB = 354 MB through every GPU; ~1.2 ms if RCCL
    spreads it over the seven xGMI links of a GPU (~300 GB/s bus bandwidth), ~4.6 ms on one link direction --
    5-20 % of a 22 ms step when serial, which is why it is overlapped.

    The forward of the next replay starts with the grouped re-pack of every operand stream the update made stale
    (`Conv2d.repack_stale`, in place): all parameters are marked changed before the capture so that those launches are recorded.
    The step keeps every operand stream, count sink and static buffer its graphs have addresses of alive for its own lifetime,
    so using the model eagerly in between (`invalidate()`, then evaluation / `compress`, then more steps) is safe.

        step = GraphedTrainStep(model, optimizer, example_x)        # after torch.distributed is initialised (or not at all)
        loss = step(x)                                              # x: this rank's shard, shape of example_x
        step.invalidate(); model.eval(); ...; model.train()         # evaluating in between: eager code re-packs its streams
        step.close()                                                # done: the step cannot be replayed any more

    Under more than one rank the constructor broadcasts rank 0's parameters and buffers (as DDP does), so the replicas start
    equal.  An optimizer that already holds state (resumed from a checkpoint) keeps it: its tensors are restored after the
    throw-away update that brings missing state into existence.
    A captured update bakes in whatever the optimizer read on the host at capture time: pass `scheduler=` (below), or give a scheduled
    learning rate to the optimizer as a TENSOR (torch.optim reads it on the device then; Adam / AdamW additionally need `capturable=True`), or pass
    `capture_post=False` and the update (with the EMA) runs eagerly after the exchange -- ~15 launches, still no per-layer host work.
    `transform` (a `data.transforms.TrainingInput`, or any `utils.vision.Augment`): `example_x` and every later `x` are RAW batches
    (uint8 or float32 at source size); the transform's two launches are captured at the head of the first segment and write the
    model's input, which is also the `x` that `loss_fn` sees.  Each replay draws fresh decisions on the device
    (`transform.last_params` is the table of the last step); the generator's {seed, offset} is in `transform.state_dict()`.
    `max_grad_norm` clips the averaged gradient by its global norm in front of the update (the reference's step does,
    mcquic/train/trainer.py:280; torch.nn.utils.clip_grad_norm_'s arithmetic over the flat buffer, on the device); the norm before
    clipping is `step.grad_norm` (a 0-dim device tensor, valid after each call).  An optimizer that clips by itself
    (`mcquic_amd.optim.SGD(max_grad_norm=...)`: its `grad_norm()`) goes with `max_grad_norm=None` here; setting both is refused.
    `ema` (a `mcquic_amd.optim.EMA` of this model): `ema.update()` follows the optimizer's update, inside the post graph when that
    is captured (two more launches; the update count and the decay's warm-up advance on the device with every replay).  The
    constructor leaves the averages and the count bit for bit as they were, as it leaves optimizer state.  To evaluate under the
    average between steps: `with ema.applied(): model.eval(); ...` -- the swap marks the parameters changed by itself, and a call
    of the step while the average is swapped in raises.
    `meter` (a `mcquic_amd.monitor.StepMeter` of this model): `meter.update(...)` is the LAST thing of the update, after the frequency
    EMA (its EMA columns describe the table the next `compress` would use), inside the post graph when that is captured (two more
    launches).  It records `self.loss` -- this rank's LOCAL loss: no collective is added for a global one --, the global code counts,
    the gradient norm before clipping (the step's, or the optimizer's own where it computes one: `optim.Lamb`, `optim.SGD` with `max_grad_norm` or `skip_nonfinite`), the first parameter group's learning rate (read
    on the device at every replay when it is a device tensor, as it is now when it is a host number) and the optimizer's `skipped`
    count where it has one.  The constructor leaves the meter's count, shadow and ring bit for bit as they were.  Without a meter
    not one launch changes.
    `stats` (a `mcquic_amd.monitor.ParamStats` of this model): per-parameter weight, gradient and update norms and the count of non-finite
    gradient elements, recorded on the device -- `stats.before()` directly in front of the optimizer's step (the clip, if any, has run: the
    gradient is the one the optimizer consumes), `stats.after(skip=flag)` directly behind it and before the EMA, inside the post graph when
    that is captured (three launches; on a step its `every` does not sample they read the decision and return).  With `skip_nonfinite` a
    skipped step always leaves a row, so `stats.blame()` names the tensor the guard cannot.  It only reads: parameters and every other state
    keep the bits they have without it; the constructor leaves its count, blame words, ring and shadow as they were.  Works with every
    optimizer the step accepts.  Without it not one launch changes.
    `reassign` (a `mcquic_amd.CodebookReassign` of this model; the reference's one training hook, mcquic/train/hooks.py:100-121):
    `reassign.step(skip=flag)` follows the frequency EMA -- the reference's forward updates the EMA and its hook runs at step finish, so
    the NEW frequencies are the ones consulted -- and precedes the scheduler and the meter, inside the post graph when that is captured:
    two more launches, which on a step that does not fire read the decision words and return.  On a firing step (the completed count s
    with (s + 1) % freq == 0) the dead codewords of every level are overwritten by the most used ones, in place; the re-pack at the head
    of the next replay packs the moved codebooks like any other update's (the packed copy and the clone its backward reads are made
    there: no other cached operand of a codebook outlives a replay), and `invalidate()` covers eager use as it does for the optimizer's
    update.  A step the guard skips neither fires nor counts.  Under more than one rank nothing is exchanged for it: the ranks hold the
    same frequencies (the all-reduced counts), the same codebooks and the same generator state, so they make the same moves.  With
    `accumulate=k` one call is one update and one count.  The constructor leaves the object's count, generator state and scalars bit for
    bit as they were (its warm-up launches run under a set flag: nothing fires, no draw is consumed).  Without it not one launch or
    buffer changes.
    `scheduler` (a `mcquic_amd.schedule` scheduler of this optimizer): `scheduler.step()` follows the optimizer, the EMA and the frequency
    EMA and precedes the meter -- the reference steps its scheduler after every batch and logs `get_last_lr()` afterwards
    (mcquic/train/trainer.py `_stepFinish`) --, inside the post graph when that is captured: one more launch of one workgroup that
    advances the schedule's state on the device and stores the next rate into the tensors the optimizer's kernel reads, so replays
    follow the schedule with no host work in between.  The constructor leaves the schedule's state and the rates bit for bit as they
    were.  Without a scheduler not one launch changes.
    `skip_nonfinite=True`: ONE device-side guard for the whole update (`mcquic_amd.guard.StepGuard`, csrc/step_guard.hip), exposed as
    `step.guard` (`skip`, `skipped`, `consecutive`, `grad_norm`: 0-dim device tensors).  The update starts with it, after `/ world` and
    before clipping: the global norm G of the gradient decides skip = !isfinite(G), and EVERY later launch of the update takes the flag --
    the clip (the factor of a skipped step is never applied), the optimizer (`mcquic_amd.optim.Adam / AdamW / Lamb / SGD`; any other
    optimizer is refused: it could not obey), the EMA, the frequency EMA and the scheduler.  A skipped step leaves every tensor the update
    owns bit for bit as it was: parameters, optimizer state and step counts, the EMA shadow and its count, every `_freqEMA`, scheduler
    state and rates; only the guard's record and the meter's row change (its `skipped` column is the guard's count; `step.grad_norm` is
    the guard's norm).  A clean step produces the bits it produces with the guard off.  No second reduction is launched where a norm of
    the same gradient exists: with `max_grad_norm` the guard takes the clip's sum of squares by pointer (one launch of one lane; the flag
    is then float32's -- a finite gradient whose SQUARES overflow float32 is skipped rather than scaled to zero), Lamb and SGD with
    `max_grad_norm` lend the partials of their own norm; otherwise the guard reduces the flat buffer itself (double partials per chunk,
    a fixed tree: a finite gradient of 1e19 per element is not skipped).  The flag is computed from the ALL-REDUCED gradient only, never
    from the rank-local loss: a NaN or inf on any rank survives the sum, every rank sees the same buffer and so every rank decides alike;
    a flag from the local loss would let the replicas diverge.  `step.guard.check(max_consecutive=...)` is the one host read: it raises
    the reference's `Loss becomes NAN. Train crashed.` once that many steps IN A ROW were skipped.  Setting it beside an optimizer's own
    `skip_nonfinite` is refused, as `max_grad_norm` is.  With `skip_nonfinite=False` not one launch changes.

    `keep_outputs=True` keeps references to the reconstruction, the codes and the level-0 logits of the captured forward pass (`step.outputs`;
    the graph's pool is larger by the logits, no launch is added), so that `step.snapshot(snap)` can make the reference trainer's periodic log
    payload (`monitor.StepSnapshot`) of the last replay whenever the host wants one, outside the graphs.
    `accumulate=k` (an int >= 1, `step.accumulate`): gradient accumulation -- one call consumes k micro-batches and makes ONE update, so the
    reference's effective batch (`batchSize` x its 8+ GPUs, which `totalStep` and the schedules are written for) is reached on fewer GPUs
    without a larger capture.  `example_x` stays ONE micro-batch [n, ...]; `step(x)` takes [k n, ...] (raw with a `transform`), micro-batch j
    being x[j n: (j + 1) n].  The SAME segment graphs are replayed k times -- captured memory does not grow with k --: before each replay
    the host enqueues the copy of the micro-batch and of j into a device phase word (from a pinned [0 .. k-1] array; no host read, no
    synchronisation), and two launches read it: the gather into the flat buffer accumulates (`mcq_gather_accum_flat_f32`: per element, in
    float32, g0, then + g_j in order, then * float32(1 / k) inside the last micro-step -- (((g0 + g1) + ...) + g_{k-1}) * fl(1 / k)), and one
    launch at the end of the first segment (`mcq_accum_step_scalars`) adds the code counts into an int64 accumulator of the step's
    (`step.counts`: the SUM over the micro-batches, what the frequency EMA and the meter get) and forms `step.loss`, the mean of the k micro
    losses by the same rule.  Nothing is exchanged before the last micro-step: there the slices and the counts are all-reduced as ever
    (overlapped segment by segment), then `/ world` and the update ONCE -- clip, guard, optimizer, `ema`, frequency EMA, `scheduler`, `meter`
    see the accumulated, averaged gradient; a NaN of any micro-batch survives the sum, so the guard skips the whole update.  The frequency EMA
    does not move between micro-steps: all k forwards draw `_randomDrop` from the same table, as one large batch would; a `transform` draws
    fresh decisions in every replay.  `step.outputs` / `step.snapshot(snap)` describe the LAST micro-batch; the meter's `pixels` is the
    caller's and per update: k n H W.  With accumulate=1 not one launch or buffer changes (`step.counts` is the coder's sink itself).
    """

    def __init__(self, model: torch.nn.Module, optimizer, example_x: torch.Tensor, loss_fn=None, group=None,
                 forward_kwargs: dict | None = None, warmup: int = 2, capture_post: bool = True, segments: int | None = None,
                 broadcast: bool = True, max_grad_norm: float | None = None, transform=None, ema=None, meter=None, scheduler=None,
                 skip_nonfinite: bool = False, keep_outputs: bool = False, accumulate: int = 1, stats=None, reassign=None):
        self.model, self.optimizer, self.group, self.ema, self.meter, self.scheduler = model, optimizer, group, ema, meter, scheduler
        self.stats, self.reassign = stats, reassign
        self.accumulate, self.max_grad_norm, self.kwargs = accumulate, max_grad_norm, dict(forward_kwargs or {})
        self.keep_outputs, self.outputs = bool(keep_outputs), None      # (xHat, codes, level-0 logits) of the last replay, for `snapshot`
        self.world = dist.get_world_size(group) if dist.is_available() and dist.is_initialized() else 1
        self.grad_norm = None                                 # 0-dim device tensor: the global gradient norm of the last step, before clipping
        self._check_arguments(example_x, loss_fn, segments, skip_nonfinite)
        self._static_input(example_x, transform)
        self.loss_fn = loss_fn or _default_loss
        self.params = [p for p in model.parameters() if p.requires_grad]
        self.coders = [m for m in model.modules() if hasattr(m, "deferCounts")]
        self.closed = False
        if self.world > 1 and broadcast:
            self._broadcast_state()
        model.train()
        for c in self.coders:
            c.deferCounts(True)
        # (under a process group RCCL's watchdog thread may query events while we capture: thread-local mode keeps a capture from
        #  being invalidated by what OTHER threads do; the autograd thread's launches are captured either way -- capture follows
        #  the stream, not the thread)
        self._mode = dict(capture_error_mode="thread_local") if (dist.is_available() and dist.is_initialized()) else {}
        # warm-up and capture share ONE side stream: autograd's gradient accumulators remember the stream they were created on, and
        # a capture on another stream would pull that one (the legacy default stream, if the warm-up ran there) into the graph
        self._stream = torch.cuda.Stream(self.x.device)
        self._stream.wait_stream(torch.cuda.current_stream(self.x.device))
        from .nn import blocks
        streams, blocks._BRANCH_STREAMS = blocks._BRANCH_STREAMS, False     # nested stream forks crash hipGraph capture (ROCm 7.2): one stream
        try:
            self._warm_segments(warmup)                       # inside: the warm-up runs (and traces) the single-stream launches the capture records
            pinned = self._pin_operand_streams()              # inside: sets `_packMasks`, which the captured re-pack reads
            # inside because they lie between the two: they need the warm-up's gradients, and the captures need them; a failure of any
            # of them hands the coders back to the eager update like a failed capture
            self._flat_layout()
            self._gather_tables()
            self._accum_buffers()
            self._init_optimizer_state()
            self._capture_segments()                          # inside: one stream, and the re-pack masks
        except BaseException:
            for c in self.coders:
                c.deferCounts(False)
            raise
        finally:
            model.__dict__.pop("_packMasks", None)
            blocks._BRANCH_STREAMS = streams
        self._pinned = pinned + [c.countSink() for c in self.coders]     # (what the graphs hold addresses of: alive as long as the step)
        self._bind_grads()
        self._prepare_update()
        self._capture_post(capture_post)

    # ---- the constructor's phases, in its order ------------------------------------------------------------------------------
    def _check_arguments(self, example_x, loss_fn, segments, skip_nonfinite):
        """Every refusal of the constructor, before anything is built; leaves `self.segments` and `self.guard`."""
        optimizer, max_grad_norm = self.optimizer, self.max_grad_norm
        if not example_x.is_cuda:
            raise RuntimeError("GraphedTrainStep needs a HIP device (hipGraph capture)")
        if not isinstance(self.accumulate, int) or isinstance(self.accumulate, bool) or self.accumulate < 1:
            raise ValueError(f"accumulate must be an int >= 1 (micro-batches per update), got {self.accumulate!r}")
        if self.scheduler is not None and getattr(self.scheduler, "optimizer", None) is not optimizer:
            raise ValueError("GraphedTrainStep: `scheduler` steps another optimizer's learning rates than `optimizer`'s")
        if self.reassign is not None and not all(any(c is p for p in self.model.parameters()) for c in self.reassign.codebooks):
            raise ValueError("GraphedTrainStep: `reassign` refills another model's codebooks than `model`'s")
        staged = all(hasattr(self.model, a) for a in ("_encoder", "_quantizer", "_decoder", "_repackStale")) and set(self.kwargs) <= {"uniforms"}
        if segments is None:
            segments = 3 if (self.world > 1 and staged) else 1
        if segments not in (1, 3):
            raise ValueError("segments must be 1 (one graph, one all-reduce) or 3 (decoder / quantizer / encoder backward)")
        if segments == 3 and not staged:
            raise ValueError("segments=3 needs a model with _encoder / _quantizer / _decoder stages and no forward_kwargs but `uniforms`")
        if segments == 3 and getattr(loss_fn, "single_segment", False):
            raise ValueError("this loss_fn reaches parameters from outside the model's output (loss.step_loss(rate=...) reads the codebooks): "
                             "their gradients would come from two segments; use segments=1")
        self.segments = segments
        if max_grad_norm is not None and not max_grad_norm > 0:
            raise ValueError("max_grad_norm must be positive (or None: no clipping)")
        if max_grad_norm is not None and getattr(optimizer, "max_grad_norm", None) is not None:
            raise ValueError("both the step and the optimizer clip (`max_grad_norm`): the gradient would be scaled twice; set one of them")
        self.guard = None                                     # guard.StepGuard with `skip_nonfinite`: the flag every launch of the update obeys
        if skip_nonfinite:
            if not self._own_optimizer():
                raise ValueError("skip_nonfinite needs an optimizer whose kernels take the guard's flag (mcquic_amd.optim.Adam / AdamW / Lamb / "
                                 f"SGD); {type(optimizer).__module__}.{type(optimizer).__name__} would update through a skipped step")
            if optimizer.guards_itself:
                raise ValueError("both the step and the optimizer guard against a non-finite gradient (`skip_nonfinite`): one step would be "
                                 "counted twice; set one of them")
            from .guard import StepGuard
            self.guard = StepGuard(example_x.device)
        if loss_fn is not None and not memset_nodes_replay_correctly(example_x.device):
            import warnings
            warnings.warn("this process replays memset nodes of captured hipGraphs wrongly (ROCm 7.2; DEBUG_CLR_GRAPH_PACKET_CAPTURE=0 was not "
                          "in the environment when the HIP runtime started): a library reduction inside `loss_fn` (x.mean(), x.sum() over "
                          "~1e5+ elements) may return stale values from a replay.  Import mcquic_amd before the first device call, or set the "
                          "variable yourself.", RuntimeWarning, stacklevel=3)

    def _own_optimizer(self) -> bool:
        """Is the optimizer one of `mcquic_amd.optim`'s: does it answer `guards_itself`, `lends_norm`, `last_grad_norm()`, `skip_count()`?"""
        from .optim import _Planned
        return isinstance(self.optimizer, _Planned)

    def _static_input(self, example_x, transform):
        """`self.x`, the model's static input; with a transform `self.raw` holds the RAW images and the transform's two launches write self.x."""
        self.x = example_x.detach().clone()
        self.transform, self.raw = transform, None
        if transform is not None:
            self.raw = self.x
            self.transform = transform.to(self.raw.device)    # (its generator state and gain table: on the device before any capture)
            with torch.no_grad():
                self.x = self.transform(self.raw).detach()

    def _warm_segments(self, warmup: int):
        """The segments eagerly on the capture's stream: caches, workspaces, the coders' count sinks, every parameter's `.grad` -- and the
        trace of which copy of its operand stream every conv launch of the step reads."""
        from . import ops
        ops.section_trace(True)
        try:
            with torch.cuda.stream(self._stream):
                for _ in range(max(1, warmup)):
                    for k in range(self.segments):
                        self._segment(k)
            torch.cuda.current_stream(self.x.device).wait_stream(self._stream)
        finally:
            ops.section_trace(False)

    def _pin_operand_streams(self) -> list:
        """The operand streams the graphs re-pack into / read from, to be kept for as long as they live; the copies the warm-up's launches
        read go into the model's `_packMasks`: the captured re-pack refreshes those only (replays repeat the launches)."""
        from . import ops
        masks, pinned = {}, []
        for m in self.model.modules():
            for pk in (m.__dict__.get("_packed"), getattr(m.__dict__.get("_dgradCache"), "packed", None)):
                if pk is not None and hasattr(pk, "wp"):
                    pinned.append(pk.wp)
                    used = ops.sections_used(pk)
                    if used:
                        masks[id(pk)] = used
        self.model.__dict__["_packMasks"] = masks
        return pinned

    def _flat_layout(self):
        """`live_groups`, `live`, `flat`, `slices`: the flat layout is the segments' order (backward order), parameters the warm-up gave no
        gradient left out."""
        self.live_groups = [[p for p in g if p.grad is not None] for g in self._param_groups()]
        self.live = [p for g in self.live_groups for p in g]
        self.flat = torch.empty(sum(p.numel() for p in self.live), dtype=torch.float32, device=self.x.device)
        self.slices, off = [], 0
        for g in self.live_groups:
            n = sum(p.numel() for p in g)
            self.slices.append(self.flat[off: off + n])
            off += n

    def _capture_segments(self):
        """`graphs` (and `graph`, the first): each segment with the gather of its gradients behind it; the first one leaves `counts`."""
        torch.cuda.synchronize()
        with torch.no_grad():
            torch._foreach_add_(self.params, 0.0)             # every parameter "changed": the capture records all re-packs
        for p in self.params:
            p.grad = None
        self.graphs, self.counts = [], None
        pool = torch.cuda.graph_pool_handle() if self.segments > 1 else None
        for k in range(self.segments):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=pool, stream=self._stream, **self._mode):
                self._segment(k)
                if self.live_groups[k]:
                    self._gather(k)
                if k == 0:
                    sinks = [c.countSink() for c in self.coders]
                    # (one coder per model: its count buffer itself -- the sampling kernels add into it, nothing is copied)
                    self.counts = (sinks[0] if len(sinks) == 1 else torch.cat(sinks)) if sinks else None
                    if self.accumulate > 1:
                        self._accum_scalars()
            self.graphs.append(g)
        self.graph = self.graphs[0]
        self._carry = None                                    # (the autograd graph between segments: only needed while capturing)

    def _bind_grads(self):
        """Every live parameter's `.grad` becomes its view of the flat buffer: the optimizer reads the reduced gradients."""
        off = 0
        for p in self.live:
            p.grad = self.flat[off: off + p.numel()].view_as(p)
            off += p.numel()

    def _prepare_update(self):
        """Everything the update needs before it can be captured: who runs the guard, then every participant's device tables and its
        kernels' first launch -- a throw-away update after which its state has its bits back (the EMA's averages and count; the meter's
        count, shadow and ring; the schedule's last_epoch, state and rates; the statistics' count, blame words, ring and shadow; the
        reassignment's count, generator state and scalars)."""
        if self.guard is not None:
            # who runs the guard: the step from its clip's sum of squares; else the optimizer from the partials of its own norm (Lamb,
            # SGD with max_grad_norm); else the step over the flat buffer
            self._guard_lender = "clip" if self.max_grad_norm is not None else "optimizer" if self.optimizer.lends_norm else "flat"
            self.optimizer.attach_guard(self.guard, decided=self._guard_lender != "optimizer")
            if self._guard_lender == "flat":
                self.guard.prepare_flat(self.flat)
            self.grad_norm = self.guard.grad_norm
        if hasattr(self.optimizer, "prepare"):                # (mcquic_amd.optim.Adam / Lamb / SGD: device tables for the flat gradient views)
            self.optimizer.prepare()
        for h in (self.ema, self.meter, self.scheduler, self.stats, self.reassign):
            if h is not None:
                h.prepare()
                h.warm()
        if self.guard is not None:
            self._warm_guard()

    def _capture_post(self, capture_post: bool):
        """`post`: the update as one graph, or None -- not asked for, or an optimizer that cannot be captured: its update runs eagerly."""
        self.post = None
        if not capture_post:
            return
        before = self._snapshot_optimizer_state()
        try:
            post = torch.cuda.CUDAGraph()
            with torch.cuda.graph(post, stream=self._stream, **self._mode):
                self._update(self.guard)
            self.post = post
        except Exception:
            torch.cuda.synchronize()
            self._restore_optimizer_state(before)            # (host-side counters may have moved before the capture gave up)

    def _gather(self, k: int):
        """Segment k's gradients into its slice of the flat buffer: ONE launch over device tables (mcq_gather_flat_f32) instead of
        torch.cat's six.  Called inside the capture: the gradients' addresses (allocations of the captured backward pass, the same
        on every replay) reach the device table through a copy node from a pinned host tensor this object keeps alive."""
        from . import _lib
        from .ops import check, _guard, _stream
        params = self.live_groups[k]
        lib = _lib.load()
        dev = self.flat.device
        table, offs, host, ptrs = self._gatherTables[k]
        grads = [p.grad if p.grad.is_contiguous() else p.grad.contiguous() for p in params]
        self._gatherGrads[k] = grads                          # (alive as long as the tables point at them)
        host.copy_(torch.tensor([g.data_ptr() for g in grads], dtype=torch.int64))
        ptrs.copy_(host, non_blocking=True)                   # (a copy NODE inside the capture: re-read from the pinned tensor on every replay)
        if self.accumulate > 1:                               # the same tables, accumulating by the phase word (mcq_gather_accum_flat_f32)
            from . import ops
            ops.gather_accum_flat_(ptrs, self.slices[k], offs, table, self._phase, self.accumulate)
            return
        with _guard(dev):
            check(lib.mcq_gather_flat_f32(ptrs.data_ptr(), self.slices[k].data_ptr(), offs.data_ptr(), table.numel.data_ptr(),
                                          table.blk_tensor.data_ptr(), table.blk_first.data_ptr(), table.nblocks, _stream()), "mcq_gather_flat_f32")

    def _accum_buffers(self):
        """With `accumulate` > 1, OUTSIDE the captures and alive as long as the step: the device phase word the accumulating launches
        read, the pinned [0 .. k-1] array the host copies it from before every replay, the int64 accumulator of the code counts (as long
        as the coders' sinks together) and the float32 accumulator of the loss.  With accumulate=1 nothing is made."""
        self._phase = self._phaseHost = self._countsAcc = self._lossAcc = None
        if self.accumulate == 1:
            return
        dev = self.flat.device
        self._phase = torch.zeros(1, dtype=torch.int32, device=dev)
        self._phaseHost = torch.arange(self.accumulate, dtype=torch.int32).pin_memory()
        n = sum(c.countSink().numel() for c in self.coders)
        self._countsAcc = torch.zeros(n, dtype=torch.int64, device=dev) if n else None
        self._lossAcc = torch.zeros((), dtype=torch.float32, device=dev)

    def _accum_scalars(self):
        """The last launch of segment 0's capture with `accumulate` > 1 (mcq_accum_step_scalars): this micro-step's counts (`self.counts`:
        the sink the prologue zeroes on every replay) into the step's accumulator and its loss into the mean; from here on `self.counts`
        and `self.loss` ARE the accumulators -- what the all-reduce, `applyCounts`, the meter and the caller read."""
        from . import ops
        if not (torch.is_tensor(self.loss) and self.loss.dtype == torch.float32 and self.loss.numel() == 1):
            raise ValueError("GraphedTrainStep(accumulate > 1): the loss must be one float32 on the device (its mean over the micro-batches is "
                             "formed by a kernel)")
        ops.accum_step_scalars_(self.counts, self._countsAcc, self.loss, self._lossAcc, self._phase, self.accumulate)
        self.counts, self.loss = self._countsAcc, self._lossAcc

    def _gather_tables(self):
        """The static side of `_gather`, built OUTSIDE the captures (host-to-device copies from pageable memory invalidate a capture): per
        segment (chunk table, offsets into the slice, pinned host pointers, device pointers).  The pointer pair is the gather's own and not
        a `TensorList`: its addresses are known only inside the capture and travel through a copy node."""
        from .tensor_list import ChunkTable
        dev = self.flat.device
        self._gatherTables, self._gatherGrads = {}, {}
        for k, params in enumerate(self.live_groups):
            if not params:
                continue
            sizes = [p.numel() for p in params]
            offs = torch.tensor([0] + sizes[:-1], dtype=torch.int64).cumsum(0)     # (densely packed: a gradient's slice is only 4-byte aligned)
            self._gatherTables[k] = (ChunkTable(sizes, dev), offs.to(dev),
                                     torch.empty(len(params), dtype=torch.int64, pin_memory=True), torch.empty(len(params), dtype=torch.int64, device=dev))
        torch.cuda.synchronize()

    # ---- replica state ---------------------------------------------------------------------------------------------------
    def _broadcast_state(self):
        """Rank 0's parameters and buffers to every rank (what DDP's constructor does): replicas that start from different
        weights would average gradients of diverging models without any error."""
        src = dist.get_global_rank(self.group, 0) if self.group is not None else 0
        seen = set()
        with torch.no_grad():
            for t in list(self.model.parameters()) + list(self.model.buffers()):
                if id(t) in seen:
                    continue
                seen.add(id(t))
                buf = _staged(t.detach(), self.group)
                buf = buf if buf.is_contiguous() else buf.contiguous()
                dist.broadcast(buf, src, group=self.group)
                if buf.data_ptr() != t.data_ptr():
                    t.copy_(buf)

    # ---- optimizer state ---------------------------------------------------------------------------------------------------
    def _snapshot_optimizer_state(self):
        return {(id(p), k): v.detach().clone() for p, st in self.optimizer.state.items() for k, v in st.items() if torch.is_tensor(v)}

    def _restore_optimizer_state(self, snap):
        """State tensors that existed at the snapshot get their values back; the ones created since are zeroed -- which is the
        state a fresh optimizer starts from (SGD with momentum, Adam / AdamW; an optimizer whose initial state is not zeros
        needs its own warm-up)."""
        with torch.no_grad():
            for p, st in self.optimizer.state.items():
                for k, v in st.items():
                    if torch.is_tensor(v):
                        old = snap.get((id(p), k))
                        if old is None:
                            v.zero_()
                        else:
                            v.copy_(old)

    def _init_optimizer_state(self):
        """An optimizer creates its state (momentum buffers, Adam's moments and step counter) inside its first `step()`; created
        inside the capture they would be re-created by every replay.  One throw-away update with the warm-up gradients brings
        them into existence; then the parameters and every state tensor that existed BEFORE (an optimizer resumed from a
        checkpoint: momentum, moments, step counters) are restored and only the newly created ones are zeroed."""
        saved = [p.detach().clone() for p in self.params]
        snap = self._snapshot_optimizer_state()
        self.optimizer.step()
        with torch.no_grad():
            for p, v in zip(self.params, saved):
                p.copy_(v)
        self._restore_optimizer_state(snap)

    # ---- the step's segments ---------------------------------------------------------------------------------------------
    def _param_groups(self):
        """Parameters by segment, in the order the backward pass finishes them: decoder, quantizer, encoder (+ anything else)."""
        if self.segments == 1:
            return [list(self.params)]
        taken, groups = set(), []
        for stage in (self.model._decoder, self.model._quantizer):
            g = [p for p in stage.parameters() if p.requires_grad and id(p) not in taken]
            taken.update(id(p) for p in g)
            groups.append(g)
        groups.append([p for p in self.params if id(p) not in taken])
        return groups

    def _segment(self, k: int):
        if self.segments == 1:
            self.loss = self._forward_backward()
            return
        from . import ops
        m = self.model
        if k == 0:
            for p in self.params:
                p.grad = None
            self._input()
            m._repackStale()
            y = m._trainEncode(self.x) if hasattr(m, "_trainEncode") else m._encoder(self.x)     # (no padding in the training forward, compressor.py:39)
            yl = y.detach().requires_grad_()
            tw = ops.silu_twin(y)
            if tw is not None:
                ops.set_silu_twin(yl, tw)
            yHat, codes, logits = m._quantizer(yl, self.kwargs.get("uniforms"))
            yh = yHat.detach().requires_grad_()
            tw = ops.silu_twin(yHat)
            if tw is not None:
                ops.set_silu_twin(yh, tw)
            lgl = [lg.detach().requires_grad_() if (torch.is_tensor(lg) and lg.requires_grad) else lg for lg in logits]
            xHat = m._decoder(yh)
            loss = self.loss_fn((xHat, yh, codes, lgl), self.x)
            _backward(loss)                                   # decoder parameters, d yHat (, d logits)
            self._keep((xHat, yHat, codes, logits))
            self.loss = loss.detach()
            self._carry = (y, yl, yHat, yh, logits, lgl)
        elif k == 1:
            y, yl, yHat, yh, logits, lgl = self._carry
            outs, grads = [yHat], [yh.grad]
            for lg, leaf in zip(logits, lgl):
                if torch.is_tensor(leaf) and leaf is not lg and leaf.grad is not None:
                    outs.append(lg)
                    grads.append(leaf.grad)
            from .autograd import run_backward
            run_backward(outs, grads)                         # quantizer parameters, d y
        else:
            y, yl = self._carry[0], self._carry[1]
            from .autograd import run_backward
            run_backward([y], [yl.grad])                      # encoder parameters
            self._carry = None

    def _input(self):
        """With a transform: the draw and the apply launch, from the static raw batch into the model's static input."""
        if self.transform is not None:
            with torch.no_grad():
                self.transform(self.raw, out=self.x)

    def _forward_backward(self):
        for p in self.params:
            p.grad = None
        self._input()
        out = self.model(self.x, **self.kwargs)
        loss = self.loss_fn(out, self.x)
        _backward(loss)
        self._keep(out)
        return loss.detach()

    def _keep(self, out):
        """With `keep_outputs`: references to the reconstruction, the codes and the level-0 logits of the forward pass, so that the
        capture's allocations stay theirs after the backward pass (no launch is added; the graph's pool is larger by the logits)."""
        if not self.keep_outputs:
            return
        if not (isinstance(out, (tuple, list)) and len(out) == 4 and len(out[3]) > 0):
            raise ValueError("GraphedTrainStep(keep_outputs=True): the model's training forward must return (xHat, yHat, codes, logits)")
        self.outputs = (out[0].detach(), [c.detach() for c in out[2]], out[3][0].detach())

    @torch.no_grad()
    def snapshot(self, snap) -> dict:
        """The log payload of the LAST replay (`monitor.StepSnapshot.read()`'s dict) from the step's static input and outputs: `snap`'s
        launches go to the current stream, behind the replay, when the host wants one (the reference: every `ValFreq // 10` steps);
        nothing of it is in the captured graphs.  Needs `keep_outputs=True`."""
        if self.closed:
            raise RuntimeError("GraphedTrainStep: the step was closed; build a new one")
        if self.outputs is None:
            raise RuntimeError("GraphedTrainStep.snapshot: build the step with `keep_outputs=True` (the captured forward pass frees its "
                               "reconstruction, codes and logits otherwise)")
        xHat, codes, logits0 = self.outputs
        snap.capture(self.x, xHat, codes, logits0)
        return snap.read()

    def _update(self, guard=None, decides: bool = True):
        """The update, written once -- captured as the post graph, or run eagerly after the exchange: `/ world`, clip, optimizer, EMA,
        frequency EMA, codebook reassignment, scheduler, meter (`stats` around the optimizer).  `guard`: the `StepGuard` whose flag every launch takes, or None: the launches are the ones
        they have always been (every entry point selects its plain kernel for a flag that is None).  `decides`: the guard's own launches
        run here, on the all-reduced, averaged gradient (not in `_warm_guard`, whose scratch flag is set by hand)."""
        from . import ops
        flag = None if guard is None else guard.skip
        if self.world > 1:
            self.flat.mul_(1.0 / self.world)
        if self.max_grad_norm is not None:                    # trainer.py:280 `clip_grad_norm(4.0)`: global norm of the AVERAGED gradient,
            sq = ops.sumsq(self.flat)                         # two launches over the flat buffer, nothing read by the host
            if guard is not None and decides:                 # the clip's sum of squares decides: no second reduction
                guard.from_norm(sq, squared=True)
            norm = ops.clip_by_norm_(self.flat, self.max_grad_norm, sq=sq, skip=flag)
            if guard is None:                                 # (with a guard `grad_norm` is the guard's)
                self.grad_norm = norm
        elif guard is not None and decides and self._guard_lender == "flat":
            guard.run_flat(self.flat)
        if self.stats is not None:                            # (the clip has run: the gradient is the one the optimizer consumes)
            self.stats.before()
        self.optimizer.step()                                 # (`attach_guard`: every launch obeys; the "optimizer" lender runs the guard here)
        if self.stats is not None:
            self.stats.after(skip=flag)
        if self.ema is not None:
            self.ema.update(skip=flag)
        self._apply_counts(flag)
        if self.reassign is not None:                         # (the reference's hook runs at step finish: the NEW frequencies are consulted)
            self.reassign.step(skip=flag)
        if self.scheduler is not None:                        # (the reference's order, trainer.py `_stepFinish`: step the scheduler, then log
            self.scheduler.step(skip=flag)                    #  get_last_lr(): the meter's `lr` column is the rate of the NEXT update)
        if self.meter is not None:
            self._meter_update()

    def _apply_counts(self, skip=None):
        """The frequency EMA of every coder from its part of the GLOBAL counts."""
        off = 0
        for c in self.coders:
            n = c.countSink().numel()
            c.applyCounts(self.counts[off: off + n], skip=skip)
            off += n

    def _warm_guard(self):
        """Every kernel of the guarded update once outside any capture, without moving a bit of state: the guard's own three launches into
        a scratch record, then the update under that scratch guard with its flag SET (a skipped launch writes nothing)."""
        from . import ops
        from .guard import StepGuard
        scratch = StepGuard(self.flat.device)
        scratch.run_flat(self.flat)
        scratch.from_partials(scratch._partials, 1)
        scratch.from_norm(ops.sumsq(self.flat), squared=True)
        scratch.record[0] = 1                                 # (the int32 `skip` is the low word)
        self.optimizer.attach_guard(scratch, decided=True)
        meter, self.meter = self.meter, None                  # (it has warmed itself and obeys no flag: a row of the warm-up would stay)
        stats, self.stats = self.stats, None                  # (likewise: a set flag FORCES a row)
        try:
            self._update(scratch, decides=False)
        finally:
            self.meter, self.stats = meter, stats
            self.optimizer.attach_guard(self.guard, decided=self._guard_lender != "optimizer")
        torch.cuda.synchronize()

    def _meter_update(self):
        """The telemetry row of this step (monitor.StepMeter.update): every value goes by device pointer, nothing is read here."""
        opt, norm, skipped = self.optimizer, self.grad_norm, None
        if self.guard is not None:                            # (the guard's record: its norm, its count of skipped steps)
            norm, skipped = self.guard.grad_norm, self.guard.skipped
        elif self._own_optimizer():
            if norm is None:                                  # (Lamb always; SGD with max_grad_norm or skip_nonfinite)
                norm = opt.last_grad_norm()
            skipped = opt.skip_count()                        # (SGD always; Adam / AdamW / Lamb with their own `skip_nonfinite`)
        self.meter.update(self.loss, self.counts, grad_norm=norm, lr=opt.param_groups[0]["lr"], skipped=skipped)

    def _start_all_reduce(self, buf: torch.Tensor):
        """Sum `buf` over the ranks without waiting for it: under RCCL an async all-reduce (its stream waits for what the current
        stream has enqueued so far -- the segment that just filled `buf` -- and the returned work is joined before the post
        graph); under gloo (tests) the blocking host-staged form."""
        if buf.numel() == 0:
            return None
        if buf.is_cuda and dist.get_backend(self.group) == "gloo":
            all_reduce_(buf, self.group)
            return None
        return dist.all_reduce(buf, group=self.group, async_op=True)

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        if self.closed:
            raise RuntimeError("GraphedTrainStep: the step was closed (its count sinks are gone); build a new one")
        if self.ema is not None and self.ema.swapped:
            raise RuntimeError("GraphedTrainStep: the EMA's averaged weights are swapped in (`ema.applied()` / `ema.swap()`); training would "
                               "update the average as if it were the iterate -- swap back first")
        static = self.x if self.raw is None else self.raw
        acc, n = self.accumulate, static.shape[0]
        if tuple(x.shape) != (acc * n,) + tuple(static.shape[1:]):     # (`copy_` would BROADCAST a smaller batch into the static input silently)
            raise RuntimeError(f"GraphedTrainStep was captured for shards of shape {tuple(static.shape)}" +
                               (f" and accumulate={acc} (k = {acc} of them per call: {(acc * n,) + tuple(static.shape[1:])})" if acc > 1 else "") +
                               f", got {tuple(x.shape)}")
        if self.raw is not None and x.dtype != static.dtype:  # (`copy_` would convert a uint8 batch to float without the / 255)
            raise RuntimeError(f"GraphedTrainStep was captured for {static.dtype} shards, got {x.dtype}")
        for j in range(acc - 1):                              # micro-steps 0 .. k-2: accumulate, exchange nothing
            self._micro_step(static, x, j, exchange=False)
        # the last (or only) micro-step: the buffers hold the mean / the summed counts
        for w in self._micro_step(static, x, acc - 1, exchange=self.world > 1):
            if w is not None:
                w.wait()                                      # (the current stream waits; the host does not)
        if self.post is not None:
            self.post.replay()
        else:
            self._update(self.guard)
        for c in self.coders:
            c.resetFreqAndCDF()
        return self.loss

    def _micro_step(self, static, x, j: int, exchange: bool) -> list:
        """Micro-batch j into the static input (with `accumulate` > 1 also j into the phase word: stream-ordered like the input's copy, no
        host read, no sync), then the segments' replays; with `exchange` the all-reduce of each segment's slice (and of the counts,
        behind the first) is started as soon as the segment is enqueued, while the next one replays: the works to join."""
        if self.accumulate > 1:
            n = static.shape[0]
            static.copy_(x[j * n: (j + 1) * n], non_blocking=True)
            self._phase.copy_(self._phaseHost[j: j + 1], non_blocking=True)
        else:
            static.copy_(x, non_blocking=True)
        works = []
        for k, g in enumerate(self.graphs):
            g.replay()
            if exchange:
                works.append(self._start_all_reduce(self.slices[k]))
                if k == 0 and self.counts is not None:
                    works.append(self._start_all_reduce(self.counts))
        return works

    def invalidate(self):
        """Replays change the parameters without the host seeing it (no version counter moves): mark every parameter changed so
        that the next EAGER use of the model (evaluation, a checkpoint's `compress`) re-packs its operand streams -- they are one
        update behind after a replay.  Call before using the model outside this step; `close()` does.  The step itself stays
        usable: its graphs re-pack the copies they read at the start of every replay, into streams this object keeps alive."""
        with torch.no_grad():
            torch._foreach_add_(self.params, 0.0)

    def close(self):
        """Back to the eager step for good: the coders update their EMA inside forward again, `.grad` is whatever the last step
        left, and this object refuses further replays (its count sinks are released)."""
        if self.closed:
            return
        self.closed = True
        for c in self.coders:
            c.deferCounts(False)
        self.invalidate()
        self._pinned = []
