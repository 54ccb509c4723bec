"""Worker of tests/test_gpu_accum_two_ranks.py: one of TWO processes that share cuda:0 and talk over gloo (RCCL refuses two ranks on
one device; tests/_two_rank_worker.py's arrangement).  Each rank runs parallel.GraphedTrainStep(accumulate=2) on ITS two micro-batches of
one image (segments=3: the exchange overlapped slice by slice, on the last micro-step only); rank 0 first makes the same update alone
with accumulate=4 on all four micro-batches, compares and writes a JSON verdict.

    RANK=r WORLD_SIZE=2 MASTER_ADDR=127.0.0.1 MASTER_PORT=p python tests/_accum_two_rank_worker.py out.json
"""
import copy
import json
import os
import sys

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(rank, world, dev):
    from mcquic_amd import Compressor, parallel
    ks, hw, lr, per, steps = [64, 32, 16], 64, 1e-2, 2, 2
    torch.manual_seed(3407)
    model = Compressor(32, 2, ks).to(dev).train()
    g = torch.Generator().manual_seed(11)
    xs = [(torch.rand((per * world, 3, hw, hw), generator=g) * 2 - 1).to(dev) for _ in range(steps)]       # four micro-batches of ONE image per update
    us = []
    for lv, k in enumerate(ks):
        s = hw // 16 // (2 ** lv)
        us.append((torch.rand((1, 2, s, s, k), generator=g).to(dev), torch.rand((1, 2, s, s, k), generator=g).to(dev)))
    init = [p.detach().clone() for p in model.parameters()]
    solo = dist.new_group([0])                                           # (collective over the default group: both ranks call it)
    out, ref, ref_ema, ref_losses = {}, None, None, None
    if rank == 0:
        alone = copy.deepcopy(model)
        step = parallel.GraphedTrainStep(alone, torch.optim.SGD(alone.parameters(), lr=lr), xs[0][:1], forward_kwargs={"uniforms": us},
                                         group=solo, segments=3, accumulate=per * world)
        out["solo_world"] = step.world
        ref_losses = [float(step(x)) for x in xs]
        out["solo_counts_total"] = int(step.counts.sum())
        step.close()
        torch.cuda.synchronize()
        ref = [p.detach().clone() for p in alone.parameters()]
        ref_ema = [f.detach().clone() for f in alone._quantizer._entropyCoder._freqEMA]
    dist.barrier()
    lo, hi = rank * per, (rank + 1) * per
    step = parallel.GraphedTrainStep(model, torch.optim.SGD(model.parameters(), lr=lr), xs[0][:1], forward_kwargs={"uniforms": us}, accumulate=per)
    losses = [float(step(x[lo:hi])) for x in xs]
    counts_total = int(step.counts.sum())
    step.close()
    torch.cuda.synchronize()
    both = [torch.zeros(steps, dtype=torch.float64) for _ in range(world)]
    dist.all_gather(both, torch.tensor(losses, dtype=torch.float64))
    if rank == 0:
        worst, worst_name, moved = 0.0, "", 0.0
        for (name, p), r, p0 in zip(model.named_parameters(), ref, init):
            if not p.requires_grad:
                continue
            upd = float((r - p0).abs().max())
            if upd == 0.0:
                continue
            # (tests/_two_rank_worker.py's unit: 1e-4 of the update itself plus 4 ulps of the parameter's own magnitude)
            tol = 1e-4 * upd + 4 * 1.1920929e-07 * float(r.abs().max())
            rel = float((p.detach() - r).abs().max()) / tol
            moved = max(moved, upd)
            if rel > worst:
                worst, worst_name = rel, name
        out.update(worst_update_rel_err=worst, worst_update_name=worst_name, largest_update=moved, post_captured=step.post is not None,
                   segments=step.segments, world=step.world, accumulate=step.accumulate, counts_total=counts_total,
                   ema_max_abs_diff=max(float((a - b).abs().max()) for a, b in zip(ref_ema, model._quantizer._entropyCoder._freqEMA)),
                   solo_losses=ref_losses, mean_rank_losses=[float(v) for v in (both[0] + both[1]) / 2])
    return out


def main():
    path = sys.argv[1]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)                                       # BOTH ranks on the one GPU
    dist.init_process_group("gloo", rank=rank, world_size=world)
    out = run(rank, world, dev)
    torch.cuda.synchronize()
    dist.barrier()
    if rank == 0:
        json.dump(out, open(path, "w"))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
