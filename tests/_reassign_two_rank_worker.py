"""One rank of tests/test_gpu_reassign_two_ranks.py: both ranks sit on cuda:0 and talk over gloo (RCCL refuses two ranks on one
device).  parallel.GraphedTrainStep(segments=3, reassign=CodebookReassign(model, freq=2)) over four steps on the small Compressor of
tests/test_gpu_ema_step.py, each rank on its own shard; after every step the ranks' codebooks are gathered and compared bit for bit.
The ranks pass DIFFERENT seeds: the constructor takes rank 0's.  torch.distributed's collectives are counted while the steps run."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def main():
    path = sys.argv[1]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import mcquic_amd
    from mcquic_amd import optim, parallel
    from test_gpu_reassign_step import _setup
    model, xs, us = _setup(dev)
    re = mcquic_amd.CodebookReassign(model, freq=2, seed=5 + rank)
    x = xs[rank]                                                        # this rank's shard
    step = parallel.GraphedTrainStep(model, optim.SGD(model.parameters(), lr=1e-2, momentum=0.9), x, forward_kwargs={"uniforms": us},
                                     segments=3, reassign=re)
    calls = {"all_reduce": 0, "broadcast": 0, "barrier": 0, "all_gather": 0}
    originals = {name: getattr(dist, name) for name in calls}

    def counted(name):
        def call(*a, **kw):
            calls[name] += 1
            return originals[name](*a, **kw)
        return call
    rows = []
    for it in range(4):
        for name in calls:
            setattr(dist, name, counted(name))
        try:
            step(xs[(rank + it) % 2])
        finally:
            for name, fn in originals.items():
                setattr(dist, name, fn)
        torch.cuda.synchronize()
        mine = torch.cat([c.detach().flatten() for c in model.Codebooks]).cpu()
        both = [torch.empty_like(mine) for _ in range(world)]
        dist.all_gather(both, mine)
        out = re.read()
        rows.append({"equal": bool(torch.equal(both[0].view(torch.int32), both[1].view(torch.int32))), "moved": out["moved"],
                     "fired": out["fired"], "count": out["count"], "seed": out["seed"], "offset": out["offset"]})
    record = [torch.empty(7, dtype=torch.int64) for _ in range(world)]
    dist.all_gather(record, re._state.cpu())
    result = {"rows": rows, "calls": calls, "segments": step.segments, "post_captured": step.post is not None,
              "records_equal": bool(torch.equal(record[0], record[1]))}
    step.close()
    torch.cuda.synchronize()
    dist.barrier()
    if rank == 0:
        json.dump(result, open(path, "w"))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
