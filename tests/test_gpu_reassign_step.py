"""mcquic_amd.CodebookReassign through parallel.GraphedTrainStep(..., reassign=...), on the model and shards of tests/test_gpu_ema_step.py:
Compressor(32, 2, [64, 32, 16]), two 64 x 64 images, fixed uniforms, mcquic_amd.optim.SGD.  `_freqEMA` is set by hand so that more than
half of one group and a few of another are exactly zero on every level; a step of 2 x 4 x 4 (level 0) codes per group cannot touch all of
k = 64 entries, so zeros survive the update.  The yardstick is tests/_reassign_ref.py (pinned to the eager torch method on CPU), applied
to what the SAME step without `reassign` leaves behind."""
import copy

import numpy as np
import pytest
import torch

import _reassign_ref as RR

pytestmark = pytest.mark.gpu
SEED = 11


def _setup(dev):
    from test_gpu_ema_step import _setup as base
    model, xs, us = base(dev)
    with torch.no_grad():
        for f in model._quantizer._entropyCoder._freqEMA:
            k = f.shape[1]
            f[0, torch.randperm(k, generator=torch.Generator().manual_seed(k))[: k // 2 + k // 4]] = 0.0
            f[1, :3] = 0.0
    return model, xs, us


def _sgd(model):
    from mcquic_amd import optim
    return optim.SGD(model.parameters(), lr=1e-2, momentum=0.9)


def _yardstick(model, seed, offset):
    """The numpy rule on `model`'s codebooks and raw `_freqEMA` as they are, priorities = hash_uniform({seed, offset + level})."""
    from mcquic_amd import ops
    out = []
    for lv, (cb, f) in enumerate(zip(model.Codebooks, model._quantizer._entropyCoder._freqEMA)):
        snap = torch.tensor([seed, offset + lv], dtype=torch.int64).to(f.device)
        prio = ops.hash_uniform(snap, ops.REASSIGN_STREAM, tuple(f.shape)).cpu().numpy()
        out.append(RR.reassign(cb.detach().cpu().numpy(), f.detach().cpu().numpy(), prio))
    return out


def _bits_equal(t, a):
    return np.array_equal(t.detach().cpu().numpy().view(np.uint32), a.view(np.uint32))


def _named(model):
    return list(model.named_parameters()) + list(model.named_buffers())


@pytest.fixture(scope="module")
def pair(dev):
    """One replay of the step with CodebookReassign(model, freq=1) and of its twin without, from identical state."""
    import mcquic_amd
    from mcquic_amd import parallel
    ours, xs, us = _setup(dev)
    twin = copy.deepcopy(ours)
    re = mcquic_amd.CodebookReassign(ours, freq=1, seed=SEED)
    built, initial = re._state.clone(), [c.detach().clone() for c in ours.Codebooks]
    opt_o, opt_t = _sgd(ours), _sgd(twin)
    step_o = parallel.GraphedTrainStep(ours, opt_o, xs[0], forward_kwargs={"uniforms": us}, reassign=re, keep_outputs=True)
    after_ctor = re._state.clone()
    start = [c.detach().clone() for c in ours.Codebooks]
    step_t = parallel.GraphedTrainStep(twin, opt_t, xs[0], forward_kwargs={"uniforms": us})
    losses = (step_o(xs[0]).clone(), step_t(xs[0]).clone())
    torch.cuda.synchronize()
    return dict(ours=ours, twin=twin, re=re, opt_o=opt_o, step_o=step_o, step_t=step_t, xs=xs, us=us, built=built, after_ctor=after_ctor,
                initial=initial, start=start, losses=losses, want=_yardstick(twin, SEED, 0))


def test_constructor_leaves_the_record_and_the_codebooks_as_they_were(pair):
    assert pair["step_o"].post is not None and pair["step_t"].post is not None
    assert torch.equal(pair["built"], pair["after_ctor"]), "GraphedTrainStep's prepare() / warm() moved the count, the generator or a scalar"
    assert [int(v) for v in pair["built"]] == [0, 0, 0, 0, 0, SEED, 0]
    assert all(torch.equal(a, b) for a, b in zip(pair["initial"], pair["start"])), "the warm-up moved a codeword"


def test_one_replay_equals_the_yardstick_on_the_plain_step(pair):
    """The codebooks are, bit for bit, the numpy rule applied to the plain step's codebooks, its post-update `_freqEMA` and the draws of
    the object's snapshot; every other parameter and buffer is bit-equal between the two runs."""
    ours, twin, re = pair["ours"], pair["twin"], pair["re"]
    assert torch.equal(*pair["losses"])
    moved = 0
    for lv, ((new, source, changed), cb) in enumerate(zip(pair["want"], ours.Codebooks)):
        assert _bits_equal(cb, new), f"level {lv}"
        np.testing.assert_array_equal(re.source[lv].cpu().numpy(), source)
        np.testing.assert_array_equal(re.changed[lv].cpu().numpy(), changed)
        moved += int(changed.sum())
        f = twin._quantizer._entropyCoder._freqEMA[lv].detach()
        assert int((f[0] == 0).sum()) > 0 and int((f[1] == 0).sum()) > 0, "no zero survived the update: nothing to refill"
    assert moved > 0
    codebooks = {id(c) for c in ours.Codebooks}
    for (name, a), (_, b) in zip(_named(ours), _named(twin)):
        if id(a) not in codebooks:
            assert torch.equal(a.detach(), b.detach()), name
    out = re.read()
    assert out["count"] == 1 and out["fired"] == 1 and out["moved"] == moved and out["offset"] == 3
    total = sum(c.shape[0] * c.shape[1] for c in ours.Codebooks)
    assert out["Stat/ReAssignProportion"] == float(np.float32(moved) / np.float32(total))


def test_next_replay_and_eager_encode_follow_the_new_codebook(pair, dev):
    """The next replay runs against the moved codebooks: it equals, loss and codes, a plain step freshly built on a copy of the model and
    the optimizer state as the first replay left them.  Then eagerly: `encode` on a probe batch equals ops.vq_assign on a freshly packed
    copy of the codebook."""
    from mcquic_amd import ops, parallel
    ours, xs, us = pair["ours"], pair["xs"], pair["us"]
    fresh = copy.deepcopy(ours)
    opt_f = _sgd(fresh)
    sd = pair["opt_o"].state_dict()
    opt_f.load_state_dict(copy.deepcopy(sd))
    step_f = parallel.GraphedTrainStep(fresh, opt_f, xs[1], forward_kwargs={"uniforms": us}, keep_outputs=True)
    lo, lf = pair["step_o"](xs[1]).clone(), step_f(xs[1]).clone()
    assert torch.equal(lo, lf)
    for a, b in zip(pair["step_o"].outputs[1], step_f.outputs[1]):
        assert torch.equal(a, b)
    assert int(pair["re"].count) == 2 and int(pair["re"].fired) == 2
    pair["step_o"].invalidate()
    ours.eval()
    try:
        probe = xs[1]
        got = ours.encode(probe)
        qin = ours._quantizer.quantizerInputs(ours._encode_latent(probe))[0]
        want = ops.vq_assign(qin, ops.PackedCodebook(ours.Codebooks[0].detach().clone()))
        assert torch.equal(got[0], want)
    finally:
        ours.train()


def test_eager_step_drops_the_packed_codebook(dev):
    """No trainer at all: after an eager `step()` that fires, `encode` sees the moved codebook (the cache is dropped, the version bumped)."""
    import mcquic_amd
    from mcquic_amd import ops
    model, xs, _ = _setup(dev)
    model.eval()
    model.encode(xs[0])                                                 # packs the codebooks
    re = mcquic_amd.CodebookReassign(model, freq=1, seed=SEED)
    want = _yardstick(model, SEED, 0)
    versions = [c._version for c in model.Codebooks]
    re.step()
    assert all(c._version > v for c, v in zip(model.Codebooks, versions))
    assert all(_bits_equal(cb, new) for (new, _, _), cb in zip(want, model.Codebooks)) and int(re.moved) > 0
    got = model.encode(xs[0])
    qin = model._quantizer.quantizerInputs(model._encode_latent(xs[0]))[0]
    assert torch.equal(got[0], ops.vq_assign(qin, ops.PackedCodebook(model.Codebooks[0].detach().clone())))


def test_a_step_the_guard_skips_neither_fires_nor_counts(dev):
    """skip_nonfinite=True and a NaN in the input of a step that would fire: codebooks, count and generator state stay; the next clean
    step fires as if the void one had not happened -- the yardstick on the guarded twin without `reassign`, draws of offset 0."""
    import mcquic_amd
    from mcquic_amd import parallel
    ours, xs, us = _setup(dev)
    twin = copy.deepcopy(ours)
    re = mcquic_amd.CodebookReassign(ours, freq=1, seed=SEED)
    step_o = parallel.GraphedTrainStep(ours, _sgd(ours), xs[0], forward_kwargs={"uniforms": us}, reassign=re, skip_nonfinite=True)
    step_t = parallel.GraphedTrainStep(twin, _sgd(twin), xs[0], forward_kwargs={"uniforms": us}, skip_nonfinite=True)
    before, state = [c.detach().clone() for c in ours.Codebooks], re._state.clone()
    bad = xs[0].clone()
    bad[0, 0, 0, 0] = float("nan")
    step_o(bad)
    step_t(bad)
    assert int(step_o.guard.skipped) == 1
    assert all(torch.equal(a, b.detach()) for a, b in zip(before, ours.Codebooks))
    assert torch.equal(state, re._state)
    step_o(xs[1])
    step_t(xs[1])
    want = _yardstick(twin, SEED, 0)
    assert all(_bits_equal(cb, new) for (new, _, _), cb in zip(want, ours.Codebooks))
    out = re.read()
    assert out["count"] == 1 and out["fired"] == 1 and out["offset"] == 3 and out["moved"] > 0


def test_accumulate_two_is_one_update_and_one_count(dev):
    """accumulate=2, freq=2: two calls of two micro-batches each are two updates -- the first fires ((1 + 1) % 2 == 0), the second does not."""
    import mcquic_amd
    from mcquic_amd import parallel
    ours, xs, us = _setup(dev)
    re = mcquic_amd.CodebookReassign(ours, freq=2, seed=SEED)
    step = parallel.GraphedTrainStep(ours, _sgd(ours), xs[0], forward_kwargs={"uniforms": us}, reassign=re, accumulate=2)
    both = torch.cat(xs)
    step(both)
    assert re.read()["count"] == 1 and re.read()["fired"] == 1
    step(both)
    out = re.read()
    assert out["count"] == 2 and out["fired"] == 1 and out["offset"] == 3


def test_post_graph_holds_exactly_the_two_new_launches(dev, tmp_path):
    """A fresh count of the post graph's kernels (tests/_reassign_names_worker.py under rocprofv3: a plain step, then one with `reassign=`):
    the same kernels plus exactly one launch of each of the two new ones, which the plain step does not hold."""
    import collections
    import csv
    import glob
    import os
    import shutil
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    run = subprocess.run([prof, "--kernel-trace", "--hip-runtime-trace", "-f", "csv", "-d", str(tmp_path), "-o", "reassign", "--",
                          sys.executable, os.path.join(here, "_reassign_names_worker.py")], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]

    def rows(kind):
        files = glob.glob(os.path.join(str(tmp_path), "**", f"*{kind}.csv"), recursive=True)
        assert len(files) == 1, (kind, files)
        with open(files[0]) as f:
            return list(csv.DictReader(f))
    launches = sorted(int(r["Start_Timestamp"]) for r in rows("hip_api_trace") if "GraphLaunch" in r["Function"])
    assert len(launches) >= 8, launches
    seg_plain, _, seg_re, _ = launches[-4:]
    kernels = sorted((int(r["Start_Timestamp"]), r["Kernel_Name"]) for r in rows("kernel_trace") if "copyBuffer" not in r["Kernel_Name"])

    def post_graph(names):
        first = max(i for i, n in enumerate(names) if "sgd_prepare_kernel" in n)
        assert sum("sgd_prepare_kernel" in n for n in names) == 1
        return collections.Counter(names[first:])
    call_plain, call_re = [n for t, n in kernels if seg_plain <= t < seg_re], [n for t, n in kernels if t >= seg_re]
    plain, with_re = post_graph(call_plain), post_graph(call_re)
    print("post graph, plain step:", dict(plain))
    print("post graph, step with reassign:", dict(with_re))
    assert len(call_plain) > 200 and len(call_re) == len(call_plain) + 2, "the segment graphs are the same launches"
    assert not [n for n in plain if "vq_reassign" in n]
    extra = with_re - plain
    assert not (plain - with_re) and sum(extra.values()) == 2, (plain, with_re)
    assert sorted("plan" if "vq_reassign_plan_kernel" in n else "apply" if "vq_reassign_apply_kernel" in n else n for n in extra) == ["apply", "plan"]
