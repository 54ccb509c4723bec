"""parallel.GraphedTrainStep(..., keep_outputs=True).snapshot(snap), on the model and shards of tests/test_gpu_ema_step.py: Compressor(32, 2,
[64, 32, 16]), two 64 x 64 images, fixed uniforms, mcquic_amd.optim.SGD.  The payload is the references' from the step's own static tensors; the
step that keeps its outputs is the step that does not, bit for bit; and a replay launches, name for name, what a step launches that was
never shown a snapshot (a fresh child process under rocprofv3, as the other names workers)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
LR = 1e-2


def _step(dev, keep):
    from mcquic_amd import optim, parallel
    from test_gpu_ema_step import _setup
    model, xs, us = _setup(dev)
    extra = {"keep_outputs": True} if keep else {}
    step = parallel.GraphedTrainStep(model, optim.SGD(model.parameters(), lr=LR, momentum=0.9), xs[0], forward_kwargs={"uniforms": us},
                                     max_grad_norm=4.0, **extra)
    return model, xs, step


def test_payload_of_the_last_replay(dev):
    from mcquic_amd import monitor
    from test_gpu_ema_step import HW, N
    from test_gpu_step_snapshot import check_payload
    import test_gpu_step_snapshot as S
    model, xs, step = _step(dev, True)
    snap = monitor.StepSnapshot(model, batch_shape=(N, 3, HW, HW), bins=64, images=1)
    losses = [step(xs[0]).clone(), step(xs[1]).clone()]
    payload = step.snapshot(snap)
    xHat, codes, logits0 = step.outputs
    assert torch.equal(step.x, xs[1]), "the static input holds the last batch"
    assert tuple(logits0.shape) == (N, 2, 4, 4, 64) and [tuple(c.shape) for c in codes] == [(N, 2, 4, 4), (N, 2, 2, 2), (N, 2, 1, 1)]
    assert (S.KS, S.HW, S.N) == ([64, 32, 16], HW, N), "check_payload's constants are this model's"
    step.invalidate()
    check_payload(payload, snap, model, step.x, xHat, codes, [logits0], 1)
    # the kept reconstruction is the last replay's: its distortion is the loss the replay returned
    assert float(((xHat - step.x) ** 2).mean()) == pytest.approx(float(losses[1]), rel=1e-5)
    again = step.snapshot(snap)                                # nothing moved in between: the same bits
    flat = lambda p: b"".join(np.asarray(a).tobytes() for v in p.values() for a in (v if isinstance(v, tuple) else (v,)))
    assert flat(payload) == flat(again)
    # and the step that keeps its outputs trains as the one that does not
    model_b, xs_b, plain = _step(dev, False)
    assert plain.outputs is None
    with pytest.raises(RuntimeError, match="keep_outputs=True"):
        plain.snapshot(snap)
    losses_b = [plain(xs_b[0]).clone(), plain(xs_b[1]).clone()]
    assert torch.equal(torch.stack(losses), torch.stack(losses_b))
    assert all(torch.equal(p.detach(), q.detach()) for p, q in zip(model.parameters(), model_b.parameters()))
    step.close(); plain.close()


def test_replay_launches_what_a_step_without_a_snapshot_launches(dev, tmp_path):
    """A kernel trace of the last replay of two steps (tests/_snapshot_names_worker.py under rocprofv3): one built as before, one with
    `keep_outputs=True` after a `snapshot`.  The two name lists are equal, and none of the snapshot's kernels is in either."""
    import csv
    import glob
    import shutil
    import subprocess
    import sys
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    run = subprocess.run([prof, "--kernel-trace", "--hip-runtime-trace", "-f", "csv", "-d", str(tmp_path), "-o", "snap", "--",
                          sys.executable, os.path.join(HERE, "_snapshot_names_worker.py")], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]

    def rows(what):
        files = glob.glob(os.path.join(str(tmp_path), "**", f"*{what}.csv"), recursive=True)
        assert len(files) == 1, (what, files)
        with open(files[0]) as f:
            return list(csv.DictReader(f))
    launches = sorted(int(r["Start_Timestamp"]) for r in rows("hip_api_trace") if "GraphLaunch" in r["Function"])
    assert len(launches) >= 8, launches
    cuts = launches[-4:][::2] + [float("inf")]                # the segment graph's launch of each of the last two calls
    kernels = sorted((int(r["Start_Timestamp"]), r["Kernel_Name"]) for r in rows("kernel_trace") if "copyBuffer" not in r["Kernel_Name"])
    plain, kept = ([n for t, n in kernels if cuts[i] <= t < cuts[i + 1]] for i in range(2))
    everything = [n for _, n in kernels]
    mine = ("hist_", "code_max_kernel", "code_image_kernel", "snap_freq_kernel", "snap_usage_kernel")
    assert any(any(m in n for m in mine) for n in everything), "the worker did take a snapshot"
    assert len(plain) > 50 and any("gather_flat_kernel" in n for n in plain) and any("meter_commit_kernel" in n for n in plain)
    assert plain == kept, [(a, b) for a, b in zip(plain, kept) if a != b][:5]
    assert not [n for n in plain + kept if any(m in n for m in mine)]
