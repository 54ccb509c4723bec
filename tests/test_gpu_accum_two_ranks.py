"""Gradient accumulation under a process group: two ranks (both on cuda:0, gloo: tests/test_gpu_two_ranks.py's arrangement) with
accumulate=2 on one image per micro-batch make the update one process makes with accumulate=4 on the same four micro-batches --
((g0 + g1) / 2 + (g2 + g3) / 2) / 2 against (((g0 + g1) + g2) + g3) / 4: float32 reassociation only; the counts are integers."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(tmp_path, timeout=300):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = tmp_path / "accum.json"
    procs = []
    for rank in range(2):                             # one fresh child process per rank
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_accum_two_rank_worker.py"), str(out)],
                                      env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = []
    try:
        for p in procs:                               # each under its own timeout
            logs.append(p.communicate(timeout=timeout)[0])
    finally:
        for p in procs:                               # (exact PIDs we started; never by pattern)
            if p.poll() is None:
                p.kill()
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)[-4000:]
    return json.load(open(out))


def test_two_ranks_accumulating_two_equal_one_process_accumulating_four(dev, tmp_path):
    r = _run(tmp_path)
    assert r["post_captured"] and r["segments"] == 3 and r["world"] == 2 and r["accumulate"] == 2 and r["solo_world"] == 1, r
    assert r["largest_update"] > 0, r
    assert r["worst_update_rel_err"] < 1.0, r         # (in units of 1e-4 x the update + 4 ulps of the parameter: the segmented step's bar)
    assert r["ema_max_abs_diff"] < 1e-7, r
    assert r["counts_total"] == r["solo_counts_total"] == 4 * 2 * (16 + 4 + 1), r      # all four micro-batches' codes, summed over the ranks
    for a, b in zip(r["solo_losses"], r["mean_rank_losses"]):
        assert abs(a - b) <= 1e-6 * max(1.0, abs(a)), r
