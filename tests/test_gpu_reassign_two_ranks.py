"""Two ranks, one GPU, gloo (the pattern of tests/test_gpu_two_ranks.py): parallel.GraphedTrainStep(segments=3, reassign=...) with
freq=2 over four steps.  The reference reassigns on rank 0 and broadcasts (`syncCodebook`); here every rank holds the same all-reduced
frequencies, the same codebooks and the same generator state, so each makes the same moves on its own: after every step the ranks'
codebooks are bit-equal, and the collectives issued while the steps ran are the step's own all-reduces -- no broadcast, no barrier."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_two_ranks_make_the_same_moves_without_a_broadcast(dev, tmp_path):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out = tmp_path / "reassign.json"
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="4")
        procs.append(subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "_reassign_two_rank_worker.py"), str(out)],
                                      env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = []
    try:
        for p in procs:
            logs.append(p.communicate(timeout=300)[0])
    finally:
        for p in procs:                               # (exact PIDs we started; never by pattern)
            if p.poll() is None:
                p.kill()
    assert all(p.returncode == 0 for p in procs), "\n".join(logs)[-4000:]
    r = json.load(open(out))
    assert r["segments"] == 3 and r["post_captured"], r
    rows = r["rows"]
    assert [row["equal"] for row in rows] == [True] * 4, rows
    assert [row["count"] for row in rows] == [1, 2, 3, 4]
    assert [row["fired"] for row in rows] == [1, 1, 2, 2], rows      # (s + 1) % 2 == 0: the completed counts 1 and 3
    assert rows[0]["moved"] > 0 and rows[2]["moved"] > 0, rows
    assert all(row["seed"] == 5 for row in rows) and [row["offset"] for row in rows] == [3, 3, 6, 6]      # rank 0's seed on both
    assert r["records_equal"]
    # the steps' own collectives: per step one all-reduce per segment slice and one of the code counts; nothing for the reassignment
    assert r["calls"] == {"all_reduce": 16, "broadcast": 0, "barrier": 0, "all_gather": 0}, r["calls"]
