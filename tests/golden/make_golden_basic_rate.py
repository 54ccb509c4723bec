#!/usr/bin/env python3
"""Capture F18 (tests/golden/f18_basic_rate.npz): the codebook regulariser of the REAL reference, `BasicRate`
(mcquic/loss/__init__.py:27-44), imported unmodified from the reference tree through oracle/ref_harness and run on CPU autograd
in float32 and in float64.  Runs only where the reference tree is; the output is data (seeds, shapes, losses, gradient samples,
error figures).

    python tests/golden/make_golden_basic_rate.py

Inputs: `tests/_cosine_ref.make_codebook(m, k, d, seed)`, one level.  Stored:
    cases [n, 5]           (m, k, d, seed, with_grad)
    gamma                  the BasicRate gamma of every case
    loss32_i, loss64_i     the reference's value in float32 / float64 (the 8192 case: float64 from the chunked sum of
                           tests/_cosine_ref, the [k, k] float64 planes of the formula being 512 MiB each)
    lossrel32_i            |loss32 - loss64| / |loss64|: the reference's own float32 error
    rows32_i, rows64_i     d loss / d codebook, group 0, the first SAMPLE_ROWS codewords (cases with a gradient)
    graderr32_i            the reference's own float32 gradient error in the tests' metric (tests/_cosine_ref.grad_error: largest
                           per-row deviation beyond the ambiguous pairs' allowance, over the largest gradient element)
"""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from oracle import ref_harness              # noqa: E402
import _cosine_ref as R                     # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
GAMMA = 0.25
SAMPLE_ROWS = 8
F18_CASES = [(1, 2, 1, 0, 1), (1, 5, 3, 0, 1), (2, 33, 16, 0, 1), (1, 64, 64, 0, 1), (3, 127, 8, 0, 1), (2, 130, 64, 0, 1), (1, 257, 32, 1, 1),
             (1, 7, 3, 0, 1), (1, 64, 256, 0, 1), (2, 2048, 64, 0, 1), (2, 8192, 64, 0, 0)]


def reference_basic_rate():
    ref_harness.load_validate_handlers()                       # (mcquic.validate as a shell package; metrics / utils import from it)
    if "mcquic.utils" not in sys.modules:
        ref_harness._pkg("mcquic.utils", ref_harness.REF + "/mcquic/utils")
    return importlib.import_module("mcquic.loss").BasicRate


def main():
    BasicRate = reference_basic_rate()
    rate = BasicRate(GAMMA)
    f18 = {"cases": np.array(F18_CASES, dtype=np.int64), "gamma": np.array([GAMMA])}
    for i, (m, k, d, seed, with_grad) in enumerate(F18_CASES):
        cb = R.make_codebook(m, k, d, seed)
        ref = R.cosine_ref(cb, want_grad=bool(with_grad))
        if with_grad:
            out = {}
            for tag, dt in (("32", torch.float32), ("64", torch.float64)):
                c = cb.to(dt).clone().requires_grad_()
                loss = rate(None, [c])
                loss.backward()
                out[tag] = (float(loss), c.grad)
                f18[f"rows{tag}_{i}"] = c.grad[0, :SAMPLE_ROWS].numpy()
            loss32, loss64 = out["32"][0], out["64"][0]
            f18[f"graderr32_{i}"] = np.array([R.grad_error(out["32"][1], ref, GAMMA)[0]])
            assert R.grad_error(out["64"][1], ref, GAMMA)[0] < 1e-12 and R.loss_error(loss64, GAMMA * ref.loss) < 1e-12
        else:
            with torch.no_grad():
                loss32 = float(rate(None, [cb]))
            loss64 = GAMMA * ref.loss
        f18[f"loss32_{i}"], f18[f"loss64_{i}"] = np.array([loss32]), np.array([loss64])
        f18[f"lossrel32_{i}"] = np.array([R.loss_error(loss32, loss64)])
        print(f"case {i} {(m, k, d, seed)}: loss64 {loss64:.12g} rel32 {f18[f'lossrel32_{i}'][0]:.3e} "
              f"graderr32 {f18.get(f'graderr32_{i}', [float('nan')])[0]:.3e} ambiguous {ref.n_ambiguous} rows {ref.ambiguous_rows:.4f}")
    path = os.path.join(OUT, "f18_basic_rate.npz")
    np.savez_compressed(path, **f18)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
