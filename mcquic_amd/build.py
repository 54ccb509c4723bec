"""Build recipe for libmcquic_hip.so (gfx950 only, hipcc; no cmake, no JIT cache -- the .so lives in-tree).

Every source is compiled to its own object (in parallel, only when it or a file it includes changed: hipcc's depfiles) and the objects are linked
into mcquic_amd/libmcquic_hip.so.  Objects live in mcquic_amd/_obj/ (git-ignored)."""
from __future__ import annotations

import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "_obj")
LIB = os.path.join(HERE, "libmcquic_hip.so")
# conv_mfma_kernel's instances are spread over conv_tiles_*.hip / conv_wino32.hip (build section, has their compile
# times); conv_launch.hip and conv_pack.hip hold none, so an edit to the launcher or the pack layout rebuilds in seconds.
SOURCES = ["conv_tiles_128.hip", "conv_wino32.hip", "conv_tiles_41.hip", "conv_tiles_32.hip", "conv_tiles_64.hip", "conv_launch.hip",
           "conv_pack.hip", "conv_wino16.hip", "vq.hip", "vq_rate_map.hip", "rate_activity.hip", "vq_kmeans.hip", "vq_reassign.hip", "vq_cdf.hip", "vq_train.hip", "vq_bwd_mfma.hip", "codebook_cos.hip", "train_ops.hip", "adam.hip",
           "lamb.hip", "sgd.hip", "ema.hip", "schedule.hip", "step_guard.hip", "step_ops.hip", "step_meter.hip", "param_stats.hip", "step_snapshot.hip", "wgrad_rows.hip", "metrics.hip", "msssim_loss.hip", "norm.hip", "augment.hip", "rans.cpp", "rans_dev.hip", "rans_lanes.hip"]
# -ffp-contract=off: element-wise epilogues keep the reference's one-rounding-per-op sequence
#   (e.g. a * sigmoid(b) then + x are two torch kernels in mcquic/nn/blocks.py:286-287).
# -pragma-unroll-threshold: the 128-register epilogue must be fully unrolled or the accumulators spill to scratch.
CFLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-pthread",
          "-mllvm", "-pragma-unroll-threshold=1000000"]
LDFLAGS = ["--offload-arch=gfx950", "-shared", "-fPIC", "-pthread"]


def _includes(path: str):
    """The files `path` includes with quotes (its own headers), resolved against its directory."""
    here = os.path.dirname(path)
    found = re.findall(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', open(path).read(), re.M)
    return [os.path.normpath(os.path.join(here, f)) for f in found]


def conv_files():
    """Every file that holds convolution device code: the conv_* sources and, transitively, the headers they include."""
    todo = [os.path.join(CSRC, s) for s in SOURCES if s.startswith("conv_")]
    seen = set()
    while todo:
        f = todo.pop()
        if f not in seen:
            seen.add(f)
            todo += _includes(f)
    return sorted(seen)


def csrc_sha() -> str:
    """SHA-256 over conv_files() (names + contents): what measurement artefacts about the convolution kernels are stamped with
    (profiles/rNN_pmc.json) so that a number collected on an older kernel can be recognised as stale."""
    import hashlib
    h = hashlib.sha256()
    for f in conv_files():
        h.update(os.path.relpath(f, CSRC).replace(os.sep, "/").encode() + b"\0")
        h.update(open(f, "rb").read())
    return h.hexdigest()


def _obj_of(src: str, objdir: str = OBJ) -> str:
    return os.path.join(objdir, os.path.splitext(src)[0] + ".o")


def _deps(src: str):
    """What the object of `src` was compiled from, as hipcc's depfile of that compilation recorded it (paths relative to csrc/).
    Without that record (a tree that came with the library but without its objects): the source and every header."""
    try:
        text = open(_obj_of(src) + ".d").read()
    except OSError:
        return [os.path.join(CSRC, src), os.path.join(HERE, "..", "include", "mcquic_hip.h")] + \
               [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    names = re.split(r"(?<!\\)\s+", text.replace("\\\n", " ").split(":", 1)[1].strip())       # (make syntax: a space inside a name is "\ ")
    return [os.path.join(CSRC, d.replace("\\ ", " ")) for d in names]


def _newer(deps, t: float) -> bool:
    return any(not os.path.exists(d) or os.path.getmtime(d) > t for d in set(deps) | {os.path.abspath(__file__)})


def _obj_stale(src: str) -> bool:
    o = _obj_of(src)
    return not (os.path.exists(o) and os.path.exists(o + ".d")) or _newer(_deps(src), os.path.getmtime(o))


def _stale() -> bool:
    return not os.path.exists(LIB) or _newer([d for s in SOURCES for d in _deps(s)], os.path.getmtime(LIB))


def build(force: bool = False, verbose: bool = False, extra_flags=(), lib: str = LIB) -> str:
    """Compile csrc/* into mcquic_amd/libmcquic_hip.so with hipcc (cross-compiles without a GPU).  `extra_flags` /
    `lib`: kernel A/B variants (e.g. -DMCQ_PFB=36 into mcquic_amd/variants/...), always compiled from scratch."""
    variant = bool(extra_flags) or lib != LIB
    if not force and not variant and not _stale():
        return LIB
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc not found: libmcquic_hip.so cannot be built")
    objdir = OBJ if not variant else lib + ".obj"
    os.makedirs(objdir, exist_ok=True)

    def compile_one(src: str) -> str:
        o = _obj_of(src, objdir)
        if force or variant or _obj_stale(src):
            cmd = [hipcc] + CFLAGS + list(extra_flags) + ["-MD", "-MF", o + ".d", "-c", src, "-o", o]      # (run in csrc/: the depfile names the project's files relative to it)
            if verbose:
                print(" ".join(cmd), file=sys.stderr)
            subprocess.run(cmd, check=True, cwd=CSRC)
        return o

    with ThreadPoolExecutor(max_workers=min(len(SOURCES), os.cpu_count() or 1, 16)) as pool:
        objs = list(pool.map(compile_one, SOURCES))
    cmd = [hipcc] + LDFLAGS + ["-o", lib + ".tmp"] + objs
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=CSRC)
    os.replace(lib + ".tmp", lib)
    if variant:
        shutil.rmtree(objdir, ignore_errors=True)
    return lib


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
