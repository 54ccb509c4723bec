"""ctypes binding of libmcquic_hip.so, derived from include/mcquic_hip.h when this module is imported.

The header is the only copy of the C-ABI: `_abi.read` turns its prototypes into SYMBOLS, its structs into ctypes
Structures (mcq_conv_desc -> ConvDesc, mcq_lr_schedule -> LrSchedule) and its `#define MCQ_X <integer>` lines into
module attributes.  A new entry point is declared in the header, with MCQ_ABI_VERSION bumped; there is no second place.

There is no fallback: if the shared library is missing or a symbol is absent, importing the op layer
raises.  The product path never routes through a CPU or PyTorch implementation of these ops.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_int32

from . import _abi

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MCQUIC_AMD_LIB") or os.path.join(HERE, "libmcquic_hip.so")   # override: kernel A/B experiments
HEADER = os.path.join(HERE, "..", "include", "mcquic_hip.h")

try:
    with open(HEADER) as _f:
        CONSTANTS, STRUCTS, SYMBOLS = _abi.read(_f.read())     # once per process: the module is the memo
except OSError as e:
    raise ImportError(f"{HEADER} is missing: mcquic_amd runs from a checkout and takes its binding from that header") from e

# every MCQ_X under its own name; the conv flags, the schedule kinds / modes and the augment columns also without the prefix
# (CONV_SILU_IN, LR_COSINE, AUG_TOP); the structs under their Python names
globals().update(CONSTANTS)
globals().update({k[4:]: v for k, v in CONSTANTS.items() if k.startswith(("MCQ_CONV_", "MCQ_LR_", "MCQ_AUG_"))})
globals().update({s.__name__: s for s in STRUCTS.values()})
# (bound above already; spelled out for the reader and the linter because this module uses them itself)
MCQ_OK, MCQ_EINVAL, MCQ_ELAUNCH, MCQ_ETOOLARGE = (CONSTANTS[k] for k in ("MCQ_OK", "MCQ_EINVAL", "MCQ_ELAUNCH", "MCQ_ETOOLARGE"))
ABI_VERSION = CONSTANTS["MCQ_ABI_VERSION"]     # the name the rest of the package and load() know the header's version by

_ERR = {MCQ_EINVAL: "MCQ_EINVAL (invalid argument)", MCQ_ELAUNCH: "MCQ_ELAUNCH (kernel launch failed)",
        MCQ_ETOOLARGE: "MCQ_ETOOLARGE (tensor exceeds the addressing window)"}

_lib = None


def load() -> ctypes.CDLL:
    """dlopen the in-tree library and type every entry point; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: run `python -m mcquic_amd.build` (or __graft_entry__.build()). "
            "mcquic_amd has no CPU / PyTorch fallback for its HIP kernels.")
    lib = ctypes.CDLL(LIB_PATH)
    try:
        lib.mcq_abi_version.restype = c_int32
        built = int(lib.mcq_abi_version())
    except AttributeError:
        built = None
    if built != ABI_VERSION:        # a stale .so under these prototypes would misalign arguments silently
        raise ImportError(f"{LIB_PATH} was built for ABI version {built}, this binding needs {ABI_VERSION}: "
                          "rebuild with `python -m mcquic_amd.build --force`")
    for name, (restype, argtypes) in SYMBOLS.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = lib
    return lib


def check(status: int, what: str) -> None:
    if status != MCQ_OK:
        raise RuntimeError(f"{what} failed: {_ERR.get(status, status)}")
