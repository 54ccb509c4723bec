"""The device rANS coder's surface without a device: the three entry points are declared in the header and bound from it, the op
wrappers refuse CPU tensors, and the `coder=` argument of compress / decompress leaves the host path's bytes as they were."""
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("mcq_rans_encode_dev", "mcq_rans_pack_dev", "mcq_rans_decode_dev")


def test_the_entry_points_are_declared_bound_and_exported():
    from ctypes import c_int32, c_int64, c_void_p
    from mcquic_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "mcquic_hip.h")).read()
    for name in ENTRY_POINTS:
        assert len(re.findall(rf"\bint\s+{name}\s*\(", header)) == 1, name
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is c_int32 and argtypes[-1] is c_void_p            # int mcq_...(..., void* stream)
    assert _lib.SYMBOLS["mcq_rans_pack_dev"][1] == [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p]
    assert _lib.SYMBOLS["mcq_rans_encode_dev"][1][5:9] == [c_int32] * 4 and _lib.SYMBOLS["mcq_rans_encode_dev"][1][10] is c_int64
    assert "rans_dev.hip" in build.SOURCES
    chunk = _lib.MCQ_RANS_DEV_CHUNK
    assert chunk >= 64 and chunk & (chunk - 1) == 0
    assert (_lib.MCQ_RANS_OK, _lib.MCQ_RANS_BAD_SYMBOL, _lib.MCQ_RANS_BAD_STREAM) == (0, 1, 2)
    lib = _lib.load()                                                       # (raises if the library lacks a declared symbol)
    assert all(hasattr(lib, name) for name in ENTRY_POINTS)
    # the binding comes from the header alone: no second, hand-written copy of the prototypes in the package
    package = os.path.join(ROOT, "mcquic_amd")
    for name in os.listdir(package):
        if name.endswith(".py"):
            assert "mcq_rans_encode_dev.argtypes" not in open(os.path.join(package, name)).read(), name


def test_the_wrappers_refuse_cpu_tensors():
    from mcquic_amd import ops
    codes = [torch.zeros((1, 2, 3, 3), dtype=torch.int64)]
    table = torch.tensor([[0, 32768, 65536]] * 2, dtype=torch.int64).to(torch.uint32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rans_encode_dev(codes, [table])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rans_decode_dev(torch.zeros(8, dtype=torch.uint8), torch.tensor([0, 8]), [table], [(1, 2, 3, 3)])


class _FixedCodes:
    """A quantizer whose `encode` / `decode` are the identity on a list of codes: the coder argument's path without a kernel."""

    @staticmethod
    def make():
        from mcquic_amd.modules.quantizer import BaseQuantizer

        class Fixed(BaseQuantizer):
            def encode(self, x):
                return x

            def decode(self, codes):
                return codes
        return Fixed(2, [16, 8, 4])


def _codes(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, k, (3, 2, 4 >> lv, 8 >> lv), generator=g) for lv, k in enumerate((16, 8, 4))]


def test_an_unknown_coder_is_a_value_error():
    from mcquic_amd import Compressor
    q = _FixedCodes.make()
    with pytest.raises(ValueError, match="bogus"):
        q.compress(_codes(), coder="bogus")
    _, binaries, sizes = q.compress(_codes())
    with pytest.raises(ValueError, match="bogus"):
        q.decompress(binaries, sizes, coder="bogus")
    model = Compressor(8, 2, [16, 8, 4]).eval()
    x = torch.zeros((1, 3, 64, 64))
    with pytest.raises(ValueError, match="'host' or 'device'"):             # before any kernel is asked for
        model.compress(x, coder="bogus")
    with pytest.raises(ValueError, match="'host' or 'device'"):
        model.decompress([], [], coder="bogus")
    from mcquic_amd.validate import validate
    with pytest.raises(ValueError, match="'exact'"):
        validate(model, x, bits="bogus")


def test_the_host_coder_is_the_default_and_gives_the_same_bytes():
    q = _FixedCodes.make()
    with torch.no_grad():
        for f in q._entropyCoder._freqEMA:
            f.copy_(torch.rand(f.shape, generator=torch.Generator().manual_seed(1)) ** 4 + 1e-6)
    codes = _codes(5)
    _, plain, plain_sizes = q.compress(codes)
    _, named, named_sizes = q.compress(codes, coder="host")
    direct, direct_sizes = q._entropyCoder.compress(codes)
    assert plain == named == direct and plain_sizes == named_sizes == direct_sizes
    for back in (q.decompress(plain, plain_sizes), q.decompress(plain, plain_sizes, coder="host")):
        assert all(np.array_equal(a.numpy(), b.numpy()) for a, b in zip(back, codes))


def test_the_device_coder_on_a_cpu_model_raises():
    q = _FixedCodes.make()
    codes = _codes(2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        q.compress(codes, coder="device")
    _, binaries, sizes = q.compress(codes)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        q.decompress(binaries, sizes, coder="device")
