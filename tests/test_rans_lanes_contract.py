"""The lanes coder's surface without a device: the entry points are declared in the header, bound from it and exported; the device
entry points refuse bad arguments before any launch; the op wrappers refuse CPU tensors; and the `lanes=` argument of compress /
decompress reaches the host lanes coder, keeps the plain path's bytes as they were, and never lets one layout be decoded as the other."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEVICE_ENTRY_POINTS = ("mcq_rans_lanes_encode_dev", "mcq_rans_lanes_decode_dev")
HOST_ENTRY_POINTS = ("mcq_rans_lanes_encode_batch", "mcq_rans_lanes_decode_batch", "mcq_rans_lanes_auto")


def test_the_entry_points_are_declared_bound_and_exported():
    from ctypes import c_int32, c_int64, c_void_p
    from mcquic_amd import _lib, build
    header = open(os.path.join(ROOT, "include", "mcquic_hip.h")).read()
    for name in DEVICE_ENTRY_POINTS + HOST_ENTRY_POINTS:
        assert len(re.findall(rf"\bint(?:32_t)?\s+{name}\s*\(", header)) == 1, name
        assert _lib.SYMBOLS[name][0] is c_int32
    for name in DEVICE_ENTRY_POINTS:
        assert _lib.SYMBOLS[name][1][-1] is c_void_p                        # int mcq_...(..., void* stream)
    enc, dec = (_lib.SYMBOLS[name][1] for name in DEVICE_ENTRY_POINTS)
    assert enc == [c_void_p] * 6 + [c_int32] * 4 + [c_void_p, c_int64, c_void_p, c_void_p, c_void_p]
    assert dec == _lib.SYMBOLS["mcq_rans_decode_dev"][1], "the two decoders take one argument list"
    assert _lib.SYMBOLS["mcq_rans_lanes_auto"][1] == [c_int64]
    assert "rans_lanes.hip" in build.SOURCES
    assert (_lib.MCQ_RANS_LANES_MAX, _lib.MCQ_RANS_LANES_AUTO_SYMBOLS) == (64, 512)
    assert _lib.MCQ_RANS_LANES_MAGIC == int.from_bytes(b"MQL", "little")
    assert _lib.MCQ_RANS_DEV_CHUNK >= 2 * _lib.MCQ_RANS_LANES_MAX + 1 + 64
    lib = _lib.load()
    assert all(hasattr(lib, name) for name in DEVICE_ENTRY_POINTS + HOST_ENTRY_POINTS)
    # the pack kernels are reused through the existing entry point, not copied
    source = open(os.path.join(ROOT, "mcquic_amd", "csrc", "rans_lanes.hip")).read()
    assert "rans_scan_kernel(" not in source and "rans_copy_kernel(" not in source and "mcq_rans_pack_dev" in source


def _encode_args(**change):
    """A full, valid argument list of mcq_rans_lanes_encode_dev over host memory that no launch may ever see."""
    levels = change.pop("nlevels", 2)
    buf = (ctypes.c_int64 * 64)()
    ok = ctypes.addressof(buf)
    ptrs = lambda: (ctypes.c_void_p * levels)(*[ok] * levels)
    ints = lambda v: (ctypes.c_int32 * levels)(*[v] * levels)
    args = dict(codes=ptrs(), cdf=ptrs(), m=ints(2), k=ints(512), hw=ints(100), lanes=ints(0), levels=levels, n=3, level0=0, row_levels=levels,
                scratch=ok, cap=4 * (1 + 128 + 200), sizes=ok, status=ok, stream=None)
    for key, value in change.items():
        args[key] = ints(value) if key in ("m", "k", "hw", "lanes") and isinstance(value, int) else value
    return list(args.values()), buf


def _decode_args(**change):
    levels = 2
    buf = (ctypes.c_int64 * 64)()
    ok = ctypes.addressof(buf)
    ptrs = lambda: (ctypes.c_void_p * levels)(*[ok] * levels)
    ints = lambda v: (ctypes.c_int32 * levels)(*[v] * levels)
    args = dict(blob=ok, blob_bytes=64, offsets=ok, cdf=ptrs(), m=ints(2), k=ints(512), hw=ints(100), levels=levels, n=3, level0=0,
                row_levels=levels, codes=ptrs(), status=ok, stream=None)
    for key, value in change.items():
        args[key] = ints(value) if key in ("m", "k", "hw") and isinstance(value, int) else value
    return list(args.values()), buf


def test_the_device_entry_points_refuse_bad_arguments_before_any_launch():
    from mcquic_amd import _lib
    lib = _lib.load()
    big = _lib.MCQ_RANS_DEV_MAX_SYMBOLS
    einval = [dict(codes=None), dict(cdf=None), dict(m=None), dict(k=None), dict(hw=None), dict(lanes=None), dict(scratch=None), dict(sizes=None),
              dict(status=None), dict(levels=0), dict(levels=_lib.MCQ_VQ_MAX_LEVELS + 1), dict(n=0), dict(level0=-1), dict(row_levels=1),
              dict(cap=8), dict(cap=4 * (1 + 128 + 200) + 2), dict(m=0), dict(k=0), dict(hw=0), dict(k=_lib.MCQ_CDF_MAX_K + 1),
              dict(lanes=3), dict(lanes=128), dict(lanes=-1), dict(lanes=65),
              dict(lanes=64, cap=4 * (2 * 64 + 200)),           # one word short of 4 (1 + 2 W + m hw)
              dict(lanes=1, cap=4 * (2 + 200)),
              dict(scratch=ctypes.addressof((ctypes.c_int64 * 2)()) + 1)]
    for change in einval:
        args, keep = _encode_args(**change)
        assert lib.mcq_rans_lanes_encode_dev(*args) == _lib.MCQ_EINVAL, change
    for change in (dict(n=65536), dict(m=1, hw=big + 1, cap=0x7fffffff0)):
        args, keep = _encode_args(**change)
        assert lib.mcq_rans_lanes_encode_dev(*args) == _lib.MCQ_ETOOLARGE, change
    # auto at 200 symbols is W = 1: a slot of 4 (1 + 2 + 200) bytes would do, one word less would not
    args, keep = _encode_args(cap=4 * (2 + 200))
    assert lib.mcq_rans_lanes_encode_dev(*args) == _lib.MCQ_EINVAL
    einval = [dict(blob=None), dict(offsets=None), dict(cdf=None), dict(m=None), dict(k=None), dict(hw=None), dict(codes=None), dict(status=None),
              dict(levels=0), dict(levels=_lib.MCQ_VQ_MAX_LEVELS + 1), dict(n=0), dict(level0=-1), dict(row_levels=1), dict(blob_bytes=-1),
              dict(m=0), dict(k=0), dict(hw=0), dict(k=_lib.MCQ_CDF_MAX_K + 1)]
    for change in einval:
        args, keep = _decode_args(**change)
        assert lib.mcq_rans_lanes_decode_dev(*args) == _lib.MCQ_EINVAL, change
    for change in (dict(n=65536), dict(m=1, hw=big + 1)):
        args, keep = _decode_args(**change)
        assert lib.mcq_rans_lanes_decode_dev(*args) == _lib.MCQ_ETOOLARGE, change


def test_the_wrappers_refuse_cpu_tensors_and_bad_widths():
    from mcquic_amd import ops
    codes = [torch.zeros((1, 2, 3, 3), dtype=torch.int64)]
    table = torch.tensor([[0, 32768, 65536]] * 2, dtype=torch.int64).to(torch.uint32)
    for lanes in ("auto", 1, 64, [8]):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.rans_encode_dev(codes, [table], lanes=lanes)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rans_decode_dev(torch.zeros(12, dtype=torch.uint8), torch.tensor([0, 12]), [table], [(1, 2, 3, 3)], lanes=True)
    for lanes in (3, 0, 128, -4, True, "wide", 2.0, [8, 8]):
        with pytest.raises(ValueError, match="lanes"):
            ops.rans_encode_dev(codes, [table], lanes=lanes)
    assert ops.rans_lanes_widths("auto", 3) == [0, 0, 0] and ops.rans_lanes_widths([1, "auto", 64], 3) == [1, 0, 64]
    assert ops.RANS_LANES_HEAD == 4 * (1 + 2 * 64)


def _quantizer():
    from mcquic_amd.modules.quantizer import BaseQuantizer

    class Fixed(BaseQuantizer):
        """`encode` / `decode` are the identity on a list of codes: the coder arguments' path without a kernel."""

        def encode(self, x):
            return x

        def decode(self, codes):
            return codes
    q = Fixed(2, [16, 8, 4])
    with torch.no_grad():
        for f in q._entropyCoder._freqEMA:
            f.copy_(torch.rand(f.shape, generator=torch.Generator().manual_seed(1)) ** 4 + 1e-6)
    return q


def _codes(seed=0, n=3, side=32):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, k, (n, 2, side >> lv, (2 * side) >> lv), generator=g) for lv, k in enumerate((16, 8, 4))]


def test_lanes_reach_the_host_coder_and_the_plain_bytes_stay():
    from mcquic_amd.modules.entropyCoder import isLanesStream, lanesAuto
    q = _quantizer()
    codes = _codes(5)
    _, plain, plain_sizes = q.compress(codes)
    _, none, none_sizes = q.compress(codes, lanes=None)
    assert plain == none and plain_sizes == none_sizes
    for lanes in ("auto", 1, 8, 64):
        _, lan, sizes = q.compress(codes, coder="host", lanes=lanes)
        assert sizes == plain_sizes
        direct, _ = q._entropyCoder.compress(codes, lanes=lanes)
        assert lan == direct
        for binary in lan:
            for lv, b in enumerate(binary):
                symbols = codes[lv][0].numel()
                w = lanesAuto(symbols) if lanes == "auto" else lanes
                assert isLanesStream(b) and b[3] == w and len(b) <= 4 * (1 + 2 * w + symbols)
        if lanes == 1:
            assert all(b == b"MQL\x01" + p for bl, bp in zip(lan, plain) for b, p in zip(bl, bp))
        back = q.decompress(lan, sizes, lanes=True)
        assert all(np.array_equal(a.numpy(), b.numpy()) for a, b in zip(back, codes))
        assert all(torch.equal(a, b) for a, b in zip(q._entropyCoder.decompress(lan, sizes, lanes=True), codes))
        with pytest.raises(RuntimeError, match="lanes=True"):
            q.decompress(lan, sizes)
        with pytest.raises(RuntimeError, match="lanes=True"):
            q.decompress(lan, sizes, lanes=False)
    with pytest.raises(RuntimeError, match="truncated or malformed"):
        q.decompress(plain, plain_sizes, lanes=True)
    assert all(torch.equal(a, b) for a, b in zip(q.decompress(plain, plain_sizes, lanes=False), codes))
    assert lanesAuto(codes[0][0].numel()) == 8, "level 0 holds 4096 symbols"
    _, mixed, sizes = q.compress(codes, lanes=[64, "auto", 2])
    assert [b[3] for b in mixed[0]] == [64, 2, 2]
    assert all(torch.equal(a, b) for a, b in zip(q.decompress(mixed, sizes, lanes=True), codes))


def test_bad_lanes_arguments():
    q = _quantizer()
    codes = _codes(2)
    for lanes in (3, 128, 0, "wide", True, [8, 8]):
        with pytest.raises(ValueError, match="lanes"):
            q.compress(codes, lanes=lanes)
    with pytest.raises(ValueError, match="'host' or 'device'"):             # `coder` keeps its two values and its error text
        q.compress(codes, coder="bogus", lanes="auto")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        q.compress(codes, coder="device", lanes="auto")
    _, lan, sizes = q.compress(codes, lanes="auto")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        q.decompress(lan, sizes, coder="device", lanes=True)


def test_a_coder_without_tables_has_no_lanes_layout():
    from mcquic_amd.modules.entropyCoder import VariousMCoder
    q = _quantizer()
    q._entropyCoder = VariousMCoder([2, 2, 2], [16, 8, 4])
    codes = _codes(3)
    _, raw, sizes = q.compress(codes)                                       # the plain calls are as they were
    assert all(torch.equal(a, b) for a, b in zip(q.decompress(raw, sizes), codes))
    with pytest.raises(NotImplementedError, match="lanes"):
        q.compress(codes, lanes="auto")
    with pytest.raises(NotImplementedError, match="lanes"):
        q.decompress(raw, sizes, lanes=True)


def test_the_compressor_takes_the_argument_before_any_kernel():
    import inspect
    from mcquic_amd import Compressor
    from mcquic_amd.modules.entropyCoder import EntropyCoder
    from mcquic_amd.modules.quantizer import UMGMQuantizer
    for fn, default in ((Compressor.compress, None), (UMGMQuantizer.compress, None), (EntropyCoder.compress, None), (EntropyCoder.compressDevice, None),
                        (Compressor.decompress, False), (UMGMQuantizer.decompress, False), (EntropyCoder.decompress, False),
                        (EntropyCoder.decompressDevice, False)):
        assert inspect.signature(fn).parameters["lanes"].default is default, fn.__qualname__
    model = Compressor(8, 2, [16, 8, 4]).eval()
    with pytest.raises(ValueError, match="'host' or 'device'"):
        model.compress(torch.zeros((1, 3, 64, 64)), coder="bogus", lanes="auto")
