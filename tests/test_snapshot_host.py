"""CPU: the log-payload entry points' binding and argument checks (every refusal below returns before anything is launched: each pointer is
either NULL or never dereferenced before the check), the workspace queries, and the Python side's refusals that need no device."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mcq_histogram_chunk", "mcq_histogram_workspace_bytes", "mcq_histogram_f32", "mcq_log_distance_f32", "mcq_code_image_u8",
       "mcq_code_image_first_u8", "mcq_snapshot_freq_workspace_bytes", "mcq_snapshot_freq_f32"]


def test_binding_and_abi_number_unchanged():
    from mcquic_amd import _lib
    header = open(os.path.join(ROOT, "include", "mcquic_hip.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SYMBOLS and re.search(r"\b%s\s*\(" % name, header) and getattr(lib, name) is not None
    assert lib.mcq_abi_version() == _lib.ABI_VERSION == 18, "additions only: the header's rule bumps for incompatible changes"
    assert lib.mcq_histogram_chunk() == 4096


def test_histogram_refuses_before_any_launch():
    from mcquic_amd import _lib
    lib = _lib.load()
    E = _lib.MCQ_EINVAL
    p = ctypes.c_void_p(64)

    def call(x=p, n=100, transform=0, bins=64, counts=p, edges=p, stats=p, ws=p):
        return lib.mcq_histogram_f32(x, n, transform, 1e-6, bins, counts, edges, stats, ws, None)

    for null in ("x", "counts", "edges", "stats", "ws"):
        assert call(**{null: None}) == E, null
    for n in (0, -1):
        assert call(n=n) == E
    for bins in (0, -1, 4097):
        assert call(bins=bins) == E
    for transform in (-1, 2):
        assert call(transform=transform) == E
    assert call(ws=ctypes.c_void_p(68)) == E                          # the workspace holds doubles
    assert call(n=(1 << 40) + 1) == _lib.MCQ_ETOOLARGE
    assert lib.mcq_log_distance_f32(None, p, 4, 1e-6, None) == E
    assert lib.mcq_log_distance_f32(p, None, 4, 1e-6, None) == E
    assert lib.mcq_log_distance_f32(p, p, 0, 1e-6, None) == E


def test_histogram_workspace_query():
    from mcquic_amd import _lib
    lib = _lib.load()
    chunk = lib.mcq_histogram_chunk()
    for n, bins in ((0, 64), (-5, 64), (100, 0), (100, 4097), ((1 << 40) + 1, 64)):
        assert lib.mcq_histogram_workspace_bytes(n, bins) == 0
    head = lib.mcq_histogram_workspace_bytes(1, 1) - 24                # four doubles in front, 24 bytes per workgroup
    assert head == 32
    for n, groups in ((1, 1), (chunk, 1), (chunk + 1, 2), (1000 * chunk, 1000), (32 * 32 * 8192, 1024), (1 << 40, 1024)):
        assert lib.mcq_histogram_workspace_bytes(n, 64) == head + 24 * groups
        assert lib.mcq_histogram_workspace_bytes(n, 4096) == head + 24 * groups


def test_code_image_and_freq_refuse_before_any_launch():
    from mcquic_amd import _lib
    lib = _lib.load()
    E = _lib.MCQ_EINVAL
    p = ctypes.c_void_p(64)
    assert lib.mcq_code_image_u8(None, p, p, 1, 1, 1, 1, None) == E
    assert lib.mcq_code_image_u8(p, None, p, 1, 1, 1, 1, None) == E
    assert lib.mcq_code_image_u8(p, p, None, 1, 1, 1, 1, None) == E
    for dims in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, -1)):
        assert lib.mcq_code_image_u8(p, p, p, *dims, None) == E
    assert lib.mcq_code_image_u8(p, ctypes.c_void_p(66), p, 1, 1, 1, 1, None) == E          # 32-bit stores
    for keep in (0, 3):
        assert lib.mcq_code_image_first_u8(p, p, p, 2, 1, 1, 1, keep, None) == E
    m, k = (ctypes.c_int32 * 2)(2, 2), (ctypes.c_int32 * 2)(64, 32)
    ptrs = (ctypes.c_void_p * 2)(64, 64)
    assert lib.mcq_snapshot_freq_workspace_bytes(m, k, 2) == 4 * 4
    assert lib.mcq_snapshot_freq_workspace_bytes(m, k, 0) == 0 and lib.mcq_snapshot_freq_workspace_bytes(None, k, 2) == 0
    assert lib.mcq_snapshot_freq_workspace_bytes(m, k, lib.mcq_vq_max_levels() + 1) == 0
    assert lib.mcq_snapshot_freq_workspace_bytes(m, (ctypes.c_int32 * 2)(64, 0), 2) == 0
    assert lib.mcq_snapshot_freq_f32(None, m, k, 2, p, p, p, None) == E
    assert lib.mcq_snapshot_freq_f32(ptrs, m, k, 2, None, p, p, None) == E
    assert lib.mcq_snapshot_freq_f32(ptrs, m, k, 2, p, None, p, None) == E
    assert lib.mcq_snapshot_freq_f32(ptrs, m, k, 2, p, p, None, None) == E
    assert lib.mcq_snapshot_freq_f32(ptrs, m, k, 0, p, p, p, None) == E
    assert lib.mcq_snapshot_freq_f32((ctypes.c_void_p * 2)(64, None), m, k, 2, p, p, p, None) == E


def test_python_side_refusals():
    from mcquic_amd import Compressor, monitor, ops
    model = Compressor(8, 2, [64, 32, 16])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        monitor.StepSnapshot(model, batch_shape=(2, 3, 64, 64))
    with pytest.raises(ValueError, match="no entropy coder"):
        monitor.StepSnapshot(torch.nn.Linear(2, 2), batch_shape=(2, 3, 64, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.histogram(torch.zeros(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.log_distance(torch.zeros(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.code_image(torch.zeros((1, 1, 2, 2), dtype=torch.int64))
    src = open(os.path.join(ROOT, "mcquic_amd", "monitor.py")).read()
    assert not re.search(r"^\s*(import|from)\s+wandb", src, re.M)
