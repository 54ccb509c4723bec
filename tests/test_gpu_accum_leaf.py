"""GPU: the two kernels of gradient accumulation, alone, against tests/_accum_ref.py bit for bit (tests/test_accum_ref.py holds that
reference to its definition on the CPU and shows that another summation order, or the mean rounded once, differs on these inputs).

mcq_gather_accum_flat_f32 moves its destination in 128-bit pieces between a scalar head and tail, and a tensor's slice of the flat
buffer is only 4-byte aligned: the list below puts a tensor at every destination alignment mod 16 bytes, on both sides of a chunk, with
sources at every alignment of their own, and guard bands before, between and after the slices."""
import ctypes
import types

import pytest
import torch

import _accum_ref as A

pytestmark = pytest.mark.gpu

GUARD = 7.5


def _bits(t):
    return t.contiguous().view(torch.int32)


def _layout(chunk):
    """(sizes, offsets into the flat buffer, its length): two densely packed groups, a band of 5 floats in front (so the buffer's own
    alignment is not the slices'), 7 between the groups and 9 behind."""
    a = [1, 3, chunk - 1, chunk, chunk + 1, 2 * chunk + 3]
    b = [3, chunk + 1, 1, 2 * chunk + 3, chunk - 1, chunk]
    sizes, offs, at = [], [], 5
    for group in (a, b):
        for n in group:
            sizes.append(n)
            offs.append(at)
            at += n
        at += 7
    return sizes, offs, at + 2


def _tables(sizes, offs, chunk, dev):
    """The chunk tables by hand, as parallel.GraphedTrainStep's are laid out (one (tensor, first element) entry per chunk)."""
    blk_t, blk_f = [], []
    for i, n in enumerate(sizes):
        for first in range(0, n, chunk):
            blk_t.append(i)
            blk_f.append(first)
    table = types.SimpleNamespace(numel=torch.tensor(sizes, dtype=torch.int64).to(dev), blk_tensor=torch.tensor(blk_t, dtype=torch.int32).to(dev),
                                  blk_first=torch.tensor(blk_f, dtype=torch.int64).to(dev), nblocks=len(blk_t))
    return table, torch.tensor(offs, dtype=torch.int64).to(dev)


@pytest.mark.parametrize("k", [2, 3, 4])
def test_gather_accum_flat_every_phase(dev, k):
    from mcquic_amd import _lib, ops
    chunk = _lib.load().mcq_adam_chunk()
    sizes, offs, total = _layout(chunk)
    assert {o % 4 for o in offs} == {0, 1, 2, 3}, "a destination alignment mod 16 bytes is missing"
    table, offs_d = _tables(sizes, offs, chunk, dev)
    assert table.nblocks > len(sizes)                                     # (more than one workgroup per tensor somewhere)
    # micro-step j's sources: tensor i is a view that starts shift[i] floats into its allocation (1, 2, 3: misaligned views `base[s:]`)
    shift = [0, 1, 2, 3, 0, 3, 2, 3, 0, 0, 2, 3]
    host = [[A.hard_values(n, 1000 * j + 10 * i + k) for i, n in enumerate(sizes)] for j in range(k)]
    bases = [[torch.cat([torch.zeros(shift[i]), h]).to(dev) for i, h in enumerate(row)] for row in host]
    srcs = [[b[shift[i]:] for i, b in enumerate(row)] for row in bases]
    assert any(s.data_ptr() % 16 == 4 for s in srcs[0]) and all(s.is_contiguous() for row in srcs for s in row)
    assert {(s.data_ptr() // 4 - o) % 4 for s, o in zip(srcs[0], offs)} == {0, 1, 2, 3}       # source against destination: every relative alignment
    flat = torch.full((total,), GUARD, device=dev)
    inside = torch.zeros(total, dtype=torch.bool)
    for n, o in zip(sizes, offs):
        inside[o: o + n] = True
        flat[o: o + n] = float("nan")                                     # phase 0 must not read what the buffer held
    assert flat.data_ptr() % 16 == 0
    phase = torch.zeros(1, dtype=torch.int32, device=dev)
    want = [None] * len(sizes)
    for j in range(k):
        phase.fill_(j)
        ptrs = torch.tensor([s.data_ptr() for s in srcs[j]], dtype=torch.int64).to(dev)
        ops.gather_accum_flat_(ptrs, flat, offs_d, table, phase, k)
        torch.cuda.synchronize()
        got = flat.cpu()
        for i, (n, o) in enumerate(zip(sizes, offs)):
            want[i] = A.accum(want[i], host[j][i], j, k)
            assert torch.equal(_bits(got[o: o + n]), _bits(want[i])), (k, j, i, n, o)
        assert bool((got[~inside] == GUARD).all()), "written outside the slices"
    big = sizes.index(2 * chunk + 3)
    gs = [host[j][big] for j in range(k)]
    assert bool((gs[0].view(torch.int32) == 1).any()) and bool((gs[0] == 0).any())       # the smallest denormal, zeros
    if k > 2:                                                                              # (k = 2 has one add: no order to tell)
        assert not torch.equal(_bits(want[big]), _bits(A.mean_rounded_once(gs)))           # these inputs tell the rule from the once-rounded mean
        assert not torch.equal(_bits(want[big]), _bits(A.accum_all(gs[::-1])))             # ... and from another order
    # the sources are only read
    for row_h, row_d in zip(host, srcs):
        assert all(torch.equal(_bits(h), _bits(d.cpu())) for h, d in zip(row_h, row_d))


def test_same_tensor_twice_is_the_tensor(dev):
    """k = 2 on the same sources: bit for bit the sources (+-0 and denormals included) -- what lets a step with accumulate=2 on a repeated
    micro-batch equal the plain step."""
    from mcquic_amd import _lib, ops
    chunk = _lib.load().mcq_adam_chunk()
    sizes, offs, total = _layout(chunk)
    table, offs_d = _tables(sizes, offs, chunk, dev)
    host = [A.hard_values(n, 77 + i) for i, n in enumerate(sizes)]
    srcs = [h.to(dev) for h in host]
    ptrs = torch.tensor([s.data_ptr() for s in srcs], dtype=torch.int64).to(dev)
    flat = torch.full((total,), GUARD, device=dev)
    phase = torch.zeros(1, dtype=torch.int32, device=dev)
    for j in range(2):
        phase.fill_(j)
        ops.gather_accum_flat_(ptrs, flat, offs_d, table, phase, 2)
    got = flat.cpu()
    for h, n, o in zip(host, sizes, offs):
        assert torch.equal(_bits(got[o: o + n]), _bits(h))


def test_bad_arguments_are_refused(dev):
    from mcquic_amd import _lib, ops
    lib = _lib.load()
    chunk = lib.mcq_adam_chunk()
    table, offs_d = _tables([8], [0], chunk, dev)
    src, flat = torch.ones(8, device=dev), torch.zeros(8, device=dev)
    ptrs = torch.tensor([src.data_ptr()], dtype=torch.int64).to(dev)
    phase = torch.zeros(1, dtype=torch.int32, device=dev)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    good = [ptrs.data_ptr(), flat.data_ptr(), offs_d.data_ptr(), table.numel.data_ptr(), table.blk_tensor.data_ptr(), table.blk_first.data_ptr(), 1,
            phase.data_ptr(), 2, stream]
    assert lib.mcq_gather_accum_flat_f32(*(good[:8] + [1, stream])) == _lib.MCQ_EINVAL                  # k = 1: callers use the copy kernel
    for at in (0, 1, 2, 3, 4, 5, 7):
        bad = list(good)
        bad[at] = None
        assert lib.mcq_gather_accum_flat_f32(*bad) == _lib.MCQ_EINVAL, at
    counts, acc, loss, lacc = (torch.ones(8, dtype=torch.int64, device=dev), torch.zeros(8, dtype=torch.int64, device=dev),
                               torch.ones((), device=dev), torch.zeros((), device=dev))
    assert lib.mcq_accum_step_scalars(counts.data_ptr(), acc.data_ptr(), 8, loss.data_ptr(), lacc.data_ptr(), phase.data_ptr(), 1, stream) == _lib.MCQ_EINVAL
    assert lib.mcq_accum_step_scalars(counts.data_ptr(), acc.data_ptr(), 8, loss.data_ptr(), lacc.data_ptr(), None, 2, stream) == _lib.MCQ_EINVAL
    assert lib.mcq_accum_step_scalars(counts.data_ptr(), None, 8, loss.data_ptr(), lacc.data_ptr(), phase.data_ptr(), 2, stream) == _lib.MCQ_EINVAL
    assert lib.mcq_accum_step_scalars(None, None, 0, None, None, phase.data_ptr(), 2, stream) == _lib.MCQ_EINVAL
    torch.cuda.synchronize()
    assert bool((flat == 0).all()) and bool((acc == 0).all()) and float(lacc) == 0.0                   # nothing was launched
    with pytest.raises(ValueError):
        ops.gather_accum_flat_(ptrs, flat, offs_d, table, phase, 1)
    with pytest.raises(ValueError):
        ops.accum_step_scalars_(counts, acc, loss, lacc, phase, 1)
    with pytest.raises(ValueError):
        ops.accum_step_scalars_(counts, acc[:4], loss, lacc, phase, 2)


@pytest.mark.parametrize("k", [2, 3, 4])
def test_step_scalars(dev, k):
    """Counts up to 2^40 per micro-step sum exactly (more entries than one pass of the grid covers, not a multiple of the block); the loss
    follows the gradients' rule; the bands around the accumulator keep their bits; either half alone works."""
    from mcquic_amd import ops
    n, band = 1024 * 256 + 77, 5
    gen = torch.Generator().manual_seed(40 + k)
    cs = [torch.randint(0, (1 << 40) + 1, (n,), generator=gen, dtype=torch.int64) for _ in range(k)]
    for c in cs:
        c[-1] = 1 << 40
    ls = [torch.rand((), generator=gen) * 3 for _ in range(k)]
    buf = torch.full((n + 2 * band,), -12345, dtype=torch.int64, device=dev)
    acc = buf[band: band + n]
    lbuf = torch.full((3,), float("nan"), device=dev)
    lacc = lbuf[1:2].view(())
    only = torch.full((n,), -1, dtype=torch.int64, device=dev)
    lonly = torch.full((), float("nan"), device=dev)
    phase = torch.zeros(1, dtype=torch.int32, device=dev)
    want_c, want_l = None, None
    for j in range(k):
        phase.fill_(j)
        c, l = cs[j].to(dev), ls[j].to(dev)
        ops.accum_step_scalars_(c, acc, l, lacc, phase, k)
        ops.accum_step_scalars_(c, only, None, None, phase, k)
        ops.accum_step_scalars_(None, None, l, lonly, phase, k)
        torch.cuda.synchronize()
        want_c, want_l = A.accum_counts(want_c, cs[j], j), A.accum(want_l, ls[j], j, k)
        assert torch.equal(acc.cpu(), want_c) and torch.equal(only.cpu(), want_c), (k, j)
        assert torch.equal(_bits(lacc.cpu()), _bits(want_l)) and torch.equal(_bits(lonly.cpu()), _bits(want_l)), (k, j)
    assert int(want_c[-1]) == k << 40
    got = buf.cpu()
    assert bool((got[:band] == -12345).all()) and bool((got[-band:] == -12345).all())
    assert bool(torch.isnan(lbuf[0])) and bool(torch.isnan(lbuf[2]))
