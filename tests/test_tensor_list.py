"""mcquic_amd.tensor_list without a GPU: the host mirror of csrc/tensor_list.h, built on the CPU -- the chunk table against `chunk_tables`,
the flat layout, the pointer buffer's refill rule, and the order of the arguments the entry points take."""
import ctypes

import pytest
import torch

SIZES = [0, 1, 3, 4095, 4096, 4097, 3 * 4096 + 5]


def test_chunk_table_holds_what_chunk_tables_lists():
    from mcquic_amd import optim, tensor_list
    assert optim.chunk_tables is tensor_list.chunk_tables, "`optim.chunk_tables` stays importable"
    blk_t, blk_f, first_blk = tensor_list.chunk_tables(SIZES)
    tb = tensor_list.ChunkTable(SIZES, "cpu")
    assert (tb.sizes, tb.ntensors, tb.nblocks) == (SIZES, len(SIZES), len(blk_t))
    assert tb.numel.dtype == torch.int64 and tb.numel.tolist() == SIZES
    assert tb.blk_tensor.dtype == torch.int32 and tb.blk_tensor.tolist() == blk_t
    assert tb.blk_first.dtype == torch.int64 and tb.blk_first.tolist() == blk_f
    fb = tb.tensor_first_blk
    assert fb.dtype == torch.int32 and fb.tolist() == first_blk and tb.tensor_first_blk is fb, "built once, on first use"
    assert fb.numel() == tb.ntensors + 1 and int(fb[-1]) == tb.nblocks
    assert int(fb[1]) - int(fb[0]) == 0 and 0 not in blk_t, "the empty tensor owns no chunk"


def test_flat_layout_is_aligned_and_disjoint():
    from mcquic_amd.tensor_list import flat_layout
    offs, total = flat_layout(SIZES)
    assert len(offs) == len(SIZES) and all(o % 4 == 0 for o in offs), "16-byte aligned float32 slices"
    for i in range(len(SIZES) - 1):
        assert offs[i] + SIZES[i] <= offs[i + 1], "the slices do not overlap"
    assert total == offs[-1] + (SIZES[-1] + 3) // 4 * 4
    assert flat_layout([0, 0, 0]) == ([0, 0, 0], 0) and flat_layout([]) == ([], 0)


def test_fill_refills_in_place_and_only_on_change():
    from mcquic_amd.tensor_list import TensorList
    sizes = [5, 1, 7]
    n = len(sizes)
    a, b, c = ([torch.zeros(s) for s in sizes] for _ in range(3))
    tl = TensorList(sizes, "cpu", rows=3)
    base = tl.ptrs.data_ptr()
    assert tl.ptrs.dtype == torch.int64 and tl.ptrs.numel() == 3 * n and not tl.ptrs.any()
    tl.fill(a, None, b)
    for t in range(n):                                        # row k of tensor t sits at k * ntensors + t; a None row is zeros
        assert [int(tl.ptrs[k * n + t]) for k in range(3)] == [a[t].data_ptr(), 0, b[t].data_ptr()]
    version = tl.ptrs._version
    tl.fill(a, None, b)
    tl.fill(a)                                                # (the leading rows alone: the ones behind keep what they hold)
    assert tl.ptrs._version == version, "identical addresses: no upload"
    tl.fill(c)
    assert tl.ptrs._version > version and tl.ptrs.data_ptr() == base, "new addresses: the SAME buffer, refilled"
    assert tl.ptrs.tolist() == [t.data_ptr() for t in c] + [0] * n + [t.data_ptr() for t in b]
    version = tl.ptrs._version
    tl.fill(c, None, b)
    assert tl.ptrs._version == version
    for rows in ((a[:2],), (a, b, c, a)):                     # a row of another length, more rows than the buffer has
        with pytest.raises(ValueError):
            tl.fill(*rows)
    assert tl.ptrs._version == version


def test_args_are_the_entry_points_leading_arguments():
    from mcquic_amd import _lib
    from mcquic_amd.tensor_list import TensorList
    lib = _lib.load()
    tl = TensorList(SIZES, "cpu")
    assert tl.ptrs.numel() == 4 * len(SIZES)
    want = (tl.ptrs.data_ptr(), tl.ntensors, tl.numel.data_ptr(), tl.blk_tensor.data_ptr(), tl.blk_first.data_ptr(), tl.nblocks)
    assert tl.args() == want
    assert tl.args(first_blk=True) == want[:5] + (tl.tensor_first_blk.data_ptr(), tl.nblocks)
    for fn, args in ((lib.mcq_adam_step_f32, tl.args()), (lib.mcq_sgd_step_f32, tl.args()), (lib.mcq_ema_update_f32, tl.args()),
                     (lib.mcq_ema_swap_f32, tl.args()), (lib.mcq_lamb_grad_partials_f32, tl.args()),
                     (lib.mcq_lamb_step_f32, tl.args(first_blk=True))):
        assert len(args) == (7 if fn is lib.mcq_lamb_step_f32 else 6)
        for value, ctype in zip(args, fn.argtypes):           # the int32 counts where the ABI has them, addresses everywhere else
            assert ctype in (ctypes.c_int32, ctypes.c_void_p)
            assert (ctype is ctypes.c_int32) == (value in (tl.ntensors, tl.nblocks)), (fn.__name__, ctype, value)
    assert [lib.mcq_lamb_step_f32.argtypes[i] for i in (1, 6)] == [ctypes.c_int32] * 2
    assert [lib.mcq_adam_step_f32.argtypes[i] for i in (1, 5)] == [ctypes.c_int32] * 2
