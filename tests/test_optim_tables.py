"""mcquic_amd.optim.chunk_tables without a GPU: the host chunk tables of the whole-model kernels (csrc/tensor_list.h) against a restatement
that asks every element which chunk it is in.  (tests/test_gpu_leaf_ops.py::test_gather_flat builds its tables by hand: the independent
restatement on the device side.)"""


def _brute(sizes, c):
    seen = []                                                 # (tensor, first element of the chunk), once each, in element order
    for i, n in enumerate(sizes):
        for e in range(n):
            entry = (i, e - e % c)
            if not seen or seen[-1] != entry:
                seen.append(entry)
    first_blk = [sum(1 for t, _ in seen if t < i) for i in range(len(sizes) + 1)]
    return [t for t, _ in seen], [f for _, f in seen], first_blk


def test_chunk_tables_match_a_brute_force_restatement():
    from mcquic_amd import _lib, optim
    c = _lib.load().mcq_adam_chunk()
    sizes = [0, 1, c - 1, c, c + 1, 2 * c + 5]
    for case in (sizes, sizes[::-1], []):
        blk_tensor, blk_first, tensor_first_blk = optim.chunk_tables(case)
        want_t, want_f, want_b = _brute(case, c)
        assert (blk_tensor, blk_first, tensor_first_blk) == (want_t, want_f, want_b), case
        assert len(tensor_first_blk) == len(case) + 1 and tensor_first_blk[-1] == len(blk_tensor)
        for i, n in enumerate(case):
            assert tensor_first_blk[i + 1] - tensor_first_blk[i] == (n + c - 1) // c, "a tensor without elements owns no chunk"
