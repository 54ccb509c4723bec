"""CPU: the k-means reference against a hand-computed case; the new entry points' argument checks and the ABI version."""
import ctypes
import os
import re

import numpy as np

import _kmeans_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_against_a_hand_computed_case():
    """m = 1, d = 2, five vectors on a 1 x 5 map, k = 3: code 1 stays empty, vector 3 carries the out-of-range code 7."""
    x = np.array([[1, 2], [3, 4], [-1, 0.5], [2, 2], [10, 10]], np.float32).T.reshape(1, 2, 1, 5)
    codes = np.array([0, 2, 0, 7, 2], np.int64).reshape(1, 1, 1, 5)
    sums, sqsums, counts = R.accumulate(x, codes, R.new_acc(1, 3, 2))
    assert sums.tolist() == [[[0.0, 2.5], [0.0, 0.0], [13.0, 14.0]]]
    assert sqsums.tolist() == [[6.25, 0.0, 225.0]]
    assert counts.tolist() == [[2, 0, 2]]
    old = np.array([[[0, 1], [5, 5], [6, 7]]], np.float32)
    new, inertia, empty = R.update(old, (sums, sqsums, counts))
    assert new.dtype == np.float32 and new.tolist() == [[[0.0, 1.25], [5.0, 5.0], [6.5, 7.0]]]
    # |v0 - (0,1)|^2 + |v2 - (0,1)|^2 = 2 + 1.25; |v1 - (6,7)|^2 + |v4 - (6,7)|^2 = 18 + 25
    assert inertia.tolist() == [46.25] and empty.tolist() == [1]
    # a second batch adds on
    R.accumulate(x, codes, (sums, sqsums, counts))
    assert counts.tolist() == [[4, 0, 4]] and sums[0, 2].tolist() == [26.0, 28.0]
    u = np.array([0.0, 0.5, (2 ** 24 - 1) / 2 ** 24], np.float32)
    assert R.picks(u, 5).tolist() == [0, 2, 4]
    assert R.picks(np.array([0.999], np.float32), 1).tolist() == [0]
    seeded = R.seed(x, old, u, counts=np.array([[2, 0, 2]]))
    assert seeded.tolist() == [[[0.0, 1.0], [-1.0, 0.5], [6.0, 7.0]]]
    assert R.seed(x, old, u).tolist() == [[[1.0, 2.0], [-1.0, 0.5], [10.0, 10.0]]]


def test_invalid_arguments_return_einval_without_a_device():
    from mcquic_amd import _lib
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)                       # a non-null host address: never dereferenced before the checks fail
    p = ctypes.addressof(buf)
    E = _lib.MCQ_EINVAL
    good = dict(N=1, m=1, d=2, h=1, w=5, k=3)

    def acc(ptrs=(p,) * 5, **kw):
        a = {**good, **kw}
        return lib.mcq_vq_kmeans_accumulate_f32(*ptrs, a["N"], a["m"], a["d"], a["h"], a["w"], a["k"], None)

    def upd(ptrs=(p,) * 6, **kw):
        a = {**good, **kw}
        return lib.mcq_vq_kmeans_update_f32(*ptrs, a["m"], a["k"], a["d"], None)

    def seed(ptrs=(p, p, None, p), **kw):
        a = {**good, **kw}
        return lib.mcq_vq_kmeans_seed_f32(*ptrs, a["N"], a["m"], a["d"], a["h"], a["w"], a["k"], None)

    for i in range(5):
        assert acc(ptrs=tuple(None if j == i else p for j in range(5))) == E
    for i in range(6):
        assert upd(ptrs=tuple(None if j == i else p for j in range(6))) == E
    for i in (0, 1, 3):                                          # (argument 2, the counts, may be NULL)
        assert seed(ptrs=tuple(None if j == i else q for j, q in enumerate((p, p, p, p)))) == E
    for name in good:
        for bad in (0, -1):
            assert acc(**{name: bad}) == E
            assert seed(**{name: bad}) == E
            if name in ("m", "k", "d"):
                assert upd(**{name: bad}) == E
                assert lib.mcq_vq_kmeans_zero(p, p, p, *[bad if n == name else 1 for n in ("m", "k", "d")], None) == E
    for i in range(3):
        assert lib.mcq_vq_kmeans_zero(*[None if j == i else p for j in range(3)], 1, 1, 1, None) == E


def test_abi_version_matches_the_header():
    from mcquic_amd import _lib
    header = open(os.path.join(ROOT, "include", "mcquic_hip.h")).read()
    declared = int(re.search(r"#define\s+MCQ_ABI_VERSION\s+(\d+)", header).group(1))
    assert _lib.load().mcq_abi_version() == declared == _lib.ABI_VERSION
    assert declared >= 11                                        # the k-means entries arrived with 11
    for name in ("mcq_vq_kmeans_zero", "mcq_vq_kmeans_accumulate_f32", "mcq_vq_kmeans_update_f32", "mcq_vq_kmeans_seed_f32"):
        assert name in _lib.SYMBOLS and re.search(r"\b%s\s*\(" % name, header)
