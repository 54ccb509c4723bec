"""tests/_cdf_ref.py (the numpy restatement the device tables are compared with) against the library's host function
`pmfToQuantizedCDF`, which tests/test_entropy_coder.py pins to the reference's compiled coder.  No GPU."""
import numpy as np
import pytest

import _cdf_ref as C


@pytest.mark.parametrize("name", sorted(C.cases()))
def test_numpy_table_rule_equals_the_host_function(name):
    from mcquic_amd.modules.entropyCoder import pmfToQuantizedCDF
    row = C.cases()[name]
    got, status = C.quantized_cdf(row)
    assert status == C.OK
    want = np.asarray(pmfToQuantizedCDF(row, 16), dtype=np.uint32)
    assert got.dtype == np.uint32 and got.shape == want.shape
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    assert got[0] == 0 and got[-1] == 65536 and np.all(np.diff(got.astype(np.int64)) >= 1)


@pytest.mark.parametrize("name", sorted(C.bad_cases()))
def test_rows_the_host_function_rejects(name):
    from mcquic_amd.modules.entropyCoder import pmfToQuantizedCDF
    row, status = C.bad_cases()[name]
    assert C.quantized_cdf(row)[1] == status != C.OK
    with pytest.raises(ValueError):
        pmfToQuantizedCDF(row, 16)


def test_the_cases_cover_what_they_claim():
    """The steal loop's paths, read off the numpy rule: both range directions in one row, a tie among donors, a donor used up."""
    cases = C.cases()

    def steals(row):
        p = np.asarray(row, np.float32)
        c = np.floor(p.astype(np.float64) * 65536.0 + 0.5).astype(np.uint64)
        q = (np.uint64(65536) * c) // np.uint64(int(c.sum()))
        cdf = np.concatenate([[0], np.cumsum(q)]).astype(np.int64)
        cdf[-1] = 65536
        out = []
        for i in range(len(p)):
            if cdf[i] == cdf[i + 1]:
                freq = np.diff(cdf)
                spare = np.where(freq > 1, freq, 1 << 40)
                j = int(np.argmin(spare))
                out.append((i, j, int(freq[j]), int((spare == spare[j]).sum())))
                if j < i:
                    cdf[j + 1: i + 1] -= 1
                else:
                    cdf[i + 1: j + 1] += 1
        return out
    both = steals(cases["both_directions"])
    assert any(j < i for i, j, _, _ in both) and any(j > i for i, j, _, _ in both)
    assert any(tied > 1 for _, _, _, tied in steals(cases["donor_ties"]))
    used = steals(cases["donor_used_up"])
    assert used[0][2] == 2 and used[1][1] != used[0][1]                 # the width-2 donor gives once, then the next donor
    big = cases["k8192_more_than_half_zero"]
    assert (big == 0).sum() > 4096
    assert len(steals(cases["all_mass_on_one"])) == 512


def test_normalise_rule_and_bit_sum():
    raw = (np.random.default_rng(0).random((3, 100)) * 5).astype(np.float32)
    p = C.normalise(raw)
    s = np.array([np.float32(sum(float(v) for v in r)) for r in raw], np.float32)       # exact double sum here (100 terms), one rounding
    assert np.array_equal(p, raw / s[:, None])
    table = np.array([[0, 1, 65536], [0, 32768, 65536]], np.uint32)
    codes = [np.array([[[[0, 1]], [[1, 1]]]], np.int64)]                               # n = 1, m = 2, 1 x 2
    assert C.code_bits(codes, [table])[0, 0] == 16.0 + (16.0 - np.log2(65535.0)) + 1.0 + 1.0


def test_closed_form_of_the_steal_loop_equals_the_sequential_loop():
    """What csrc/vq_cdf.hip evaluates in place of the loop (`_cdf_ref.quantized_cdf_closed`, the kernel's steps in numpy) against the
    sequential rule: every shared case, and 1500 seeded rows of 2 to 400 symbols with up to 90 % of them empty, plain and with many
    equal widths (ties among donors)."""
    for name, row in C.cases().items():
        assert np.array_equal(C.quantized_cdf_closed(row), C.quantized_cdf(row)[0]), name
    g = np.random.default_rng(0)
    for t in range(1500):
        k = int(g.integers(2, 400))
        p = g.random(k) ** int(g.integers(1, 14))
        p[g.random(k) < g.random() * 0.9] = 0.0
        if t % 3 == 0:
            p = np.round(p * 8) / 8
        if p.sum() == 0:
            p[-1] = 1.0
        p = (p / p.sum()).astype(np.float32)
        want, status = C.quantized_cdf(p)
        assert status == C.OK
        assert np.array_equal(C.quantized_cdf_closed(p), want), (t, k)
