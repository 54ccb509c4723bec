"""mcq_code_bits (csrc/vq_cdf.hip): per image and level the sum over groups and positions of 16 - log2(cdf[c + 1] - cdf[c]), against the
float64 numpy sum of tests/_cdf_ref.py.

Tolerance, derived: a term lies in [0, 16]; one ulp of a double at 16 is 2^-48.  The device's double `log2` is the ROCm device library's,
documented at 1 ulp; the subtraction from 16 rounds once more (half an ulp), so a term is within 1.5 * 2^-48 of its value, and numpy's
within an ulp.  The partial sums stay below 16 N (N = m h w symbols per image and level) and the kernel adds along a fixed tree of depth
ceil(N / 1024) + 6 + 4 (a lane's own terms, the wave, the sixteen waves), each addition within half an ulp of its sum: depth * 16 N *
2^-53.  For the largest N here (3072) that is 13 * 2^-49 N; with the terms' 2.5 * 2^-48 N and numpy's pairwise sum (depth ~12) the two
sides differ by less than N * 2^-44, which is the bound asserted."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _cdf_ref as C

pytestmark = pytest.mark.gpu

KS = (512, 64, 7)
M = 2


def _tables(dev, seed=0):
    from mcquic_amd import ops
    g = np.random.default_rng(seed)
    rows = []
    for k in KS:
        f = g.random((M, k)) ** 6 + 1e-9
        f[0, g.random(k) < 0.3] = 0.0                       # (bins of width 1 among wide ones)
        rows.append((f / f.sum(-1, keepdims=True)).astype(np.float32))
    tables, status = ops.pmf_to_quantized_cdf_dev([torch.from_numpy(r).to(dev) for r in rows])
    assert not status.cpu().numpy().any()
    return tables


def _codes(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, k, (n, M, max(1, h >> lv), max(1, w >> lv)), generator=g) for lv, k in enumerate(KS)]


@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (17, 9), (48, 32)])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_bits_against_the_float64_sum(dev, n, hw):
    from mcquic_amd import ops
    tables = _tables(dev)
    codes = _codes(n, hw[0], hw[1], seed=10 * n + hw[0])
    bits, err = ops.code_bits([c.to(dev) for c in codes], tables)
    assert bits.dtype == torch.float64 and tuple(bits.shape) == (n, len(KS)) and err.dtype == torch.int32
    want = C.code_bits([c.numpy() for c in codes], [t.cpu().numpy() for t in tables])
    got = bits.cpu().numpy()
    for lv, c in enumerate(codes):
        symbols = c[0].numel()
        diff = np.abs(got[:, lv] - want[:, lv]).max()
        print(f"n={n} map={hw} level={lv}: N={symbols} max |device - float64| = {diff:.3e} bits (allowed {symbols * 2.0 ** -44:.3e})")
        assert diff <= symbols * 2.0 ** -44
    assert not err.cpu().numpy().any()
    again, _ = ops.code_bits([c.to(dev) for c in codes], tables)
    assert torch.equal(bits, again)                                                     # the same bits on every run


def test_a_code_out_of_range_sets_the_error_word_and_adds_nothing(dev):
    from mcquic_amd import ops
    tables = _tables(dev)
    codes = _codes(3, 17, 9, seed=1)
    codes[0][1, 1, 16, 8] = KS[0]                                                       # one past the last symbol
    codes[2][2, 0, 0, 0] = -1
    out = torch.full((3, 3), -5.0, dtype=torch.float64, device=dev)
    error = torch.full((3, 3), 9, dtype=torch.int32, device=dev)
    bits, err = ops.code_bits([c.to(dev) for c in codes], tables, out=out, error=error)
    assert bits is out and err is error
    want_err = np.zeros((3, 3), np.int32)
    want_err[1, 0] = want_err[2, 2] = 1
    assert np.array_equal(err.cpu().numpy(), want_err)
    inside = [c.clone() for c in codes]
    inside[0][1, 1, 16, 8] = 0
    inside[2][2, 0, 0, 0] = 0
    host_tables = [t.cpu().numpy() for t in tables]
    want = C.code_bits([c.numpy() for c in inside], host_tables)
    want[1, 0] -= 16.0 - np.log2(float(int(host_tables[0][1, 1]) - int(host_tables[0][1, 0])))
    want[2, 2] -= 16.0 - np.log2(float(int(host_tables[2][0, 1]) - int(host_tables[2][0, 0])))
    got = bits.cpu().numpy()
    for lv, c in enumerate(codes):
        assert np.abs(got[:, lv] - want[:, lv]).max() <= c[0].numel() * 2.0 ** -44          # each level's own symbol count


def test_shape_errors_are_those_of_compress(dev):
    from mcquic_amd.modules import entropyCoder as E
    coder = E.EntropyCoder(M, list(KS)).to(dev)
    good = [c.to(dev) for c in _codes(2, 4, 4, seed=2)]
    assert tuple(coder.codeBits(good).shape) == (2, 3) and not coder.codeBitsError().cpu().numpy().any()
    with pytest.raises(RuntimeError, match="Length of codes is 0"):
        coder.codeBits([])
    with pytest.raises(RuntimeError, match="`n` is inconsisitent"):
        coder.codeBits([good[0], good[1][:1], good[2]])
    with pytest.raises(RuntimeError, match="`m` is inconsisitent"):
        coder.codeBits([good[0], good[1][:, :1], good[2]])
    with pytest.raises(RuntimeError, match="expected 3 code levels"):
        coder.codeBits(good[:2])


def test_tables_then_bits_capture_and_replay(dev):
    """deviceCDFs(normalize=True) followed by codeBits inside torch.cuda.graph: two replays, `_freqEMA` and the codes changed in
    between, equal the eager results of the same inputs."""
    from mcquic_amd.modules import entropyCoder as E
    coder = E.EntropyCoder(M, list(KS)).to(dev)
    g = torch.Generator().manual_seed(7)
    static = [c.to(dev) for c in _codes(2, 17, 9, seed=3)]

    def refill(seed):
        gg = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for f in coder._freqEMA:
                f.copy_((torch.rand(f.shape, generator=gg) ** 4 * 3.0 + 1e-6).to(dev))
        for s, c in zip(static, _codes(2, 17, 9, seed=seed)):
            s.copy_(c.to(dev))

    def run():
        tables = coder.deviceCDFs(normalize=True)
        return tables, coder.codeBits(static, cdfs=tables)
    refill(100)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                                           # warm-up on a side stream: the buffers exist
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tables, bits = run()
    for seed in (101, 102):
        refill(seed)
        graph.replay()
        torch.cuda.synchronize()
        got_tables, got_bits = [t.clone() for t in tables], bits.clone()
        coder.resetFreqAndCDF()
        want_tables, want_bits = run()
        torch.cuda.synchronize()
        assert all(np.array_equal(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(got_tables, want_tables))
        assert torch.equal(got_bits, want_bits) and float(got_bits.min()) > 0
        raw = [f.detach().cpu().numpy() for f in coder._freqEMA]
        for r, t in zip(raw, got_tables):
            assert np.array_equal(t.cpu().numpy()[0], C.quantized_cdf(C.normalise(r)[0])[0])
    graph.reset()


def test_the_capture_holds_two_library_kernels_and_nothing_else(dev, tmp_path):
    """A kernel trace of one replay of that capture, taken in a fresh process (tests/_cdf_names_worker.py under rocprofv3, as the other
    names workers are): from the process's last hipGraphLaunch on, exactly one vq_cdf_kernel and one vq_code_bits_kernel -- no memset
    node's fill, no ATen launch, no copy."""
    import csv
    import glob
    import shutil
    here = os.path.dirname(os.path.abspath(__file__))
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    run = subprocess.run([prof, "--kernel-trace", "--hip-runtime-trace", "-f", "csv", "-d", str(tmp_path), "-o", "cdf", "--",
                          sys.executable, os.path.join(here, "_cdf_names_worker.py")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-2000:]

    def rows(kind):
        files = glob.glob(os.path.join(str(tmp_path), "**", f"*{kind}.csv"), recursive=True)
        assert len(files) == 1, (kind, files)
        with open(files[0]) as f:
            return list(csv.DictReader(f))
    launches = [int(r["Start_Timestamp"]) for r in rows("hip_api_trace") if "GraphLaunch" in r["Function"]]
    assert launches, "no hipGraphLaunch in the trace"
    names = [r["Kernel_Name"] for r in rows("kernel_trace") if int(r["Start_Timestamp"]) >= max(launches)]
    print(names)
    foreign = [n for n in names if "at::native" in n or "emset" in n or "fillBuffer" in n or "elementwise_kernel" in n or "copyBuffer" in n]
    assert not foreign, foreign
    assert sorted("cdf" if "vq_cdf_kernel" in n else "bits" if "vq_code_bits_kernel" in n else n for n in names) == ["bits", "cdf"]
