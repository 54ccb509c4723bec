"""The device coder at module level: `Compressor.compress / decompress(coder="device")`, `EntropyCoder.compressDevice / decompressDevice`,
`DeviceStreams` and `validate(bits="exact")` against the host path of the same model -- bytes, headers, codes and restored images
compared with `==`.  Compressor(8, 2, [16, 8, 4]) with frequency rows far from uniform, at 64x64 and at a size that is no multiple of
128."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [(64, 64), (72, 200)]


@pytest.fixture(scope="module")
def model(dev):
    from mcquic_amd import Compressor
    torch.manual_seed(3407)
    model = Compressor(8, 2, [16, 8, 4]).eval().to(dev)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for f in model._quantizer._entropyCoder._freqEMA:
            r = torch.rand(f.shape, generator=g) ** 6
            r[0, torch.rand(f.shape[1], generator=g) < 0.3] = 0.0
            f.copy_((r + 1e-9).to(dev))
    return model


def _images(dev, hw, n=3):
    return (torch.rand((n, 3) + hw, generator=torch.Generator().manual_seed(hw[0] + hw[1])) * 2 - 1).to(dev)


@pytest.fixture(scope="module")
def host_side(model, dev):
    """size -> (x, codes, binaries, headers, restored) of the host path, computed once."""
    out = {}
    for hw in SIZES:
        x = _images(dev, hw)
        codes, binaries, headers = model.compress(x)
        out[hw] = (x, codes, binaries, headers, model.decompress(binaries, headers))
    return out


@pytest.mark.parametrize("hw", SIZES)
def test_compress_on_the_device_returns_the_host_bytes_and_headers(model, host_side, hw):
    x, codes, binaries, headers, _ = host_side[hw]
    got_codes, got, got_headers = model.compress(x, coder="device")
    assert all(torch.equal(a, b) for a, b in zip(got_codes, codes))
    assert got == binaries
    assert got_headers == headers
    assert sum(len(b) for binary in got for b in binary) > 8 * len(got) * len(got[0])       # (words were emitted, not flushes alone)


@pytest.mark.parametrize("hw", SIZES)
def test_decompress_on_the_device_restores_the_host_image_from_either_sides_bytes(model, host_side, hw):
    x, codes, binaries, headers, restored = host_side[hw]
    coder = model._quantizer._entropyCoder
    assert torch.equal(model.decompress(binaries, headers, coder="device"), restored)
    _, dev_binaries, dev_headers = model.compress(x, coder="device")
    assert torch.equal(model.decompress(dev_binaries, dev_headers, coder="device"), restored)
    assert torch.equal(model.decompress(dev_binaries, dev_headers), restored)
    streams = coder.compressDevice(codes)                                                   # and without the bytes leaving the device
    back = coder.decompressDevice(streams, streams.codeSizes)
    assert all(a.dtype == torch.int64 and torch.equal(a, b) for a, b in zip(back, codes))
    assert not coder.decodeStatus().cpu().numpy().any()
    sizes = streams.sizes()
    assert sizes.dtype == torch.int64 and sizes.is_cuda
    assert sizes.cpu().tolist() == [[len(b) for b in binary] for binary in binaries]
    with pytest.raises(RuntimeError, match="truncated or malformed"):
        coder.decompressDevice([[b[:4] for b in binaries[0]]] + binaries[1:], [h.CodeSize for h in headers])
    with pytest.raises(RuntimeError, match="is not this model's"):                        # `_checkHeaders` runs first, unchanged
        bad = headers[0].CodeSize
        coder.decompressDevice(streams, [type(bad)(bad.m, bad.heights, bad.widths, [16, 8, 5])] * len(headers))


@pytest.mark.parametrize("hw", SIZES)
def test_validate_exact_equals_validate_coded(model, host_side, hw):
    from mcquic_amd.validate import validate
    x = host_side[hw][0]
    coded = validate(model, x, msssim=False, gather=False, bits="coded")
    exact = validate(model, x, msssim=False, gather=False, bits="exact")
    assert exact.dtype == coded.dtype and torch.equal(exact[:, 0], coded[:, 0])
    assert torch.equal(exact[:, 2], coded[:, 2]) and float(exact[:, 2].min()) > 0
    estimated = validate(model, x, msssim=False, gather=False, bits="estimated")
    assert bool((estimated[:, 2] < exact[:, 2]).all())                                      # (the flush words: tests/test_gpu_code_bits_vs_coder.py)


def test_check_raises_the_host_paths_message_for_a_code_out_of_range(model, host_side):
    coder = model._quantizer._entropyCoder
    codes = [c.clone() for c in host_side[SIZES[0]][1]]
    with pytest.raises(RuntimeError) as host:
        bad = [c.clone() for c in codes]
        bad[1][2, 1, 0, 0] = 8
        coder.compress(bad)
    streams = coder.compressDevice(bad)                                                     # does not raise: nothing is read back
    assert streams.status.cpu().tolist() == [0] * 7 + [1] + [0]
    assert streams.sizes().cpu().tolist()[2][1] == 0
    for call in (streams.check, streams.tobytes):
        with pytest.raises(RuntimeError) as device:
            call()
        assert str(device.value) == str(host.value)
    coder.compressDevice(codes).check()


def test_tables_and_streams_capture_into_one_graph(model, host_side, dev):
    """deviceCDFs(normalize=True) + compressDevice captured on ONE stream (no forks): replayed with new codes and a changed `_freqEMA`
    in between, the bytes are those of the host coder under the same normalize=True tables."""
    from mcquic_amd.modules import entropyCoder as E
    coder = E.EntropyCoder(2, [16, 8, 4]).to(dev)
    shapes = [tuple(c.shape) for c in host_side[SIZES[1]][1]]
    static = [torch.zeros(s, dtype=torch.int64, device=dev) for s in shapes]

    def refill(seed):
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for f in coder._freqEMA:
                f.copy_((torch.rand(f.shape, generator=g) ** 4 * 3.0 + 1e-6).to(dev))
        for s, k in zip(static, (16, 8, 4)):
            s.copy_(torch.randint(0, k, s.shape, generator=g).to(dev))

    def run():
        tables = coder.deviceCDFs(normalize=True)
        return tables, coder.compressDevice(static, cdfs=tables)
    refill(100)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                                                               # the kernels' first launch, outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tables, streams = run()
    seen = []
    for seed in (101, 102):
        refill(seed)
        graph.replay()
        torch.cuda.synchronize()
        got = streams.tobytes()
        for lv, (table, code) in enumerate(zip(tables, static)):
            n, m, h, w = code.shape
            host_table = E._Tables(table.cpu().numpy().astype(np.int64).tolist(), table.shape[1] - 1)
            want = E.ransEncodeBatchWithIndexes(code.cpu().numpy().reshape(n, -1), np.repeat(np.arange(m, dtype=np.int32), h * w), host_table)
            assert [got[i][lv] for i in range(n)] == want, (seed, lv)
        seen.append(got)
    assert seen[0] != seen[1]
    graph.reset()
