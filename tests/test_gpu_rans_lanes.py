"""The lanes coder on the device (csrc/rans_lanes.hip; ops.rans_encode_dev(lanes=...) / rans_decode_dev(lanes=True)) against the host
lanes coder (csrc/rans.cpp), which tests/test_rans_lanes_host.py holds byte for byte to a plain-Python restatement of the layout:
everything is integer, everything is compared with `==`.  Lengths around a round (64), a gathered chunk (ops.RANS_DEV_CHUNK) and a
stream whose words outgrow one LDS chunk; tables that make no lane emit for many rounds, every lane emit in every round, and anything
between; more levels than one launch takes; mixed widths in one call; every malformed input; the module's `lanes=` argument under both
coders; one captured graph from tables to decoded codes; and the length interval against `codeBits`."""
import math

import numpy as np
import pytest
import torch

import _rans_lanes_ref as R

pytestmark = pytest.mark.gpu

TABLES = (("uniform", 2), ("uniform", 512), ("uniform", 8192), ("peaked", 512), ("ones", 512), ("halfdead", 512))
LENGTHS = (1, 63, 64, 65, 1025)
CROSSING = 3000             # symbols per group under the uniform k = 8192 table: 13 bits each, 1218 words per group > one LDS chunk of 1024


def _draw(kind, table, n, hw, g):
    """int64 [n, m, 1, hw] codes under uint32 `table` [m, k + 1] (R.draw's kinds, vectorised)."""
    widths = np.diff(table.astype(np.int64), axis=1)
    out = np.empty((n, table.shape[0], 1, hw), dtype=np.int64)
    for j, w in enumerate(widths):
        if kind == "peaked":
            out[:, j, 0] = int(w.argmax())
        elif kind == "ones":
            out[:, j, 0] = g.choice(np.flatnonzero(w == 1), size=(n, hw))
        else:
            out[:, j, 0] = g.choice(len(w), size=(n, hw), p=w / 65536.0)
    return out


def _levels(n, m, seed):
    """[(kind, k, table uint32 [m, k + 1], codes int64 [n, m, 1, hw])]: 40 levels."""
    g = np.random.default_rng(seed)
    out = []
    for kind, k in TABLES:
        table = np.asarray(R.tables(kind, m, k), dtype=np.uint32)
        for hw in LENGTHS + ((CROSSING,) if (kind, k) == ("uniform", 8192) else ()):
            out.append((kind, k, table, _draw(kind, table, n, hw, g)))
    table = np.asarray(R.tables("halfdead", m, 512), dtype=np.uint32)
    for hw in range(2, 11):
        out.append(("halfdead", 512, table, _draw("halfdead", table, n, hw, g)))
    return out


def _host_streams(levels, n, widths):
    """bytes per stream, image-major, from the host lanes coder."""
    from mcquic_amd.modules.entropyCoder import ransLanesEncodeBatch
    per_level = [ransLanesEncodeBatch(c.reshape(n, -1), c.shape[1], c.shape[3], t, "auto" if w == 0 else w)
                 for (_, _, t, c), w in zip(levels, widths)]
    return [per_level[lv][i] for i in range(n) for lv in range(len(levels))]


def _upload(streams, dev):
    offs = np.zeros(len(streams) + 1, dtype=np.int64)
    np.cumsum([len(b) for b in streams], out=offs[1:])
    data = np.frombuffer(b"".join(streams), dtype=np.uint8).copy()          # exactly the streams: nothing readable behind the last one
    return torch.from_numpy(data).to(dev), torch.from_numpy(offs).to(dev)


def _device_streams(enc):
    blob, offsets, status = (t.cpu().numpy() for t in enc)
    return [blob[offsets[s]:offsets[s + 1]].tobytes() for s in range(len(status))], offsets, status


def _dev_table(table, dev):
    return torch.from_numpy(table.view(np.int32)).view(torch.uint32).to(dev)


@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 5])
def test_bytes_offsets_sizes_and_codes_equal_the_host_coder(dev, n, m):
    from mcquic_amd import _lib, ops
    levels = _levels(n, m, 100 * n + m)
    assert len(levels) == 40 > _lib.MCQ_VQ_MAX_LEVELS      # the binding chunks at 32
    codes = [torch.from_numpy(c).to(dev) for _, _, _, c in levels]
    tables = [_dev_table(t, dev) for _, _, t, _ in levels]
    shapes = [tuple(c.shape) for c in codes]
    mixed = [(1, 2, 4, 8, 16, 32, 64, "auto")[i % 8] for i in range(len(levels))]
    enc = None
    for lanes in R.WIDTHS + ("auto", mixed):
        widths = ops.rans_lanes_widths(lanes, len(levels))
        want = _host_streams(levels, n, widths)
        enc = ops.rans_encode_dev(codes, tables, out=enc, lanes=lanes)      # (the buffers of the first call, written in place)
        got, offsets, status = _device_streams(enc)
        assert not status.any(), lanes
        for s, (a, b) in enumerate(zip(got, want)):
            kind, k, _, c = levels[s % len(levels)]
            assert a == b, (lanes, s // len(levels), kind, k, c.shape[3], len(a), len(b))
            W = a[3]
            assert W == (widths[s % len(levels)] or R.auto_width(m * c.shape[3])) and len(a) <= 4 * (1 + 2 * W + m * c.shape[3])
            if kind == "peaked" and m * -(-c.shape[3] // W) * math.log2(65536 / (65536 - 511)) < 31:
                assert len(a) == 4 * (1 + 2 * W), "no lane emits: the stream is its prefix and states"
        assert np.array_equal(offsets, np.concatenate([[0], np.cumsum([len(b) for b in want])]))
        assert np.array_equal(enc.sizes.cpu().numpy(), [len(b) for b in want])
        if lanes in (1, 64, "auto") or lanes is mixed:
            for source, (b, o) in (("host bytes", _upload(want, dev)), ("device blob", (enc.blob, enc.offsets))):
                back, st = ops.rans_decode_dev(b, o, tables, shapes, lanes=True)
                assert not st.cpu().numpy().any(), (lanes, source)
                for lv, (a, c) in enumerate(zip(back, codes)):
                    assert a.dtype == torch.int64 and torch.equal(a, c), (lanes, source, levels[lv][:2], shapes[lv])
    assert enc.blob.numel() == n * sum(4 * m * s[3] + 8 + 4 * (1 + 2 * 64) for s in shapes)
    with pytest.raises(ValueError, match="earlier call"):
        ops.rans_encode_dev(codes, tables, out=enc)                         # a plain call does not take a lanes call's buffers


def test_every_width_decodes_on_the_device(dev):
    from mcquic_amd import ops
    levels = [lv for lv in _levels(2, 2, 7) if lv[3].shape[3] in (65, 1025, CROSSING)]
    codes = [torch.from_numpy(c).to(dev) for _, _, _, c in levels]
    tables = [_dev_table(t, dev) for _, _, t, _ in levels]
    shapes = [tuple(c.shape) for c in codes]
    for W in R.WIDTHS:
        blob, offs = _upload(_host_streams(levels, 2, [W] * len(levels)), dev)
        back, st = ops.rans_decode_dev(blob, offs, tables, shapes, lanes=True)
        assert not st.cpu().numpy().any() and all(torch.equal(a, c) for a, c in zip(back, codes)), W


def _five(dev, m=2, hw=700):
    """Five images, two levels (half dead, uniform at k = 512): streams long enough to hold words."""
    g = np.random.default_rng(5)
    levels = []
    for kind in ("halfdead", "uniform"):
        table = np.asarray(R.tables(kind, m, 512), dtype=np.uint32)
        levels.append((kind, 512, table, _draw(kind, table, 5, hw, g)))
    return levels, [_dev_table(t, dev) for _, _, t, _ in levels]


@pytest.mark.parametrize("bad", ["k", "minus one", "both"])
def test_a_code_out_of_range_sets_that_streams_status_and_no_other(dev, bad):
    from mcquic_amd import ops
    levels, tables = _five(dev)
    want = _host_streams(levels, 5, [64, 64])
    codes = [torch.from_numpy(c.copy()).to(dev) for _, _, _, c in levels]
    if bad in ("k", "both"):
        codes[0][2, 1, 0, 699] = 512
    if bad in ("minus one", "both"):
        codes[0][2, 0, 0, 3] = -1
    got, offsets, status = _device_streams(ops.rans_encode_dev(codes, tables, lanes=64))
    want_status = np.zeros(10, np.int32)
    want_status[2 * 2 + 0] = ops.RANS_BAD_SYMBOL
    assert np.array_equal(status, want_status)
    for s in range(10):
        assert got[s] == (b"" if s == 4 else want[s]), s
    assert offsets[5] == offsets[4]


@pytest.mark.parametrize("W", [4, 64])
@pytest.mark.parametrize("how", list(R.MALFORMED))
def test_a_malformed_stream_is_refused_and_zeroed_and_the_others_decode(dev, how, W):
    from mcquic_amd import ops
    levels, tables = _five(dev)
    streams = _host_streams(levels, 5, [W, W])
    victim = 2 * 2 + 1                                      # image 2, level 1
    assert len(streams[victim]) > 4 * (1 + 2 * W) + 64
    streams[victim] = R.MALFORMED[how](streams[victim])     # (a length that is not a multiple of 4 also starts the NEXT stream off a word boundary)
    blob, offs = _upload(streams, dev)
    shapes = [tuple(c.shape) for _, _, _, c in levels]
    poison = ([torch.full(s, 77, dtype=torch.int64, device=dev) for s in shapes], torch.full((10,), 9, dtype=torch.int32, device=dev))
    back, status = ops.rans_decode_dev(blob, offs, tables, shapes, out=poison, lanes=True)
    want_status = np.zeros(10, np.int32)
    want_status[victim] = ops.RANS_BAD_STREAM
    assert np.array_equal(status.cpu().numpy(), want_status)
    for lv, (_, _, _, c) in enumerate(levels):
        want = c.copy()
        if lv == 1:
            want[2] = 0
        assert np.array_equal(back[lv].cpu().numpy(), want), lv


@pytest.mark.parametrize("how", ["past the blob", "decreasing", "negative", "broken table"])
def test_offsets_outside_the_blob_and_a_bin_without_cum_are_refused(dev, how):
    from mcquic_amd import ops
    levels, tables = _five(dev)
    streams = _host_streams(levels, 5, [64, 64])
    blob, offs = _upload(streams, dev)
    offs = offs.cpu().numpy().copy()
    refused = {"past the blob": [9], "decreasing": [4, 5], "negative": [0], "broken table": [0, 2, 4, 6, 8]}[how]
    if how == "past the blob":
        offs[10] += 4096
    elif how == "decreasing":
        offs[5] = offs[4] - 8                               # stream 4 ends before it starts; stream 5 then starts inside stream 3
    elif how == "negative":
        offs[0] = -64
    else:
        broken = levels[0][2].copy()
        broken[:, 0] = 65535                                # entry 0 above every cum: the bin the bisection ends in does not contain it
        tables = [_dev_table(broken, dev), tables[1]]
    shapes = [tuple(c.shape) for _, _, _, c in levels]
    back, status = ops.rans_decode_dev(blob, torch.from_numpy(offs).to(dev), tables, shapes, lanes=True)
    status = status.cpu().numpy()
    assert all(status[s] == ops.RANS_BAD_STREAM for s in refused) and not status[[s for s in range(10) if s not in refused]].any()
    for s in range(10):
        i, lv = divmod(s, 2)
        got = back[lv][i].cpu().numpy()
        assert not got.any() if s in refused else np.array_equal(got, levels[lv][3][i]), s


def _model(dev, seed=3407):
    """Compressor(32, 2, [64, 32, 16]) with random weights and frequency rows far from uniform."""
    from mcquic_amd import Compressor
    torch.manual_seed(seed)
    model = Compressor(32, 2, [64, 32, 16]).eval().to(dev)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for f in model._quantizer._entropyCoder._freqEMA:
            f.copy_((torch.rand(f.shape, generator=g) ** 6 + 1e-9).to(dev))
    return model


@pytest.mark.parametrize("size", [(64, 64), (72, 200)])
def test_the_module_gives_one_stream_and_one_image_under_both_coders(dev, size):
    model = _model(dev)
    x = (torch.rand((3, 3) + size, generator=torch.Generator().manual_seed(1)) * 2 - 1).to(dev)
    codes, plain, headers = model.compress(x)
    image = model.decompress(plain, headers)
    on_host = model.compress(x, coder="host", lanes="auto")
    on_device = model.compress(x, coder="device", lanes="auto")
    assert on_host[1] == on_device[1] and on_host[1] != plain
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(codes, on_host[0], on_device[0]))
    assert [h.CodeSize for h in on_host[2]] == [h.CodeSize for h in headers]
    for binaries in (on_host[1], on_device[1]):
        for coder in ("host", "device"):
            assert torch.equal(model.decompress(binaries, headers, coder=coder, lanes=True), image), coder
            with pytest.raises(RuntimeError, match="lanes=True"):
                model.decompress(binaries, headers, coder=coder, lanes=False)
    for coder in ("host", "device"):
        with pytest.raises(RuntimeError, match="truncated or malformed"):
            model.decompress(plain, headers, coder=coder, lanes=True)
    forced = model.compress(x, coder="device", lanes=64)[1]
    assert forced == model.compress(x, coder="host", lanes=64)[1] and all(b[3] == 64 for binary in forced for b in binary)
    assert torch.equal(model.decompress(forced, headers, coder="device", lanes=True), image)


def test_tables_streams_and_decoded_codes_replay_from_one_graph(dev):
    """deviceCDFs(normalize=True) + compressDevice(lanes=64) + decompressDevice(lanes=True) captured on one stream: replayed with new
    codes, the decoded codes are the new codes and the bytes the host lanes coder's.  The frequency rows are small integers, so the row
    sums are exact and the normalize=True tables the encoder uses equal the normalize=False tables the decoder builds."""
    from mcquic_amd.modules import entropyCoder as E
    coder = E.EntropyCoder(2, [16, 8, 4]).to(dev)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for f in coder._freqEMA:
            f.copy_(torch.randint(1, 64, f.shape, generator=g).float().to(dev))
    shapes = [(3, 2, 40 >> lv, 56 >> lv) for lv in range(3)]
    static = [torch.zeros(s, dtype=torch.int64, device=dev) for s in shapes]

    def refill(seed):
        g = torch.Generator().manual_seed(seed)
        for s, k in zip(static, (16, 8, 4)):
            s.copy_(torch.randint(0, k, s.shape, generator=g).to(dev))

    def run():
        tables = coder.deviceCDFs(normalize=True)
        streams = coder.compressDevice(static, cdfs=tables, lanes=64)
        return tables, streams, coder.decompressDevice(streams, streams.codeSizes, check=False, lanes=True)
    refill(100)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run()                                               # the kernels' first launch, outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tables, streams, decoded = run()
    seen = []
    for seed in (101, 102):
        refill(seed)
        graph.replay()
        torch.cuda.synchronize()
        assert not coder.decodeStatus().cpu().numpy().any() and not streams.status.cpu().numpy().any()
        assert all(torch.equal(a, b) for a, b in zip(decoded, static)), seed
        got = streams.tobytes()
        for lv, (table, code) in enumerate(zip(tables, static)):
            n, m, h, w = code.shape
            want = E.ransLanesEncodeBatch(code.cpu().numpy().reshape(n, -1), m, h * w, table.cpu().numpy().astype(np.int64), 64)
            assert [got[i][lv] for i in range(n)] == want, (seed, lv)
        seen.append(got)
    assert seen[0] != seen[1]
    graph.reset()


def test_device_stream_lengths_lie_in_the_derived_interval(dev):
    """B = 8 len(stream) against S = codeBits: 32 + 32 W - slack < B - S <= 32 + 64 W + slack (R.length_interval)."""
    model = _model(dev)
    coder = model._quantizer._entropyCoder
    g = torch.Generator().manual_seed(2)
    codes = [torch.randint(0, k, (2, 2, 48 >> lv, 32 >> lv), generator=g).to(dev) for lv, k in enumerate((64, 32, 16))]
    bits = coder.codeBits(codes).cpu().numpy()
    assert not coder.codeBitsError().cpu().numpy().any()
    for lanes in (1, 8, 64, "auto"):
        streams = coder.compressDevice(codes, lanes=lanes)
        sizes = streams.sizes().cpu().numpy()
        binaries = streams.tobytes()
        for lv, code in enumerate(codes):
            symbols = code[0].numel()
            W = R.auto_width(symbols) if lanes == "auto" else lanes
            low, high = R.length_interval(symbols, W)
            for i in range(2):
                assert len(binaries[i][lv]) == sizes[i, lv] and binaries[i][lv][3] == W
                d = 8 * len(binaries[i][lv]) - bits[i, lv]
                print(f"lanes {lanes} level {lv} image {i}: W {W}, B - S = {d:.3f} in ({low:.3f}, {high:.3f}]")
                assert low < d <= high, (lanes, lv, i, d, low, high)
