"""The device rANS coder (csrc/rans_dev.hip; ops.rans_encode_dev / rans_decode_dev) against the library's own host coder (csrc/rans.cpp,
itself pinned to the reference's compiled extension in tests/test_entropy_coder.py): everything is integer, everything is compared with
`==`.  Hand-made tables and draws so that every branch is reached: the most and the fewest renormalisations, empty bins filled by the
table's steal path, the table switching inside a stream, streams around the lane count (64) and around the kernels' LDS chunk
(ops.RANS_DEV_CHUNK), levels of different k and length in one launch -- and more levels than one launch takes, so the binding's chunking
runs too."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _pmfs():
    """name -> pmf row [k] (float64, normalised below)."""
    from mcquic_amd import ops
    g = np.random.default_rng(7)
    out = {f"uniform{k}": np.ones(k) for k in (2, 512, ops.cdf_max_k())}
    peaked = np.full(ops.cdf_max_k(), 1e-9)                 # every other bin quantises to 0 and steals one count: freq == 1
    peaked[0] = 1.0
    out["peaked"] = peaked
    dead = g.random(512) ** 4 + 1e-3
    dead[g.permutation(512)[:256]] = 0.0                    # half the symbols dead before quantisation
    out["halfdead"] = dead
    return out


def _tables(m):
    """name -> the host coder's tables of m groups (each group the row rolled by 3 g, so the groups differ): (_Tables, uint32 [m, k + 1])."""
    from mcquic_amd.modules.entropyCoder import _Tables, pmfToQuantizedCDF
    out = {}
    for name, p in _pmfs().items():
        rows = [pmfToQuantizedCDF((np.roll(p, 3 * g) / p.sum()).astype(np.float32).tolist(), 16) for g in range(m)]
        out[name] = (_Tables(rows, len(p)), np.asarray(rows, dtype=np.uint32))
    return out


def _lengths(m):
    """h w per level such that m h w lands on (m = 1) or just above the seams: 1, the lane count, the LDS chunk, several chunks."""
    from mcquic_amd import ops
    ch = ops.RANS_DEV_CHUNK
    return [-(-t // m) for t in (1, 63, 64, 65, ch - 1, ch, ch + 1, 3 * ch + 5)]


def _draw(kind, table, n, m, hw, g):
    """int64 [n, m, 1, hw] codes under uint32 `table` [m, k + 1]."""
    freq = np.diff(table.astype(np.int64), axis=1)
    out = np.empty((n, m, 1, hw), dtype=np.int64)
    for j in range(m):
        if kind == "dist":
            out[:, j, 0] = g.choice(freq.shape[1], size=(n, hw), p=freq[j] / 65536.0)
        elif kind == "top":
            out[:, j, 0] = int(freq[j].argmax())
        else:                                               # "rare": a symbol of the least width (1 wherever the table has one)
            out[:, j, 0] = int(freq[j].argmin())
    return out


def _host_streams(levels, n):
    """levels: list of (host tables, codes int64 [n, m, 1, hw]) -> bytes per stream, image-major."""
    from mcquic_amd.modules.entropyCoder import ransEncodeBatchWithIndexes
    per_level = []
    for t, c in levels:
        m, hw = c.shape[1], c.shape[3]
        per_level.append(ransEncodeBatchWithIndexes(c.reshape(n, -1), np.repeat(np.arange(m, dtype=np.int32), hw), t))
    return [per_level[lv][i] for i in range(n) for lv in range(len(levels))]


def _upload(streams, dev, blob_tail=0):
    offs = np.zeros(len(streams) + 1, dtype=np.int64)
    np.cumsum([len(b) for b in streams], out=offs[1:])
    data = np.frombuffer(b"".join(streams) + b"\xee" * blob_tail, dtype=np.uint8).copy()
    return torch.from_numpy(data).to(dev), torch.from_numpy(offs).to(dev)


def _device_streams(enc):
    blob, offsets, status = (t.cpu().numpy() for t in enc)
    return [blob[offsets[s]:offsets[s + 1]].tobytes() for s in range(len(status))], offsets, status


@pytest.mark.parametrize("draw", ["dist", "top", "rare"])
@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 5])
def test_bytes_and_codes_equal_the_host_coder(dev, n, m, draw):
    from mcquic_amd import _lib, ops
    g = np.random.default_rng(100 * n + 10 * m + len(draw))
    tables = _tables(m)
    levels, dev_tables, names = [], [], []
    for name, (host, table) in tables.items():
        for hw in _lengths(m):
            levels.append((host, _draw(draw, table, n, m, hw, g)))
            dev_tables.append(torch.from_numpy(table.view(np.int32)).view(torch.uint32).to(dev))
            names.append((name, m * hw))
    assert len(levels) > _lib.MCQ_VQ_MAX_LEVELS              # more levels than one launch's tables hold
    want = _host_streams(levels, n)
    codes = [torch.from_numpy(c).to(dev) for _, c in levels]
    enc = ops.rans_encode_dev(codes, dev_tables)
    got, offsets, status = _device_streams(enc)
    assert not status.any()
    for s, (a, b) in enumerate(zip(got, want)):
        assert a == b, (s // len(levels), names[s % len(levels)], len(a), len(b))
    assert np.array_equal(offsets, np.concatenate([[0], np.cumsum([len(b) for b in want])]))
    assert np.array_equal(enc.sizes.cpu().numpy(), [len(b) for b in want])
    if draw == "top":
        # A symbol of width f adds log2(65536 / f) bits to the state, which starts at 2^31 and emits its first word only at 2^47 f >
        # 2^62: while symbols * log2(65536 / f) < 31 nothing is emitted and the stream is the 8 flush bytes.  The peaked table's top
        # symbol keeps 65536 - 8191 counts (every other bin stole one).
        f = 65536 - (ops.cdf_max_k() - 1)
        checked = 0
        for s, b in enumerate(got):
            name, symbols = names[s % len(levels)]
            if name == "peaked" and symbols * math.log2(65536 / f) < 31:
                assert len(b) == 8, (name, symbols, len(b))
                checked += 1
        assert checked >= 4 * n
    shapes = [tuple(c.shape) for c in codes]
    blob, offs = _upload(want, dev)
    for source, (b, o) in (("host bytes", (blob, offs)), ("device blob", (enc.blob, enc.offsets))):
        back, st = ops.rans_decode_dev(b, o, dev_tables, shapes)
        assert not st.cpu().numpy().any(), source
        for lv, (a, c) in enumerate(zip(back, codes)):
            assert a.dtype == torch.int64 and torch.equal(a, c), (source, names[lv])
    again = ops.rans_encode_dev(codes, dev_tables, out=enc)                 # the buffers of the first call, written in place
    assert again is enc and _device_streams(again)[0] == want


def _five(dev, seed=5, m=2, hw=700):
    """Five images, two levels (k = 512 half dead, k = 8192 peaked), draws from the tables: streams long enough to hold words."""
    g = np.random.default_rng(seed)
    tables = _tables(m)
    levels = [(tables[name][0], _draw("dist", tables[name][1], 5, m, hw, g)) for name in ("halfdead", "uniform512")]
    dev_tables = [torch.from_numpy(tables[name][1].view(np.int32)).view(torch.uint32).to(dev) for name in ("halfdead", "uniform512")]
    return levels, dev_tables


@pytest.mark.parametrize("bad", ["k", "minus one", "both"])
def test_a_code_out_of_range_sets_that_streams_status_and_no_other(dev, bad):
    from mcquic_amd import ops
    levels, dev_tables = _five(dev)
    want = _host_streams(levels, 5)
    codes = [torch.from_numpy(c.copy()).to(dev) for _, c in levels]
    if bad in ("k", "both"):
        codes[0][2, 1, 0, 699] = 512                        # one past the last symbol, in the stream's first chunk to be coded
    if bad in ("minus one", "both"):
        codes[0][2, 0, 0, 3] = -1
    got, offsets, status = _device_streams(ops.rans_encode_dev(codes, dev_tables))
    want_status = np.zeros(10, np.int32)
    want_status[2 * 2 + 0] = ops.RANS_BAD_SYMBOL
    assert np.array_equal(status, want_status)
    for s in range(10):
        assert got[s] == (b"" if s == 4 else want[s]), s
    assert offsets[5] == offsets[4]


@pytest.mark.parametrize("cut", ["by 4 bytes", "to 4 bytes", "to 0 bytes", "by 1 byte"])
def test_a_cut_stream_is_refused_and_zeroed_and_the_others_decode(dev, cut):
    from mcquic_amd import ops
    from mcquic_amd.modules.entropyCoder import ransDecodeWithIndexes
    levels, dev_tables = _five(dev)
    streams = _host_streams(levels, 5)
    victim = 2 * 2 + 1                                      # image 2, level 1
    assert len(streams[victim]) > 16
    whole = streams[victim]
    streams[victim] = {"by 4 bytes": whole[:-4], "to 4 bytes": whole[:4], "to 0 bytes": b"", "by 1 byte": whole[:-1]}[cut]
    with pytest.raises(RuntimeError):                       # the host coder refuses it too
        ransDecodeWithIndexes(streams[victim], np.repeat(np.arange(2, dtype=np.int32), 700), levels[1][0])
    blob, offs = _upload(streams, dev)
    shapes = [tuple(c.shape) for _, c in levels]
    poison = ([torch.full(s, 77, dtype=torch.int64, device=dev) for s in shapes], torch.full((10,), 9, dtype=torch.int32, device=dev))
    back, status = ops.rans_decode_dev(blob, offs, dev_tables, shapes, out=poison)
    assert back[0] is poison[0][0] and status is poison[1]
    want_status = np.zeros(10, np.int32)
    want_status[victim] = ops.RANS_BAD_STREAM
    assert np.array_equal(status.cpu().numpy(), want_status)
    for lv, (_, c) in enumerate(levels):
        want = c.copy()
        if lv == 1:
            want[2] = 0
        assert np.array_equal(back[lv].cpu().numpy(), want), lv


@pytest.mark.parametrize("how", ["past the blob", "decreasing", "negative"])
def test_offsets_outside_the_blob_are_refused(dev, how):
    from mcquic_amd import ops
    levels, dev_tables = _five(dev)
    streams = _host_streams(levels, 5)
    blob, offs = _upload(streams, dev)
    offs = offs.cpu().numpy().copy()
    refused = {"past the blob": [9], "decreasing": [4, 5], "negative": [0]}[how]
    if how == "past the blob":
        offs[10] += 4096                                    # the last stream claims bytes the blob does not have
    elif how == "decreasing":
        offs[5] = offs[4] - 8                               # stream 4 ends before it starts; stream 5 then holds both and runs on
    else:
        offs[0] = -64
    shapes = [tuple(c.shape) for _, c in levels]
    back, status = ops.rans_decode_dev(blob, torch.from_numpy(offs).to(dev), dev_tables, shapes)
    status = status.cpu().numpy()
    assert all(status[s] == ops.RANS_BAD_STREAM for s in refused if s != 5) and not status[[s for s in range(10) if s not in refused]].any()
    for s in range(10):
        i, lv = divmod(s, 2)
        got = back[lv][i].cpu().numpy()
        if s in refused and status[s]:
            assert not got.any(), s
        elif s not in refused:
            assert np.array_equal(got, levels[lv][1][i]), s
