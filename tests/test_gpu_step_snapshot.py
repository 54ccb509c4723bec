"""mcquic_amd.monitor.StepSnapshot (csrc/step_snapshot.hip) on a small Compressor(8, 2, [64, 32, 16]) and one 64 x 64 batch of 2: every
`read()` key against the CPU references of tests/_snapshot_ref.py computed from the same tensors, the single device-to-host copy, capture
inside a hipGraph with fresh inputs at replay, and the refusals.

Exact: the histogram (counts and edges against np.histogram of the unfused kernel's output on the same slab, which
tests/test_gpu_histogram_leaf.py pins element by element), the code images, the two de-transformed images, CodeUsage.  The normalised frequencies are held to
2 float32 spacings: the row sum is rounded to float32 once, from a double sum here and from an exact sum in the reference, which can fall
on either side of a rounding boundary (one spacing of the sum, at most two of the quotient)."""
import numpy as np
import pytest
import torch

import _snapshot_ref as R

pytestmark = pytest.mark.gpu
CH, KS, HW, N = 8, [64, 32, 16], 64, 2
KEYS = ["Hist/LogDistance"] + [f"Hist/{kind}Lv{l:02d}" for l in range(3) for kind in ("Freq", "Code")] + ["Train/Raw", "Train/Res", "Stat/CodeUsage"]


def _model(dev, seed=5):
    from mcquic_amd import Compressor
    torch.manual_seed(seed)
    model = Compressor(CH, 2, KS).to(dev).train()
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():                                      # frequency tables that are not uniform, with unused entries
        for f in model._quantizer._entropyCoder._freqEMA:
            t = torch.rand(f.shape, generator=g)
            t[:, ::5] = 0.0
            t[1, 1] = 1e-9
            f.copy_(t.to(dev))
    return model


def _batch(dev, seed):
    return (torch.rand((N, 3, HW, HW), generator=torch.Generator().manual_seed(seed)) * 2 - 1).to(dev)


def _forward(model, x):
    with torch.no_grad():
        xHat, _, codes, logits = model(x)
    return xHat.contiguous(), [c.contiguous() for c in codes], [lg.contiguous() for lg in logits]


def check_payload(payload, snap, model, images, restored, codes, logits, keep):
    """Every key of `payload` against the references computed from the tensors it was made from."""
    from mcquic_amd import ops
    assert list(payload) == KEYS
    # the histogram: fused == np.histogram of the unfused kernel's output (bit for bit), and of torch's float32 ops where those agree
    slab = logits[0][0, 0]
    v = ops.log_distance(slab, R.EPS).cpu().numpy().reshape(-1)
    counts, edges = payload["Hist/LogDistance"]
    want_counts, want_edges, stats = R.histogram(v, snap.bins)
    assert edges.dtype == np.float64 and counts.dtype == np.int64 and counts.shape == (snap.bins,) and edges.shape == (snap.bins + 1,)
    assert edges.tobytes() == want_edges.tobytes() and counts.tolist() == want_counts.tolist()
    assert snap.stats == stats == (slab.numel(), 0) and int(counts.sum()) == slab.numel()
    np_counts, np_edges = np.histogram(v.astype(np.float64), snap.bins)
    assert edges.tobytes() == np_edges.tobytes() and counts.tolist() == np_counts.tolist()
    # frequencies and CodeUsage
    freqs = [f.detach().cpu().numpy() for f in model._quantizer._entropyCoder._freqEMA]
    rows, usage = R.normalized_freq(freqs)
    for l, (row, k) in enumerate(zip(rows, KS)):
        got, bounds = payload[f"Hist/FreqLv{l:02d}"]
        assert got.dtype == np.float32 and got.shape == (k,) and bounds.tolist() == np.arange(0.5, k + 1.5, 1.0).tolist()
        assert (got[row == 0] == 0).all()
        assert R.ulp_distance(got, row.astype(np.float64)) <= 2.0, l
        assert np.allclose(got, model.NormalizedFreq[l][0].cpu().numpy(), rtol=8 * 2.0 ** -24, atol=0)
    assert payload["Stat/CodeUsage"] == float(usage)
    # (torch's device `mean` is the count times a reciprocal or over the size: within one float32 spacing of the quotient either way)
    assert abs(payload["Stat/CodeUsage"] - float(model.CodeUsage)) <= float(np.spacing(np.float32(usage)))
    assert isinstance(payload["Stat/CodeUsage"], float)
    # pictures
    for l, c in enumerate(codes):
        got = payload[f"Hist/CodeLv{l:02d}"]
        assert got.dtype == np.uint8 and np.array_equal(got, R.code_image(c, keep=keep).numpy()), l
    for key, t in (("Train/Raw", images), ("Train/Res", restored)):
        assert payload[key].dtype == np.uint8 and payload[key].shape == (keep, 3, HW, HW)
        assert np.array_equal(payload[key], R.detransform(t[:keep].cpu()).numpy()), key


@pytest.mark.parametrize("images", [1, None], ids=["first-image", "all-images"])
def test_every_key_against_the_cpu_references(dev, images):
    from mcquic_amd import monitor
    model = _model(dev)
    x = _batch(dev, 1)
    xHat, codes, logits = _forward(model, x)
    assert [tuple(c.shape) for c in codes] == [(N, 2, 4, 4), (N, 2, 2, 2), (N, 2, 1, 1)] and tuple(logits[0].shape) == (N, 2, 4, 4, 64)
    snap = monitor.StepSnapshot(model, batch_shape=(N, 3, HW, HW), bins=64, images=images)
    snap.prepare()
    snap.capture(x, xHat, codes, logits)
    payload = snap.read()
    check_payload(payload, snap, model, x, xHat, codes, logits, N if images is None else images)
    assert 0.5 < payload["Stat/CodeUsage"] < 0.9, "a fifth of the entries and one more are unused in these tables"


def test_read_is_one_device_to_host_copy_and_capture_is_none(dev, monkeypatch):
    """`capture` moves nothing to the host and allocates nothing on the device; `read` makes exactly one copy (one `.cpu()` of one device
    tensor, and no other route off the device)."""
    from mcquic_amd import monitor
    model = _model(dev)
    x = _batch(dev, 2)
    xHat, codes, logits = _forward(model, x)
    snap = monitor.StepSnapshot(model, batch_shape=(N, 3, HW, HW), bins=64, images=1)
    snap.prepare()
    snap.capture(x, xHat, codes, logits)                       # (first launches)
    calls = []
    for name in ("cpu", "to", "item", "tolist", "numpy", "__int__", "__float__", "__bool__", "__index__", "copy_"):
        orig = getattr(torch.Tensor, name)

        def spy(self, *a, _orig=orig, _name=name, **kw):
            if self.is_cuda or any(torch.is_tensor(t) and t.is_cuda for t in a):
                calls.append(_name)
            return _orig(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, spy)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    snap.capture(x, xHat, codes, logits)
    assert calls == [], calls
    assert torch.cuda.memory_stats(dev)["allocation.all.allocated"] == before, "capture allocated device memory"
    payload = snap.read()
    assert calls == ["cpu"], calls
    monkeypatch.undo()
    check_payload(payload, snap, model, x, xHat, codes, logits, 1)


def test_capture_inside_a_graph_reads_its_inputs_at_replay(dev):
    from mcquic_amd import monitor
    model = _model(dev)
    sx, sxh = torch.zeros((N, 3, HW, HW), device=dev), torch.zeros((N, 3, HW, HW), device=dev)
    x0 = _batch(dev, 3)
    xh0, c0, l0 = _forward(model, x0)
    scodes, slogits = [torch.zeros_like(c) for c in c0], [torch.zeros_like(lg) for lg in l0]
    snap = monitor.StepSnapshot(model, batch_shape=(N, 3, HW, HW), bins=64, images=2)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    snap.prepare()
    snap.capture(sx, sxh, scodes, slogits)                     # (the kernels' first launch, outside the capture)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        snap.capture(sx, sxh, scodes, slogits)
    seen = []
    for seed in (3, 4):
        x = _batch(dev, seed)
        xHat, codes, logits = _forward(model, x)
        sx.copy_(x); sxh.copy_(xHat)
        for s, c in zip(scodes, codes):
            s.copy_(c)
        slogits[0].copy_(logits[0])
        g.replay()
        payload = snap.read()
        check_payload(payload, snap, model, x, xHat, codes, logits, 2)
        seen.append(payload["Train/Res"].tobytes() + payload["Hist/LogDistance"][1].tobytes())
    assert seen[0] != seen[1]


def test_capture_before_prepare_is_refused_inside_a_capture(dev):
    """The buffer cannot be allocated inside a graph: the call raises before it launches anything (the capture ends empty)."""
    from mcquic_amd import monitor
    model = _model(dev)
    x = _batch(dev, 1)
    xHat, codes, logits = _forward(model, x)
    fresh = monitor.StepSnapshot(model, batch_shape=(N, 3, HW, HW))
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError, match="before capturing"):
        with torch.cuda.graph(torch.cuda.CUDAGraph(), stream=side):
            fresh.capture(x, xHat, codes, logits)
    torch.cuda.synchronize()
    fresh.prepare()
    fresh.capture(x, xHat, codes, logits)
    check_payload(fresh.read(), fresh, model, x, xHat, codes, logits, 2)


def test_refusals(dev):
    from mcquic_amd import monitor
    model = _model(dev)
    x = _batch(dev, 1)
    xHat, codes, logits = _forward(model, x)
    snap = monitor.StepSnapshot(model, batch_shape=(N, 3, HW, HW))
    with pytest.raises(RuntimeError, match="nothing was captured"):
        snap.read()
    with pytest.raises(RuntimeError, match="HIP device"):
        snap.capture(x.cpu(), xHat, codes, logits)
    with pytest.raises(TypeError, match="float32"):
        snap.capture(x.double(), xHat, codes, logits)
    with pytest.raises(ValueError, match="contiguous"):
        snap.capture(x, xHat.transpose(2, 3), codes, logits)
    with pytest.raises(ValueError, match="contiguous"):
        snap.capture(x[:1], xHat, codes, logits)
    with pytest.raises(ValueError, match="code levels"):
        snap.capture(x, xHat, codes[:2], logits)
    with pytest.raises(TypeError, match="int64"):
        snap.capture(x, xHat, [c.int() for c in codes], logits)
    assert monitor.StepSnapshot(model, batch_shape=(N, 3, HW, HW), images=4).keep == N
    for bad in (dict(images=0), dict(bins=0), dict(bins=4097), dict(code_shapes=[(4, 4)])):
        with pytest.raises(ValueError):
            monitor.StepSnapshot(model, batch_shape=(N, 3, HW, HW), **bad)
    with pytest.raises(ValueError):
        monitor.StepSnapshot(model, batch_shape=(N, 1, HW, HW))
