"""`EntropyCoder.codeBits` against the byte streams of `compress`: for every image and level, 8 * len(stream) - codeBits lies in an
interval that follows from the coder (csrc/rans.cpp), not from a measurement.

The coder keeps one 64-bit state x, starts at x0 = L = 2^31 and codes N symbols of widths f_i (probability f_i / 2^16).  Before a
symbol it emits the low 32 bits of x (one word, x >>= 32) when x >= 2^47 f; then x' = floor(x / f) 2^16 + (x mod f) + start.  At the end
it writes x itself: 64 bits.  With W words emitted the stream has B = 32 W + 64 bits.
  * The state.  After a word is emitted x >= 2^15 f, and without one x >= 2^31 > 2^15 f as well; so x / f >= 2^15 in every coding step and
    floor(x / f) 2^16 <= x' < (floor(x / f) + 1) 2^16 gives  log2 x' = log2 x + (16 - log2 f) + e,  |e| <= -log2(1 - 2^-15) < 4.41e-5.
    Also 2^31 <= x' < 2^63 + 2^16 after every step.
  * Summed over the stream:  log2 x_end = 31 - 32 W + S + E,  S = sum_i (16 - log2 f_i) (what codeBits returns), |E| < 4.41e-5 N.
  * So  B - S = 95 - log2 x_end + E  with 31 <= log2 x_end < 63 + 2^-46:   32 - 4.41e-5 N - 2^-46 < B - S <= 64 + 4.41e-5 N.
The lower end is the flush (64 bits) less what the state can still hold above L (32 bits): the stream is never shorter than the
estimate; the upper end is the flush alone: the renormalisation words are paid for by the state.  codeBits' own rounding (N 2^-44,
tests/test_gpu_code_bits.py) widens both ends.  No bypass symbol occurs: the tables' sentinel slot is k, which no code in [0, k)
reaches (codeBits does not model that path)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STEP_SLACK = 4.41e-5            # bits per symbol: -log2(1 - 2^-15) = 4.4028e-5, rounded up


def stream_minus_estimate_interval(symbols: int):
    """(low, high) for 8 * len(stream) - codeBits of one image and level holding `symbols` codes."""
    slack = STEP_SLACK * symbols + symbols * 2.0 ** -44 + 2.0 ** -46
    return 32.0 - slack, 64.0 + slack


def small_model(dev, seed=3407):
    """Compressor(32, 2, [64, 32, 16]) with random weights and frequency rows that are far from uniform (some symbols unused)."""
    from mcquic_amd import Compressor
    torch.manual_seed(seed)
    model = Compressor(32, 2, [64, 32, 16]).eval().to(dev)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for f in model._quantizer._entropyCoder._freqEMA:
            r = torch.rand(f.shape, generator=g) ** 6
            r[0, torch.rand(f.shape[1], generator=g) < 0.3] = 0.0
            f.copy_((r + 1e-9).to(dev))
    return model


def test_stream_lengths_lie_in_the_derived_interval(dev):
    model = small_model(dev)
    coder = model._quantizer._entropyCoder
    x = (torch.rand((4, 3, 64, 48), generator=torch.Generator().manual_seed(1)) * 2 - 1).to(dev)
    codes = model.encode(x)
    binaries, _ = coder.compress(codes)
    bits = coder.codeBits(codes).cpu().numpy()
    assert not coder.codeBitsError().cpu().numpy().any()
    diffs = []
    for lv, code in enumerate(codes):
        symbols = code[0].numel()
        low, high = stream_minus_estimate_interval(symbols)
        for i in range(code.shape[0]):
            d = 8 * len(binaries[i][lv]) - bits[i, lv]
            diffs.append(d)
            assert low <= d <= high, (i, lv, symbols, d, low, high)
    print(f"8 * len(stream) - codeBits over {len(diffs)} streams: min {min(diffs):.4f}, max {max(diffs):.4f} bits")
    # a longer stream, so that words are emitted: ten images' worth of symbols in one level-0 map
    g = torch.Generator().manual_seed(2)
    long_codes = [torch.randint(0, k, (2, 2, 48 >> lv, 32 >> lv), generator=g).to(dev) for lv, k in enumerate((64, 32, 16))]
    binaries, _ = coder.compress(long_codes)
    bits = coder.codeBits(long_codes).cpu().numpy()
    more = []
    for lv, code in enumerate(long_codes):
        low, high = stream_minus_estimate_interval(code[0].numel())
        for i in range(2):
            d = 8 * len(binaries[i][lv]) - bits[i, lv]
            more.append(d)
            assert len(binaries[i][lv]) > 8 or lv > 0
            assert low <= d <= high, (i, lv, d, low, high)
    print(f"48x32 maps: min {min(more):.4f}, max {max(more):.4f} bits")
