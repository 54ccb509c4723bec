"""The lane-interleaved rANS layout restated in plain Python integers (no numpy arithmetic, nothing shared with csrc/rans.cpp): what
tests/test_rans_lanes_host.py holds the host coder to, and through it tests/test_gpu_rans_lanes.py the device coder.

A stream codes code[m, hw] with group g's table for the hw symbols of group g, on W independent states over one word sequence.
Read forwards: the prefix 'M' 'Q' 'L' W; 2 W state words, lane 0 first, low word first; then round by round (group after group, round r
of a group holding positions r W + l < hw) the words of the lanes that renormalise, lowest lane first."""
import math
import struct

import numpy as np

L = 1 << 31
WIDTHS = (1, 2, 4, 8, 16, 32, 64)
STEP_SLACK = 4.41e-5            # bits per symbol: -log2(1 - 2^-15), rounded up (tests/test_gpu_code_bits_vs_coder.py derives it)


def auto_width(symbols: int) -> int:
    """The largest power of two <= symbols / 512, clamped to [1, 64]."""
    w = 1
    while w < 64 and 2 * w * 512 <= symbols:
        w *= 2
    return w


def encode(code, tables, W: int) -> bytes:
    """code: m rows of hw ints; tables: m rows of k + 1 ints (cdf[0] = 0 .. cdf[k] = 65536)."""
    assert W in WIDTHS
    m, hw = len(code), len(code[0])
    x = [L] * W
    back = []                                               # words in the order the encoder writes them: the stream's, reversed
    rounds = -(-hw // W)
    for g in reversed(range(m)):
        t = tables[g]
        for r in reversed(range(rounds)):
            for lane in reversed(range(W)):
                p = r * W + lane
                if p >= hw:
                    continue
                c = code[g][p]
                start, freq = t[c], t[c + 1] - t[c]
                assert 0 < freq < 65536
                if x[lane] >= freq << 47:
                    back.append(x[lane] & 0xffffffff)
                    x[lane] >>= 32
                x[lane] = ((x[lane] // freq) << 16) + (x[lane] % freq) + start
    for lane in reversed(range(W)):
        back.append(x[lane] >> 32)
        back.append(x[lane] & 0xffffffff)
    back.append(0x4D | 0x51 << 8 | 0x4C << 16 | W << 24)
    return struct.pack(f"<{len(back)}I", *reversed(back))


def decode(stream: bytes, tables, m: int, hw: int):
    """-> m rows of hw ints, or ValueError for anything the layout's list of malformed inputs names."""
    if len(stream) < 4 or len(stream) % 4:
        raise ValueError("length")
    words = struct.unpack(f"<{len(stream) // 4}I", stream)
    W = words[0] >> 24
    if words[0] & 0xffffff != (0x4D | 0x51 << 8 | 0x4C << 16) or W not in WIDTHS or len(words) < 1 + 2 * W:
        raise ValueError("prefix")
    x = [words[1 + 2 * lane] | words[2 + 2 * lane] << 32 for lane in range(W)]
    at = 1 + 2 * W
    out = [[0] * hw for _ in range(m)]
    for g in range(m):
        t = tables[g]
        k = len(t) - 1
        ta = np.asarray(t, dtype=np.int64)
        for r in range(-(-hw // W)):
            for lane in range(W):
                p = r * W + lane
                if p >= hw:
                    break
                cum = x[lane] & 0xffff
                s = int(np.searchsorted(ta[:k], cum, side="right")) - 1      # the last entry of 0 .. k - 1 that is <= cum
                if not (0 <= s < k and t[s] <= cum < t[s + 1]):
                    raise ValueError("bin")
                x[lane] = (t[s + 1] - t[s]) * (x[lane] >> 16) + cum - t[s]
                if x[lane] < L:
                    if at >= len(words):
                        raise ValueError("out of words")
                    x[lane] = (x[lane] << 32) | words[at]
                    at += 1
                out[g][p] = s
    return out


def ideal_bits(code, tables) -> float:
    """sum over the symbols of 16 - log2(width): what `EntropyCoder.codeBits` returns for the stream."""
    return sum(16.0 - math.log2(tables[g][c + 1] - tables[g][c]) for g, row in enumerate(code) for c in row)


def length_interval(symbols: int, W: int):
    """(low, high): low < 8 len(stream) - ideal_bits <= high.  The derivation of tests/test_gpu_code_bits_vs_coder.py lane by lane: each
    of the W states pays a 64-bit flush of which at most 32 bits were still free, and the prefix adds 32."""
    slack = STEP_SLACK * symbols + symbols * 2.0 ** -44 + 2.0 ** -46
    return 32.0 + 32.0 * W - slack, 32.0 + 64.0 * W + slack


# name -> what it makes of a well-formed stream that holds renormalisation words: every entry of the layout's list of malformed inputs
# that a stream's own bytes can show (offsets and tables are the callers')
MALFORMED = {
    "wrong prefix": lambda s: b"MQX" + s[3:],
    "plain stream": lambda s: s[4:],
    "W = 0": lambda s: s[:3] + b"\x00" + s[4:],
    "W = 3": lambda s: s[:3] + b"\x03" + s[4:],
    "W = 128": lambda s: s[:3] + b"\x80" + s[4:],
    "head cut short": lambda s: s[:4 * (1 + 2 * s[3]) - 4],
    "prefix only": lambda s: s[:4],
    "empty": lambda s: b"",
    "length not a multiple of 4": lambda s: s[:-1],
    "out of words": lambda s: s[:-4],
    "out of words by half": lambda s: s[:len(s) // 8 * 4],
}


def tables(kind: str, m: int, k: int = 512):
    """m rows of k + 1 ints, hand-made (no quantiser): row g is the base row's widths rolled by 3 g, so the groups differ.
    uniform: 65536 / k each.  peaked: one symbol with nearly all the mass, width 1 for every other.  ones: k - 1 symbols of width 1
    (widths that are all 1 sum to 65536 only at k = 65536) and one wide symbol that `draw` never uses, so every CODED symbol has width
    1.  halfdead: every second symbol width 1 (the quantiser's floor for a dead one), the others share the rest unevenly."""
    if kind == "uniform":
        widths = [65536 // k] * k
    elif kind == "peaked":
        widths = [65536 - (k - 1)] + [1] * (k - 1)
    elif kind == "ones":
        widths = [1] * (k - 1) + [65536 - (k - 1)]
    elif kind == "halfdead":
        live = k // 2
        base = [(i % 7 + 1) * 16 for i in range(live)]
        widths = []
        for i in range(live):
            widths += [base[i], 1]
        widths[0] += 65536 - sum(widths)
    else:
        raise KeyError(kind)
    assert sum(widths) == 65536 and min(widths) >= 1 and len(widths) == k
    rows = []
    for g in range(m):
        wg = widths[-3 * g:] + widths[:-3 * g] if g else list(widths)
        row = [0]
        for w in wg:
            row.append(row[-1] + w)
        rows.append(row)
    return rows


def draw(kind: str, rows, hw: int, rng) -> list:
    """m rows of hw codes under `rows`: uniform / halfdead from the table's own distribution, peaked the wide symbol (no lane emits for
    many rounds), ones only width-1 symbols (every lane emits every round)."""
    out = []
    for t in rows:
        widths = np.diff(np.asarray(t, dtype=np.int64))
        if kind == "peaked":
            out.append([int(widths.argmax())] * hw)
        elif kind == "ones":
            ones = np.flatnonzero(widths == 1)
            out.append([int(v) for v in rng.choice(ones, size=hw)])
        else:
            out.append([int(v) for v in rng.choice(len(widths), size=hw, p=widths / 65536.0)])
    return out
