"""The lane-interleaved stream layout without a GPU: the host coder (csrc/rans.cpp, mcq_rans_lanes_*_batch) against a plain-Python
restatement of the layout (tests/_rans_lanes_ref.py), byte for byte, for every width, the lengths around a round and a group seam, and
four hand-made tables; W = 1 against the plain coder; the auto rule; the length interval against the tables' ideal code length; every
malformed input of the layout's list; and a stand-alone build of the coder under the address and undefined-behaviour sanitizers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import _rans_lanes_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 512
KINDS = ("uniform", "peaked", "ones", "halfdead")


def _lengths(W):
    """hw around a round of the widest stream and two of them, and one below W (a round that no lane of the upper half joins)."""
    return [1, 63, 64, 65, 127, 129] + ([max(1, W // 2 - (W > 2))] if W > 1 else [])


def _case(kind, m, hw, seed):
    rows = R.tables(kind, m, K)
    return rows, R.draw(kind, rows, hw, np.random.default_rng(seed))


@pytest.mark.parametrize("m", [1, 2, 3])
@pytest.mark.parametrize("kind", KINDS)
def test_host_coder_equals_the_python_reference(kind, m):
    from mcquic_amd.modules.entropyCoder import ransLanesDecodeBatch, ransLanesEncodeBatch
    checked = 0
    for W in R.WIDTHS:
        for hw in _lengths(W):
            rows, code = _case(kind, m, hw, 1000 * W + hw)
            want = R.encode(code, rows, W)
            symbols = np.asarray(code, dtype=np.int32).reshape(1, m * hw)
            cdfs = np.asarray(rows, dtype=np.uint32)
            got = ransLanesEncodeBatch(symbols, m, hw, cdfs, W)[0]
            assert got == want, (kind, m, W, hw, len(got), len(want))
            assert got[:4] == b"MQL" + bytes([W]) and len(got) <= 4 * (1 + 2 * W + m * hw)
            assert R.decode(got, rows, m, hw) == code
            assert ransLanesDecodeBatch([got], m, hw, cdfs).reshape(m, hw).tolist() == code
            low, high = R.length_interval(m * hw, W)
            d = 8 * len(got) - R.ideal_bits(code, rows)
            assert low < d <= high, (kind, m, W, hw, d, low, high)
            if kind == "peaked" and m * hw * np.log2(65536 / (65536 - (K - 1))) < 31:
                assert len(got) == 4 * (1 + 2 * W)              # no lane ever emits: the stream is its head
            checked += 1
    assert checked == 6 + 6 * 7


def test_several_streams_in_one_call_and_threads_do_not_change_the_bytes():
    from mcquic_amd.modules.entropyCoder import ransLanesDecodeBatch, ransLanesEncodeBatch
    m, hw, n = 2, 9000, 5
    rows = R.tables("halfdead", m, K)
    g = np.random.default_rng(3)
    codes = [R.draw("halfdead", rows, hw, g) for _ in range(n)]
    symbols = np.asarray(codes, dtype=np.int32).reshape(n, m * hw)
    cdfs = np.asarray(rows, dtype=np.uint32)
    one = ransLanesEncodeBatch(symbols, m, hw, cdfs, "auto", threads=1)
    many = ransLanesEncodeBatch(symbols, m, hw, cdfs, "auto", threads=4)
    assert one == many and all(b[3] == R.auto_width(m * hw) == 32 for b in one)
    assert one[0] == R.encode(codes[0], rows, 32)
    assert np.array_equal(ransLanesDecodeBatch(one, m, hw, cdfs, threads=4), symbols)


@pytest.mark.parametrize("kind", KINDS)
def test_one_lane_is_the_prefix_and_the_plain_stream(kind):
    from mcquic_amd.modules.entropyCoder import _Tables, ransEncodeBatchWithIndexes, ransLanesEncodeBatch
    for m in (1, 2, 3):
        for hw in (1, 65, 700):
            rows, code = _case(kind, m, hw, 17 * m + hw)
            symbols = np.asarray(code, dtype=np.int32).reshape(1, m * hw)
            plain = ransEncodeBatchWithIndexes(symbols, np.repeat(np.arange(m, dtype=np.int32), hw), _Tables(rows, K))[0]
            lanes = ransLanesEncodeBatch(symbols, m, hw, np.asarray(rows, dtype=np.uint32), 1)[0]
            assert lanes == b"MQL\x01" + plain, (kind, m, hw)


def test_the_auto_rule():
    from mcquic_amd.modules.entropyCoder import lanesAuto
    want = {1: 1, 511: 1, 512: 1, 1023: 1, 1024: 2, 32767: 32, 32768: 64, 10 ** 6: 64}
    for symbols, w in want.items():
        assert lanesAuto(symbols) == w == R.auto_width(symbols), symbols
        assert w * 512 <= max(symbols, 512) and (w == 64 or 2 * w * 512 > symbols)
        assert 8 * w <= max(symbols, 512) / 64 or w == 1        # the 2 W flush words: at most 1/8 bit per symbol


def _stream(W=4, m=3, hw=700):
    from mcquic_amd.modules.entropyCoder import ransLanesEncodeBatch
    rows, code = _case("halfdead", m, hw, 99)
    cdfs = np.asarray(rows, dtype=np.uint32)
    stream = ransLanesEncodeBatch(np.asarray(code, dtype=np.int32).reshape(1, -1), m, hw, cdfs, W)[0]
    assert len(stream) > 4 * (1 + 2 * W) + 64
    return stream, cdfs, rows, code


MALFORMED = R.MALFORMED


@pytest.mark.parametrize("how", list(MALFORMED))
def test_the_host_decoder_refuses_malformed_streams(how):
    from mcquic_amd.modules.entropyCoder import ransLanesDecodeBatch
    stream, cdfs, rows, code = _stream()
    bad = MALFORMED[how](stream)
    with pytest.raises(ValueError):
        R.decode(bad, rows, 3, 700)
    out = np.full((3, 3 * 700), 7, dtype=np.int32)
    with pytest.raises(RuntimeError, match="truncated or malformed"):
        ransLanesDecodeBatch([stream, bad, stream], 3, 700, cdfs, out=out)
    assert out[0].reshape(3, 700).tolist() == code == out[2].reshape(3, 700).tolist(), "the neighbours decode"
    assert not out[1].any(), "a refused stream leaves zeros"


def test_a_bin_that_does_not_contain_cum_is_refused():
    from mcquic_amd.modules.entropyCoder import ransLanesDecodeBatch
    stream, cdfs, _, _ = _stream()
    # The bisection ends between two entries it has compared with cum, so only the table's ends can fail to bracket it: entry 0 above
    # cum here.  Symbol 0 holds three quarters of the half-dead table's mass, so the first rounds meet it.
    broken = cdfs.copy()
    broken[:, 0] = 65535
    with pytest.raises(RuntimeError, match="truncated or malformed"):
        ransLanesDecodeBatch([stream], 3, 700, broken)


@pytest.mark.parametrize("how", ["past the blob", "decreasing", "negative"])
def test_offsets_outside_the_blob_are_refused(how):
    from mcquic_amd import _lib
    stream, cdfs, _, code = _stream()
    blob = np.frombuffer(stream + stream, dtype=np.uint8).copy()
    n = len(stream)
    offs = {"past the blob": [0, n, 2 * n + 4], "decreasing": [0, n, n - 8], "negative": [-4, n, 2 * n]}[how]
    refused = {"past the blob": 1, "decreasing": 1, "negative": 0}[how]
    offs = np.asarray(offs, dtype=np.int64)
    out = np.full((2, 3 * 700), 7, dtype=np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = _lib.load().mcq_rans_lanes_decode_batch(vp(blob), blob.size, vp(offs), 2, 3, 700, vp(cdfs), K, vp(out), 1)
    assert rc == _lib.MCQ_EINVAL
    assert not out[refused].any() and out[1 - refused].reshape(3, 700).tolist() == code


def test_bad_arguments_of_the_host_entry_points():
    from mcquic_amd import _lib
    from mcquic_amd.modules.entropyCoder import ransLanesEncodeBatch
    lib = _lib.load()
    _, cdfs, _, code = _stream()
    sym = np.asarray(code, dtype=np.int32).reshape(1, -1)
    for lanes in (3, 128, -1, True, "wide", None):
        with pytest.raises(ValueError, match="lanes"):
            ransLanesEncodeBatch(sym, 3, 700, cdfs, lanes)
    for at, value in ((5, K), (2099, -1)):
        bad = sym.copy()
        bad[0, at] = value
        with pytest.raises(RuntimeError, match="rANS encode failed"):
            ransLanesEncodeBatch(bad, 3, 700, cdfs, 8)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    out = np.empty(4 * (1 + 128 + 2100), dtype=np.uint8)
    size = np.zeros(1, dtype=np.int64)
    ok = dict(symbols=vp(sym), n=1, m=3, hw=700, cdfs=vp(cdfs), k=K, lanes=4, out=vp(out), stride=out.size, sizes=vp(size), threads=1)
    assert lib.mcq_rans_lanes_encode_batch(*ok.values()) == _lib.MCQ_OK
    for change in (dict(symbols=None), dict(cdfs=None), dict(out=None), dict(sizes=None), dict(m=0), dict(hw=0), dict(k=0), dict(lanes=5),
                   dict(lanes=128), dict(lanes=-2), dict(stride=32)):
        assert lib.mcq_rans_lanes_encode_batch(*{**ok, **change}.values()) == _lib.MCQ_EINVAL, change
    assert lib.mcq_rans_lanes_encode_batch(*{**ok, "hw": _lib.MCQ_RANS_DEV_MAX_SYMBOLS}.values()) == _lib.MCQ_ETOOLARGE
    assert lib.mcq_rans_lanes_encode_batch(*{**ok, "stride": 4 * (1 + 8 + 100)}.values()) == _lib.MCQ_ETOOLARGE, "a slot the stream outgrows"


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    """tests/rans_lanes_host_main.cpp (which includes csrc/rans.cpp: no HIP header is needed) built with the host compiler under
    -fsanitize=address,undefined; the program carries its own main, so nothing is preloaded."""
    cxx = next((c for c in (shutil.which("g++"), shutil.which("c++"), shutil.which("clang++"), "/opt/rocm/lib/llvm/bin/clang++") if c and os.path.exists(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("rans_lanes") / "rans_lanes_host_main")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "rans_lanes_host_main.cpp")], check=True)
    return exe


def test_stand_alone_host_build_under_the_sanitizers(program):
    run = subprocess.run([program], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    words = run.stdout.split()
    assert words[0] == "ok" and int(words[1]) == 8 * 7 * 3 and int(words[2]) >= 15, run.stdout
