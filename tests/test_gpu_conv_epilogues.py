"""GPU: every epilogue of the fused convolution on every wave tile, against the float64 references of tests/_conv_refs.py (held to
torch / autograd on the CPU by tests/test_conv_refs.py).

conv_mfma_kernel's epilogue is six separately written paths (three-phase band epilogue, pixel-pair epilogues, the run-time-flag path
with plain and with PixelShuffle stores, the three backward pairs, all of them again behind the split-K reduction) and conv_t16_kernel
carries a seventh.  (An eighth, the POST section of conv_mfma_kernel -- the fused 1x1 layer behind a 3x3 convolution, MCQ_CONV_POST_* --
is pinned by the same method in tests/test_gpu_conv_post_epilogues.py, which imports this file's launch and guard helpers.)  The tests elsewhere hold them at `max |err| <= 2e-6 max |ref|` on the launcher's own tile, which a wrong operand
in one register, a side tensor read at the unshuffled address or a dropped res_scale on one path passes.  Here every row of ROWS
(one epilogue = one keyword set of ops._conv_desc) runs on every tile of TILES at every geometry of GEOMS, and every launch is held
to two assertions:

  (a) the epilogue alone: the same tile and split without epilogue flags gives v_gpu (accumulator + bias as THIS instance sums it);
      the epilogue launch must be out64(v_gpu, sides) to within the float32 formula's own error -- the same BITS as
      out_f32(v_gpu, sides) where no expf is involved, else float32 ulps at the float64 value (R.ulp_err in out_scale64's scale)
      within 4x the worst error of out_f32 over the same inputs, aggregated per tile class as tests/test_gpu_leaf_ops.py does;
  (b) the whole launch: e_hip = max |got - out64(conv64, sides)| / scale against e_seq, the same figure for
      out_f32(conv_seq_f32, sides) -- ONE float32 chain over all of K, at least as long as any chain a tile forms --
      e_hip <= max(4 e_seq, 1.2e-7), the bar of tests/test_gpu_group_norm_leaf.py.

Every output lies between guard bands, every input is compared with a clone afterwards, and the launcher's routing is part of the
test: `_plan` is the table of what each (epilogue, tile, geometry) does -- runs as asked, is rerouted to another instance (then it
must return that instance's bits), or is refused with MCQ_EINVAL -- and the number of distinct instances every row ran is asserted
against a literal, so that an edit of the table cannot shrink the coverage unnoticed.

Measured on an MI355X (profiles/r10_conv_epilogue_errors.json, 363 entries conv_epilogue[<row>][<tile class>]): the one-chain sum IS a
yardstick for these tiles -- over every row and tile class e_hip / e_seq is at most 1.36 (res on the pair form: 2.0e-7 against
1.5e-7), the largest e_hip 3.8e-7 for y and 7.3e-7 for a second output (d s of GDN_BWD, whose scale the derivative shrinks) next to
e_seq of 4.2e-7 and 8.3e-7; a split shortens the chains and lands at a third to a half of e_seq.  (a): every expf-free y and d s
equals the float32 restatement bit for bit; with expf the kernel's worst is the formula's own on most rows (7.2 ulp for * silu'(m),
7.2 against 7.2) and at most 1.52 x it (the twin, mcq_silu's compensated exp2 / rcp: 2.46 against 1.62 ulp on the special values)."""
import ctypes

import pytest
import torch

import _conv_refs as C
import _leaf_refs as R
from _record import record

pytestmark = pytest.mark.gpu

GUARD = 1 << 15                 # floats on both sides of every output: more than the 120 rows x 70 pixels a 128-row tile reaches past Cout = 136
FILL_Y, FILL_TWIN = 7.5, -3.25
FLOOR_B = 1.2e-7                # two float32 roundings: the floor of bar (b)

# ---- tiles -------------------------------------------------------------------------------------------------------------------------------
# tile = (log2 split-K << 8) | (MB << 4) | NB, bit 0x400 = the pixel-pair form of 0x42
BASE_TILES = (0x42, 0x41, 0x22, 0x21, 0x14, 0x12, 0x11)
TILES = tuple(t | (ksl << 8) for t in BASE_TILES for ksl in range(4)) + (0x442,)

# ---- geometries: the smallest at which each index can go wrong; N = 2 everywhere (the second image's slab is addressed) --------------------
# Cout follows the tile height: 136 for the 128-row tiles (one full tile plus 8 rows: 120 rows past Cout that must be neither read from
# res / mul nor written), 40 for the 64- and 32-row tiles (a full band plus 8 rows); both are multiples of 4 for the PixelShuffle store.
# `split`: what launch_tile makes of a requested split 0..3 per tile height -- a slice needs 8 whole channel pairs and a split at
# least as many slices as the tile has bands; 1x1 layers are never split.  Cin = 20 (10 pairs, Cin % 8 = 4: the channel-pair padding
# is live) allows none; Cin = 128 (64 pairs) is the smallest at which split 3 has its eight pairs per slice.
NO_SPLIT = {4: (0, 0, 0, 0), 2: (0, 0, 0, 0), 1: (0, 0, 0, 0)}
SPLIT64 = {4: (0, 2, 2, 3), 2: (0, 1, 2, 3), 1: (0, 1, 2, 3)}
GEOMS = {
    "odd7x9": dict(cin=20, h=7, w=9, ks=3, stride=1, split=NO_SPLIT),         # Ho Wo = 63: no multiple of 32, odd Wo
    "pair5x14": dict(cin=20, h=5, w=14, ks=3, stride=1, split=NO_SPLIT),      # even Wo, 7 pairs a row: no multiple of any pair block
    "tiny3x3": dict(cin=128, h=3, w=3, ks=3, stride=1, split=SPLIT64),        # a map smaller than one block; every split live
    "s2_7x10": dict(cin=20, h=7, w=10, ks=3, stride=2, split=NO_SPLIT),       # stride 2 from an odd and an even input side -> 4 x 5
    "k1_7x9": dict(cin=20, h=7, w=9, ks=1, stride=1, split=NO_SPLIT),         # 1x1
}
ALL5 = ("odd7x9", "pair5x14", "tiny3x3", "s2_7x10", "k1_7x9")
ONLY3X3 = ("odd7x9", "pair5x14", "tiny3x3", "s2_7x10")
PAIR_FLAGS = {"silu_out", "res", "res_scale", "dual_silu", "dsilu_mul", "shuffle2"}       # conv_launch.hip: pair_ok

# distinct instances one geometry runs: 7 unsplit tiles (+ the pair form where pair_ok holds); at 64 channel pairs 0x42 / 0x41 at
# splits {0, 2, 3} and the other five at {0, 1, 2, 3}; a backward pair one per tile height (NB = 1, no split)
N_PLAIN, N_PAIR, N_SPLIT64, N_BWD = 7, 8, 26, 3


def _row(name, ep=None, sides=(), pro=None, geoms=ALL5, runs=0, **kw):
    return dict(name=name, ep=ep or {}, sides=tuple(sides), pro=pro, geoms=geoms, runs=runs, **kw)


# `runs`: distinct instances the row must have run = the sum over its geometries (written out, not computed)
R5 = 3 * N_PLAIN + N_PAIR + N_SPLIT64          # ALL5 with the pair form at pair5x14: 55
R5_NOPAIR = 4 * N_PLAIN + N_SPLIT64            # ALL5, an epilogue the pair form does not carry (0x442 is rerouted to 0x42): 54
ROWS = [
    _row("plain", runs=55),
    _row("silu_out", dict(silu_out=True), runs=55),
    _row("dual_silu", dict(dual_silu=True), runs=55),
    _row("res", sides=("res",), runs=55),
    _row("res_scale-1", dict(res_scale=-1.0), ("res",), runs=55),
    _row("res_scale0.5", dict(res_scale=0.5), ("res",), runs=55),
    # (the combinations carry a res_scale other than 1 too: each takes another path than `res` alone on some tile)
    _row("res+dual_silu", dict(dual_silu=True, res_scale=-1.0), ("res",), runs=55),
    _row("res+silu_out", dict(silu_out=True, res_scale=0.5), ("res",), runs=55),
    _row("dsilu_mul", sides=("dsilu_mul",), runs=55),
    _row("dsilu_mul+res", dict(res_scale=-1.0), ("dsilu_mul", "res"), runs=55),
    _row("mul", sides=("mul",), runs=54),
    _row("gate", sides=("gate_mul", "gate_id"), runs=54),
    _row("gate+dual_silu", dict(dual_silu=True), ("gate_mul", "gate_id"), runs=54),
    _row("shuffle2", dict(shuffle2=True), runs=55),
    _row("shuffle2+dsilu_mul", dict(shuffle2=True), ("dsilu_mul",), runs=55),
    _row("shuffle2+dsilu_mul+res", dict(shuffle2=True, res_scale=0.5), ("dsilu_mul", "res"), runs=55),
    # GDN / IGDN: 1x1 with the squaring prologue, weights and bias positive so that v >= 1
    _row("gdn_mul", sides=("gdn_mul",), pro="square", geoms=("k1_7x9",), positive=True, runs=7),
    _row("igdn_mul", sides=("igdn_mul",), pro="square", geoms=("k1_7x9",), positive=True, runs=7),
    # the SiLU prologue exists in the 3x3 instances only (the library refuses it on 1x1: test_refusals); it takes pair_ok away
    _row("silu_in", pro="silu", geoms=ONLY3X3, runs=47),
    _row("silu_in+res+dual_silu", dict(dual_silu=True), ("res",), pro="silu", geoms=ONLY3X3, runs=47),
    _row("silu_in+shuffle2", dict(shuffle2=True), pro="silu", geoms=ONLY3X3, runs=47),
    # PackedConv.dgrad(w, 2): the four-tap walk (TAPS_LR), stored through the shuffle; no pair form
    _row("dgrad2", dict(shuffle2=True), geoms=("odd7x9", "tiny3x3"), dgrad=True, runs=33),
    _row("dgrad2+dsilu_mul+res", dict(shuffle2=True), ("dsilu_mul", "res"), geoms=("odd7x9", "tiny3x3"), dgrad=True, runs=33),
    # the backward pairs: the launcher overrides the forced tile to one pixel block per wave and no split (NB = 1, ksl = 0), so the
    # 29 tiles are three instances; square 1x1 layers for GDN / IGDN (Cin = Cout = the tile height's Cout)
    _row("GDN_BWD", dict(bwd="gdn"), ("m", "g"), pro="square", geoms=("k1_7x9",), positive=True, runs=3),
    _row("IGDN_BWD", dict(bwd="igdn"), ("m", "g"), pro="square", geoms=("k1_7x9",), positive=True, runs=3),
    _row("GATE_BWD", dict(bwd="gate"), ("m", "g"), geoms=("k1_7x9", "tiny1x1"), runs=6),
]
GEOMS["tiny1x1"] = dict(cin=128, h=3, w=3, ks=1, stride=1, split=NO_SPLIT)
assert R5 == 55 and R5_NOPAIR == 54 and 3 * N_PLAIN + N_SPLIT64 == 47 and N_PLAIN + N_SPLIT64 == 33


def _plan(row, gname, tile):
    """The table: ("run", tile) -- the instance asked for exists and runs; ("reroute", other) -- the launcher takes instance `other`
    instead (same bits as a launch that asks for `other`); nothing in ROWS x TILES x GEOMS is refused (test_refusals has those)."""
    g = GEOMS[gname]
    mb, nb, ksl, pair = (tile >> 4) & 15, tile & 15, (tile >> 8) & 3, bool(tile & 0x400)
    if row["ep"].get("bwd"):
        eff = (mb << 4) | 1                                         # NB = 1, no split, no pair form
    else:
        eff = (g["split"][mb][ksl] << 8) | (mb << 4) | nb
        pair_ok = (g["ks"] == 3 and g["stride"] == 1 and g["w"] % 2 == 0 and row["pro"] is None and not row.get("dgrad")
                   and set(row["ep"]) | set(row["sides"]) <= PAIR_FLAGS and eff == 0x42)
        if pair and pair_ok:
            eff |= 0x400
    return ("run", tile) if eff == tile else ("reroute", eff)


def _tile_class(tile):
    return f"{(tile >> 4) & 15}x{tile & 15}" + ("+split" if (tile >> 8) & 3 else "") + ("+pair" if tile & 0x400 else "")


def _cout(tile):
    return 136 if (tile >> 4) & 15 == 4 else 40


# ---- cases: inputs, packed weights and CPU references, built once and shared ---------------------------------------------------------------
_CASES = {}


class _Case:
    def __init__(self, dev, gname, cout, pro, positive, dgrad, square):
        from mcquic_amd import ops
        g = GEOMS[gname]
        self.g, self.stride, self.pro = g, g["stride"], pro
        cin, ks = (cout if square else g["cin"]), g["ks"]
        seed = 1000 + 7 * sum(ord(ch) for ch in gname) + cout
        self.x = R.randn((2, cin, g["h"], g["w"]), seed)
        if dgrad:                                                   # the stride-2 layer [cin, cout / 4, 3, 3] whose input gradient this is
            layer = R.randn((cin, cout // 4, 3, 3), seed + 1, (cin * 9) ** -0.5)
            self.w, self.b = C.dgrad2_weight(layer), None
            self.pk = ops.PackedConv.dgrad(layer.to(dev), 2)
            assert self.pk.lr_taps and (self.pk.cout, self.pk.cin) == (cout, cin)
        else:
            self.w, self.b = R.randn((cout, cin, ks, ks), seed + 1, (cin * ks * ks) ** -0.5), R.randn((cout,), seed + 2, 0.1)
            if positive:
                self.w, self.b = self.w.abs(), self.b.abs() + 1.0
            self.pk = ops.PackedConv(self.w.to(dev), self.b.to(dev))
        self.xd = self.x.to(dev)
        self.v64 = C.conv64(self.x, self.w, self.b, self.stride, pro)
        self.vscale = C.conv_scale64(self.x, self.w, self.b, self.stride, pro)
        self.vseq = C.conv_seq_f32(self.x, self.w, self.b, self.stride, pro)
        self.plain = {}                                             # effective tile -> v_gpu (CPU tensor)
        self._sides = {}

    def sides(self, names, shuffle, special=False):
        """Output-shaped side tensors (the shuffled shape behind a PixelShuffle store); `m` of GDN_BWD / IGDN_BWD is x itself."""
        key = (names, shuffle)
        if key not in self._sides:
            n, c, h, w = self.v64.shape
            shape = (n, c // 4, 2 * h, 2 * w) if shuffle else (n, c, h, w)
            scale = dict(res=1.0, mul=1.0, dsilu_mul=2.0, gate_mul=2.0, gate_id=0.5, gdn_mul=2.0, igdn_mul=2.0, m=2.0, g=1.0)
            self._sides[key] = {k: R.randn(shape, 77 + 13 * i + c, scale[k]) for i, k in enumerate(names)}
        return self._sides[key]


def _case(dev, row, gname, tile):
    square = row["ep"].get("bwd") in ("gdn", "igdn")
    key = (gname, _cout(tile), row["pro"], bool(row.get("positive")), bool(row.get("dgrad")), square)
    if key not in _CASES:
        _CASES[key] = _Case(dev, *key)
    return _CASES[key]


# ---- launches ---------------------------------------------------------------------------------------------------------------------------
def _guarded(numel, fill, dev):
    buf = torch.full((GUARD + numel + GUARD,), fill, device=dev)
    return buf, buf[GUARD:GUARD + numel]


def _guards_ok(buf, numel, fill):
    return bool((buf[:GUARD] == fill).all() & (buf[GUARD + numel:] == fill).all())


def _launch(case, tile, ep, sides_dev):
    """One launch of ops._conv_desc's descriptor with y (and the twin) inside guard bands -> (status, y, twin, section mask)."""
    from mcquic_amd import _lib, ops
    kw = {k: v for k, v in ep.items() if k != "bwd"}
    if case.pro:
        kw["silu_in" if case.pro == "silu" else "square_in"] = True
    d, y, y2, keep = ops._conv_desc(case.xd, case.pk, case.stride, tile=tile, **kw, **sides_dev)
    ybuf, yv = _guarded(y.numel(), FILL_Y, y.device)
    d.y = yv.data_ptr()
    tbuf = tv = None
    if y2 is not None:
        tbuf, tv = _guarded(y.numel(), FILL_TWIN, y.device)
        d.y_silu = tv.data_ptr()
    ops.section_trace(True)
    rc = _lib.load().mcq_conv2d_f32(ctypes.byref(d), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    sec = ops.sections_used(case.pk)
    ops.section_trace(False)
    if rc != 0:
        return rc, None, None, sec
    assert _guards_ok(ybuf, y.numel(), FILL_Y), f"tile {tile:#x}: guard band of y written"
    assert tbuf is None or _guards_ok(tbuf, y.numel(), FILL_TWIN), f"tile {tile:#x}: guard band of the twin written"
    return 0, yv.view(y.shape).cpu(), (None if tv is None else tv.view(y.shape).cpu()), sec


def _launch_bwd(case, tile, kind, sides_dev):
    """ops.conv2d_gdn_bwd / ops.conv2d_gate_bwd at a forced tile, and the same descriptor once more with both outputs inside guard
    bands (the two entry points allocate their own outputs): the same bits, guards untouched."""
    from mcquic_amd import _lib, ops
    ops.section_trace(True)
    if kind == "gate":
        (o1, o2), = ops.conv2d_gate_bwd([case.xd], [case.pk], [sides_dev["m"]], [sides_dev["g"]], tile=tile)
        flags = ops.CONV_GATE_BWD
    else:
        o1, o2 = ops.conv2d_gdn_bwd(case.xd, case.pk, sides_dev["g"], kind == "igdn", tile=tile)
        flags = ops.CONV_SQUARE_IN | (ops.CONV_IGDN_BWD if kind == "igdn" else ops.CONV_GDN_BWD)
    torch.cuda.synchronize()
    sec = ops.sections_used(case.pk)
    ops.section_trace(False)
    n, c, h, w = case.xd.shape
    b1, g1 = _guarded(o1.numel(), FILL_Y, o1.device)
    b2, g2 = _guarded(o1.numel(), FILL_TWIN, o1.device)
    d = _lib.ConvDesc(case.xd.data_ptr(), case.pk.wp.data_ptr(), case.pk.bias.data_ptr(), g1.data_ptr(), g2.data_ptr(), sides_dev["g"].data_ptr(),
                      sides_dev["m"].data_ptr(), None, n, c, h, w, case.pk.cout, 1, 1, flags, 1.0, tile)
    rc = _lib.load().mcq_conv2d_f32(ctypes.byref(d), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(g1.view(o1.shape), o1) and torch.equal(g2.view(o1.shape), o2), f"tile {tile:#x}: the guarded launch differs"
    assert _guards_ok(b1, o1.numel(), FILL_Y) and _guards_ok(b2, o1.numel(), FILL_TWIN), f"tile {tile:#x}: guard band written"
    return 0, o1.cpu(), o2.cpu(), sec


def _plain(case, tile):
    """v_gpu of the instance `tile` names: the launch without epilogue flags, once per instance."""
    if tile not in case.plain:
        rc, v, _, _ = _launch(case, tile, {}, {})
        assert rc == 0, f"plain launch at tile {tile:#x} refused ({rc})"
        case.plain[tile] = v
    return case.plain[tile]


class _Worst:
    """Worst figures per tile class of one row; recorded, then asserted together so that one run leaves every figure."""

    def __init__(self, name, prefix="conv_epilogue", ulp_bar="(a)"):
        self.name, self.fig, self.fail, self.prefix, self.ulp_bar = name, {}, [], prefix, ulp_bar

    def put(self, cls, **vals):
        f = self.fig.setdefault(cls, {})
        for k, v in vals.items():
            f[k] = max(f.get(k, 0.0), float(v))

    def close(self):
        for cls, f in sorted(self.fig.items()):
            record(f"{self.prefix}[{self.name}][{cls}]", **f)
            print(f"{self.prefix}[{self.name}][{cls}]: " + ", ".join(f"{k} {v:.3g}" for k, v in sorted(f.items())))
            for out in ("y", "second"):
                if f"{out}_gpu_ulp" in f and f[f"{out}_gpu_ulp"] > 4.0 * f[f"{out}_cpu_ulp"]:
                    self.fail.append(f"{self.ulp_bar} {cls} {out}: {f[out + '_gpu_ulp']:.2f} ulp > 4 x {f[out + '_cpu_ulp']:.2f} ulp of the float32 formula")
        assert not self.fail, f"{self.name}:\n  " + "\n  ".join(self.fail)


def _ulps(got, want64, scale64):
    assert torch.isfinite(got).all(), "non-finite result"
    return float(R.ulp_err(got, want64, scale64).max())


def _check_a(worst, cls, what, ep, sides, v_gpu, y, second):
    """(a): the epilogue on THIS instance's own accumulator."""
    f_y, f_2 = C.out_f32(v_gpu, ep, sides)
    w_y, w_2 = C.out64(v_gpu, ep, sides)
    s_y, s_2 = C.out_scale64(v_gpu.double(), v_gpu.double().abs(), ep, sides)
    if not C.has_expf(ep, sides):
        if not torch.equal(y, f_y):
            worst.fail.append(f"(a) {what}: y differs from the float32 restatement in {int((y != f_y).sum())} elements, worst {_ulps(y, f_y.double(), None):.2f} ulp")
    else:
        worst.put(cls, y_gpu_ulp=_ulps(y, w_y, s_y), y_cpu_ulp=_ulps(f_y, w_y, s_y))
    if second is None:
        return
    if ep.get("dual_silu"):                                         # the twin is silu of the STORED y, whatever path produced y
        w_t = R.silu64(y)
        worst.put(cls, second_gpu_ulp=_ulps(second, w_t, None), second_cpu_ulp=_ulps(R.silu_f32(y), w_t, None))
    elif ep.get("bwd") == "gate":
        worst.put(cls, second_gpu_ulp=_ulps(second, w_2, s_2), second_cpu_ulp=_ulps(f_2, w_2, s_2))
    elif not torch.equal(second, f_2):
        worst.fail.append(f"(a) {what}: d s differs from the float32 restatement, worst {_ulps(second, f_2.double(), None):.2f} ulp")


def _whole(case, ep, sides):
    """(b)'s references of one (case, epilogue): out64 on conv64, its scale, and e_seq of out_f32 on the one-chain sum."""
    want = C.out64(case.v64, ep, sides)
    scale = C.out_scale64(case.v64, case.vscale, ep, sides)
    seq = C.out_f32(case.vseq, ep, sides)
    e_seq = [None if w is None else C.rel_err(s_, w, sc) for w, s_, sc in zip(want, seq, scale)]
    return want, scale, e_seq


def _check_b(worst, cls, what, whole, y, second):
    want, scale, e_seq = whole
    for out, got, w, sc, es in zip(("y", "second"), (y, second), want, scale, e_seq):
        if w is None:
            continue
        e_hip = C.rel_err(got, w, sc)
        worst.put(cls, **{f"{out}_e_hip": e_hip, f"{out}_e_seq": es})
        if e_hip > max(4.0 * es, FLOOR_B):
            worst.fail.append(f"(b) {what} {out}: e_hip {e_hip:.3e} > max(4 x e_seq {es:.3e}, {FLOOR_B})")


SECTION = {4: 1, 2: 2, 1: 4}          # row-tile section of the operand stream a tile height reads (ops.sections_used)


@pytest.mark.parametrize("row", ROWS, ids=[r["name"] for r in ROWS])
def test_conv_epilogue(dev, row):
    """One epilogue on every tile of TILES at every geometry of the row, (a) and (b) as the module docstring says, guard bands and
    input clones.  Measured (profiles/r10_conv_epilogue_errors.json, conv_epilogue[<row>][<tile class>]): e.g. res+dual_silu on 4x2 y
    e_hip 2.2e-7 / e_seq 2.5e-7, twin 2.15 ulp against the formula's 1.85; shuffle2+dsilu_mul+res on 4x1 6.05 ulp = the formula's
    6.05, e_hip 3.0e-7 / e_seq 2.8e-7; GATE_BWD d s 3.79 ulp against 3.15."""
    ep, bwd = row["ep"], row["ep"].get("bwd")
    worst, runs, reroutes = _Worst(row["name"]), 0, 0
    for gname in row["geoms"]:
        results = {}                                                # tile -> (y, second) of this geometry
        for tile in TILES:
            case = _case(dev, row, gname, tile)
            sides = case.sides(row["sides"], bool(ep.get("shuffle2")))
            if bwd in ("gdn", "igdn"):
                sides = dict(sides, m=case.x)
            sides_dev = {k: t.to(dev) for k, t in sides.items()}
            clones = [(k, t, t.clone()) for k, t in list(sides_dev.items()) + [("x", case.xd)]]
            what = f"{gname} Cout={_cout(tile)} tile={tile:#x}"
            rc, y, second, sec = _launch_bwd(case, tile, bwd, sides_dev) if bwd else _launch(case, tile, ep, sides_dev)
            assert rc == 0, f"{row['name']} {what}: refused ({rc}) where the table expects a launch"
            assert sec == SECTION[(tile >> 4) & 15], f"{row['name']} {what}: read operand section {sec:#x}"
            results[tile] = (y, second)
            for k, t, c in clones:
                assert torch.equal(t, c), f"{row['name']} {what}: input {k} modified"
        for tile in TILES:
            verdict, eff = _plan(row, gname, tile)
            y, second = results[tile]
            what = f"{gname} Cout={_cout(tile)} tile={tile:#x}"
            if verdict == "reroute":
                reroutes += 1
                ey, e2 = results[eff]
                assert torch.equal(y, ey) and (second is None or torch.equal(second, e2)), \
                    f"{row['name']} {what}: the table says this runs as {eff:#x}, whose bits differ"
                continue
            runs += 1
            case = _case(dev, row, gname, tile)
            sides = case.sides(row["sides"], bool(ep.get("shuffle2")))
            if bwd in ("gdn", "igdn"):
                sides = dict(sides, m=case.x)
            cls = _tile_class(tile)
            _check_a(worst, cls, what, ep, sides, _plain(case, tile), y, second)
            key = (row["name"], gname, _cout(tile))
            if key not in _WHOLE:
                _WHOLE[key] = _whole(case, ep, sides)
            _check_b(worst, cls, what, _WHOLE[key], y, second)
        # a split that runs must differ from the unsplit instance somewhere (else the table's "run" rows prove nothing about it)
        if GEOMS[gname]["split"] is SPLIT64 and not bwd:
            assert not torch.equal(results[0x11][0], results[0x311][0]), f"{gname}: split 3 of the 32 x 32 tile returned the unsplit bits"
    worst.close()
    assert runs == row["runs"], f"{row['name']}: {runs} distinct instances ran, the table says {row['runs']}"
    assert runs + reroutes == len(TILES) * len(row["geoms"])


_WHOLE = {}


def test_pair_form_ran_where_the_table_says(dev):
    """pair_ok (conv_launch.hip) at pair5x14: the 0x442 launch is the pixel-pair instance, whose results are the 0x42 tile's bits by
    construction -- so the table's "run" there is checked the only way the outside can: both launch, agree bit for bit on every
    pair-form epilogue, and the pair form keeps 64-bit accesses inside a 14-wide row (guard bands, _launch)."""
    for row in ROWS:
        verdict, _ = _plan(row, "pair5x14", 0x442) if "pair5x14" in row["geoms"] else ("reroute", 0)
        if verdict != "run":
            continue
        case = _case(dev, row, "pair5x14", 0x442)
        sides = case.sides(row["sides"], bool(row["ep"].get("shuffle2")))
        sides_dev = {k: t.to(dev) for k, t in sides.items()}
        _, ya, ta, _ = _launch(case, 0x42, row["ep"], sides_dev)
        _, yb, tb, _ = _launch(case, 0x442, row["ep"], sides_dev)
        assert torch.equal(ya, yb) and (ta is None or torch.equal(ta, tb)), row["name"]


# ---- the small-launch kernel ----------------------------------------------------------------------------------------------------------------
T16_SUBSETS = [s for s in ([k for i, k in enumerate(("silu_out", "res", "dual_silu", "dsilu_mul")) if m >> i & 1] for m in range(16))
               if not ("silu_out" in s and "dual_silu" in s)]
T16_SHAPES = ((2, 64, 48, 5, 7), (2, 128, 32, 3, 3))        # 70 pixels: a ragged last 16-pixel tile; 18 pixels: a tile that straddles the images


@pytest.mark.parametrize("subset", T16_SUBSETS, ids=lambda s: "+".join(s) or "plain")
def test_small_launch_kernel_epilogue(dev, subset):
    """conv_t16_kernel (tile = 0 on shapes mcq_conv2d_small_launch takes) carries its own copy of the epilogue: every valid subset of
    T16_FLAGS, res_scale = 0.5, against (a) and (b); the operand section read (8) says the kernel is the one that ran.  Measured
    (conv_epilogue[t16:*]): four channel slices of 16 or 32 channels -- e_hip 0.7e-7 .. 1.5e-7 against e_seq 1.9e-7 .. 2.0e-7;
    silu_out 1.86 ulp against the formula's 1.68, * silu'(m) 7.24 = 7.24."""
    from mcquic_amd import _lib, ops
    assert len(T16_SUBSETS) == 12
    ep = dict({k: True for k in subset if k in ("silu_out", "dual_silu")}, **({"res_scale": 0.5} if "res" in subset else {}))
    names = tuple(k for k in subset if k in ("res", "dsilu_mul"))
    flags = sum({"silu_out": ops.CONV_SILU_OUT, "res": ops.CONV_RESIDUAL, "dual_silu": ops.CONV_DUAL_SILU, "dsilu_mul": ops.CONV_DSILU_MUL}[k] for k in subset)
    worst = _Worst("t16:" + ("+".join(subset) or "plain"))
    for n, cin, cout, h, w in T16_SHAPES:
        assert _lib.load().mcq_conv2d_small_launch(n, cin, h, w, cout, 3, 1, flags, 1) == 1
        gname = f"t16_{cin}_{cout}"
        GEOMS.setdefault(gname, dict(cin=cin, h=h, w=w, ks=3, stride=1, split=NO_SPLIT))
        key = (gname, cout, None, False, False, False)
        if key not in _CASES:
            _CASES[key] = _Case(dev, *key)
        case = _CASES[key]
        sides = case.sides(names, False)
        sides_dev = {k: t.to(dev) for k, t in sides.items()}
        clones = [(t, t.clone()) for t in list(sides_dev.values()) + [case.xd]]
        rc, y, second, sec = _launch(case, 0, ep, sides_dev)
        assert rc == 0 and sec == 8, f"{gname}: status {rc}, operand section {sec:#x}"
        assert all(torch.equal(t, c) for t, c in clones), "input modified"
        rc, v_gpu, _, sec = _launch(case, 0, {}, {})
        assert rc == 0 and sec == 8
        _check_a(worst, "16x16", gname, ep, sides, v_gpu, y, second)
        _check_b(worst, "16x16", gname, _whole(case, ep, sides), y, second)
    worst.close()


# ---- special values ------------------------------------------------------------------------------------------------------------------------
SPECIAL_ROWS = [r for r in ROWS if (C.has_expf(r["ep"], r["sides"]) or r["ep"].get("dual_silu")) and r["pro"] is None and not r.get("dgrad")]
SPECIAL_CASES = [(r, ks) for r in SPECIAL_ROWS for ks in (1, 3) if not (ks == 3 and r["ep"].get("bwd"))]          # (the backward pairs are 1x1 launches)
SPECIAL_TILES = (0, 0x42, 0x442, 0x41, 0x22, 0x21, 0x14, 0x12, 0x11)


@pytest.mark.parametrize("row,ks", SPECIAL_CASES, ids=[f"{r['name']}-k{ks}" for r, ks in SPECIAL_CASES])
def test_special_values_reach_the_epilogue(dev, row, ks):
    """Identity weights (1x1, and the same as a centre-tap 3x3), Cin = Cout = 40, zero bias: v is exactly the input, R.special_x --
    +-0, +-87, +-100 (expf(-x) overflows), the zero of silu' -- in v and in the silu' operand.  Every output finite and within (a)'s
    ulp bar; sigmoid in the gate, silu_out and the twin must not turn an overflowing expf into NaN.  Measured
    (conv_epilogue[special:*]): * silu'(m) 13.1 - 14.4 ulp, the formula's own figure to the digit; silu_out 1.78 against 1.27, the
    twin behind a residual 2.46 against 1.62, the gate 1.84 = 1.84."""
    from mcquic_amd import ops
    ep, bwd = row["ep"], row["ep"].get("bwd")
    c, h, w = 40, 5, 6
    shape = (2, c, h, w)
    x = R.special_x(2 * c * h * w, 5).view(shape).contiguous()
    wt = torch.zeros((c, c, ks, ks))
    wt[torch.arange(c), torch.arange(c), ks // 2, ks // 2] = 1.0
    pk = ops.PackedConv(wt.to(dev), torch.zeros(c).to(dev))
    case = _Case.__new__(_Case)
    case.xd, case.pk, case.stride, case.pro, case.x = x.to(dev), pk, 1, None, x
    oshape = (2, c // 4, 2 * h, 2 * w) if ep.get("shuffle2") else shape
    n_out = 2 * c * h * w
    sides = {k: (R.special_x(n_out, 6 + i).view(oshape).contiguous() if k == "dsilu_mul" else R.randn(oshape, 9 + i, 2.0 if k in ("gate_mul", "m") else 0.5))
             for i, k in enumerate(row["sides"])}
    sides_dev = {k: t.to(dev) for k, t in sides.items()}
    worst = _Worst(f"special:{row['name']}:k{ks}")
    for tile in SPECIAL_TILES:
        rc, v_gpu, _, _ = _launch(case, tile, {}, {})
        assert rc == 0 and torch.equal(v_gpu, x), f"tile {tile:#x}: an identity layer must return its input"
        rc, y, second, _ = _launch_bwd(case, tile, bwd, sides_dev) if bwd else _launch(case, tile, ep, sides_dev)
        assert rc == 0
        assert torch.isfinite(y).all() and (second is None or torch.isfinite(second).all()), f"tile {tile:#x}: non-finite output"
        _check_a(worst, "all", f"tile={tile:#x}", ep, sides, x, y, second)
    worst.close()


# ---- what the launcher refuses -----------------------------------------------------------------------------------------------------------
def test_refusals(dev):
    """Combinations no instance implements come back as MCQ_EINVAL (-1), with the output untouched: the SiLU prologue on 1x1, the
    squaring prologue on 3x3, SiLU out together with the twin, the PixelShuffle store with a Cout that is no multiple of 4 or with
    an epilogue other than * silu'(.) / + res, and the backward pairs on 3x3 layers."""
    from mcquic_amd import _lib, ops
    row3, row1 = dict(ROWS[0], pro=None), dict(ROWS[0], pro=None)
    c3, c1 = _case(dev, row3, "odd7x9", 0x11), _case(dev, row1, "k1_7x9", 0x11)
    side = lambda case, names, shuffle=False: {k: t.to(dev) for k, t in case.sides(names, shuffle).items()}          # noqa: E731
    refused = [
        ("silu_in on 1x1", c1, dict(silu_in=True), {}),
        ("square_in on 3x3", c3, dict(square_in=True), {}),
        ("silu_out + dual_silu", c3, dict(silu_out=True, dual_silu=True), {}),
        ("shuffle2 + silu_out", c3, dict(shuffle2=True, silu_out=True), {}),
        ("shuffle2 + mul", c3, dict(shuffle2=True), side(c3, ("mul",), True)),
        ("silu_in + square_in", c3, dict(silu_in=True, square_in=True), {}),
    ]
    for what, case, kw, sd in refused:
        for tile in (0, 0x11, 0x22, 0x242):
            keep, case.pro = case.pro, None
            try:
                rc, _, _, _ = _launch(case, tile, kw, sd)
            finally:
                case.pro = keep
            assert rc == _lib.MCQ_EINVAL, f"{what} tile={tile:#x}: status {rc}"
    pk = ops.PackedConv(R.randn((42, 20, 3, 3), 1, 0.1).to(dev), None)
    with pytest.raises(RuntimeError, match="MCQ_EINVAL"):
        ops.conv2d(c3.xd, pk, 1, shuffle2=True, tile=0x11)          # Cout = 42
    d = _lib.ConvDesc(c3.xd.data_ptr(), c3.pk.wp.data_ptr(), None, c3.xd.data_ptr(), c3.xd.data_ptr(), c3.xd.data_ptr(), c3.xd.data_ptr(), None,
                      2, 20, 7, 9, 40, 3, 1, ops.CONV_GATE_BWD, 1.0, 0x11)
    keep = c3.xd.clone()
    assert _lib.load().mcq_conv2d_f32(ctypes.byref(d), None) == _lib.MCQ_EINVAL and torch.equal(c3.xd, keep)
