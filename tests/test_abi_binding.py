"""CPU: the ctypes binding mcquic_amd/_lib.py derives from include/mcquic_hip.h -- the reader on small synthetic headers, its
refusals, the struct layouts against the host C compiler, and hand-written pins of prototypes the reader cannot vouch for itself.
All from the header alone, except the stale-library refusal, which loads the built library (like tests/test_host_abi.py)."""
import ctypes
import os
import re
import shutil
import subprocess
from ctypes import POINTER, c_char_p, c_double, c_float, c_int32, c_int64, c_size_t, c_uint32, c_void_p

import pytest

from mcquic_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mcquic_hip.h")

SNIPPET = """
/* a header in small; mcq_not_declared(int x) inside a comment is no declaration */
#define MCQ_ABI_VERSION   7
#define MCQ_HEX    0x1F   /* trailing comment */
#define MCQ_NEG   -3
#define MCQ_U      0x200u /* a comment that runs
                           * over two lines */
#define MCQ_LL     0x40000000LL
#define MCQ_BOTH   (MCQ_HEX | MCQ_U)
typedef struct mcq_conv_desc {
    const float* x;        /* [N, Cin, H, W] */
    float*       y;
    int32_t N, Cin, H;
    uint32_t flags;
    double a, b;
    float   scale;
} mcq_conv_desc;
size_t mcq_bytes(int32_t n, int64_t m);
void mcq_trace(int32_t on);
const char* mcq_name(void);
int32_t mcq_none();
int mcq_run(const mcq_conv_desc* d, void* stream);
int mcq_many(const mcq_conv_desc* const* ds, float* const* out /* [n] device pointers */, const void* table, uint32_t id,
             const uint8_t* mask /* or NULL */, const uint64_t* rng, float bound, double rate,
             void* stream);
"""


def test_reader_on_a_synthetic_header():
    constants, structs, symbols = _abi.read(SNIPPET)
    assert constants == {"MCQ_ABI_VERSION": 7, "MCQ_HEX": 31, "MCQ_NEG": -3, "MCQ_U": 512, "MCQ_LL": 1 << 30, "MCQ_BOTH": 543}
    assert all(type(v) is int for v in constants.values())
    assert list(structs) == ["mcq_conv_desc"]
    desc = structs["mcq_conv_desc"]
    assert issubclass(desc, ctypes.Structure) and desc.__name__ == "ConvDesc"
    assert desc._fields_ == [("x", c_void_p), ("y", c_void_p), ("N", c_int32), ("Cin", c_int32), ("H", c_int32), ("flags", c_uint32),
                             ("a", c_double), ("b", c_double), ("scale", c_float)]
    assert symbols == {
        "mcq_bytes": (c_size_t, [c_int32, c_int64]),
        "mcq_trace": (None, [c_int32]),
        "mcq_name": (c_char_p, []),                                 # (void)
        "mcq_none": (c_int32, []),                                  # ()
        "mcq_run": (c_int32, [POINTER(desc), c_void_p]),            # const mcq_conv_desc*
        # a pointer to struct pointers, float* const*, a comment inside the list, three lines
        "mcq_many": (c_int32, [c_void_p, c_void_p, c_void_p, c_uint32, c_void_p, c_void_p, c_float, c_double, c_void_p]),
    }


@pytest.mark.parametrize("text, named", [
    ("int mcq_f(long double x, void* stream);", "mcq_f"),                                       # a scalar type the table does not hold
    ("int mcq_f(float out[3]);", "mcq_f"),                                                      # an argument that does not split
    ("int mcq_f(int32_t);", "mcq_f"),                                                           # ... nor does one without a name
    ("int mcq_f(int32_t n) int mcq_g(void);", "mcq_g"),                                         # two declarations run together
    ("int mcq_f(void (*callback)(int), void* stream);", "mcq_f"),
    ("mcq_thing* mcq_f(void);", "mcq_f"),                                                       # a pointee nobody declared
    ("typedef struct mcq_a { int32_t n; } mcq_a;\ntypedef struct mcq_b { mcq_a inner; float x; } mcq_b;", "mcq_a inner"),
    ("typedef struct mcq_a { int32_t n; } mcq_a;\nint mcq_f(mcq_a by_value);", "mcq_f"),
    ("typedef struct mcq_a { uint32_t flag : 3; uint32_t rest : 29; } mcq_a;", "flag : 3"),     # a bit-field
    ("typedef struct mcq_a { float taps[11]; } mcq_a;", "taps[11]"),
    ("typedef struct mcq_a { int32_t n; } mcq_other;", "mcq_other"),
    ("#define MCQ_SHIFTED (1 << 4)", "MCQ_SHIFTED"),
    ("#define MCQ_A 1\n#define MCQ_MASK (MCQ_A | MCQ_LATER)\n#define MCQ_LATER 2", "MCQ_MASK"),
])
def test_reader_refuses_what_it_cannot_map(text, named):
    with pytest.raises(ImportError) as e:
        _abi.read(text)
    assert named in str(e.value) and "mcquic_hip.h" in str(e.value)


def test_struct_layouts_match_the_host_compiler(tmp_path):
    """sizeof and every offsetof of each struct of the real header, from a C program built here, against ctypes' layout."""
    cc = shutil.which("cc")
    if cc is None:
        pytest.skip("no host C compiler (cc)")
    assert set(_lib.STRUCTS) >= {"mcq_conv_desc", "mcq_lr_schedule"}
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "mcquic_hip.h"', "int main(void) {"]
    for cname, struct in _lib.STRUCTS.items():
        lines.append(f'    printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        lines += [f'    printf("{cname} {field} %zu\\n", offsetof({cname}, {field}));' for field, _ in struct._fields_]
    lines += ["    return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    compiled = [tuple(line.split()) for line in out.splitlines()]
    derived = []
    for cname, struct in _lib.STRUCTS.items():
        derived.append((cname, "sizeof", str(ctypes.sizeof(struct))))
        derived += [(cname, field, str(getattr(struct, field).offset)) for field, _ in struct._fields_]
    assert compiled == derived and len(derived) == 2 + 20 + 11


def test_public_names_of_the_binding():
    assert _lib.ConvDesc is _lib.STRUCTS["mcq_conv_desc"] and _lib.LrSchedule is _lib.STRUCTS["mcq_lr_schedule"]
    assert [n for n, _ in _lib.ConvDesc._fields_] == ["x", "w_packed", "bias", "y", "y_silu", "res", "mul", "gate_id", "N", "Cin", "H", "W",
                                                      "Cout", "ksize", "stride", "flags", "res_scale", "tile", "post_w", "post_bias"]
    assert [t for _, t in _lib.ConvDesc._fields_] == [c_void_p] * 8 + [c_int32] * 7 + [c_uint32, c_float, c_int32, c_void_p, c_void_p]
    assert _lib.LrSchedule._fields_ == [("kind", c_int32), ("mode", c_int32), ("ngroups", c_int32), ("nmilestones", c_int32),
                                        ("milestones", c_void_p), ("gamma", c_double), ("first_milestone", c_double),
                                        ("total_size", c_double), ("step_ratio", c_double), ("warmup_steps", c_double),
                                        ("cycle_mult", c_double)]
    assert (_lib.MCQ_OK, _lib.MCQ_EINVAL, _lib.MCQ_ELAUNCH, _lib.MCQ_ETOOLARGE) == (0, -1, -2, -3)
    assert (_lib.CONV_SILU_IN, _lib.CONV_DUAL_SILU, _lib.CONV_WINOGRAD2D16, _lib.CONV_POST_GATE) == (0x1, 0x100, 0x2000, 0x100000)
    assert _lib.CONV_POST_MASK == 0x1C0000
    assert (_lib.LR_MAX_GROUPS, _lib.LR_STATE_WORDS, _lib.LR_COSINE, _lib.LR_EXP_RANGE) == (64, 8, 3, 2)
    assert _lib.ABI_VERSION == _lib.MCQ_ABI_VERSION == _lib.CONSTANTS["MCQ_ABI_VERSION"]
    from mcquic_amd import ops
    assert (ops.REASSIGN_STATE_WORDS, ops.REASSIGN_STREAM, ops.AUG_COLUMNS) == (7, 3, 16)
    assert (ops.AUG_TOP, ops.AUG_GAMMA_MODE, ops.AUG_OUTPUT, ops.AUG_GAMMA_IDENTITY, ops.AUG_OUT_RAW) == (0, 4, 12, 3, 2)


def test_a_library_of_another_abi_version_is_refused(monkeypatch):
    built = int(_lib.load().mcq_abi_version())
    monkeypatch.setattr(_lib, "_lib", None)                        # as in a process that has not loaded it yet
    monkeypatch.setattr(_lib, "ABI_VERSION", built + 1)            # a header one version ahead of the library
    with pytest.raises(ImportError, match=rf"was built for ABI version {built}, this binding needs {built + 1}: rebuild with"):
        _lib.load()


def test_prototypes_pinned_by_hand():
    """Written out here, not derived: a reader that went wrong cannot agree with these by construction."""
    V, I, L, D = c_void_p, c_int32, c_int64, c_double
    pins = {
        "mcq_packed_conv_weight_floats": (c_size_t, [I, I, I]),
        "mcq_conv2d_f32": (I, [POINTER(_lib.ConvDesc), V]),
        "mcq_conv_section_trace": (None, [I]),
        "mcq_version": (c_char_p, []),
        "mcq_lr_schedule_step_skip": (I, [POINTER(_lib.LrSchedule), V, V, V, V, V]),
        "mcq_freq_ema_update_skip_f32": (I, [V, V, V, I, V, D, V, V]),
        "mcq_rans_encode_with_indexes": (L, [V, V, L, V, V, V, V, V, I, V, L]),
        "mcq_lamb_step_skip_f32": (I, [V, I, V, V, V, V, I, V, I, V, V, D, D, D, D, D, I, I, I, I, D, V, V, V, V, V, V]),
    }
    for name, pin in pins.items():
        assert _lib.SYMBOLS[name] == pin, name


def test_argument_counts_from_a_separate_regex():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    counted = {}
    for name, args in re.findall(r"\b(mcq_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        counted[name] = 0 if args.strip() in ("", "void") else args.count(",") + 1
    assert len(counted) == len(_lib.SYMBOLS) >= 157
    assert {name: len(argtypes) for name, (_, argtypes) in _lib.SYMBOLS.items()} == counted
