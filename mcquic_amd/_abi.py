"""Reads include/mcquic_hip.h into what ctypes needs: constants, structs and prototypes.

The header is the only statement of the C-ABI.  Plain `re` over a regular C subset; whatever falls outside that subset
raises ImportError naming the declaration, so a prototype is never guessed.
"""
from __future__ import annotations

import re
from ctypes import POINTER, Structure, c_char_p, c_double, c_float, c_int32, c_int64, c_size_t, c_uint32, c_void_p

_SCALARS = {"int32_t": c_int32, "int": c_int32, "uint32_t": c_uint32, "int64_t": c_int64, "size_t": c_size_t,
            "float": c_float, "double": c_double}
_POINTEES = set(_SCALARS) | {"void", "char", "uint8_t", "uint64_t"}
_LITERAL = re.compile(r"(-?)(0[xX][0-9a-fA-F]+|[0-9]+)[uU]?[lL]{0,2}")


def _refuse(decl: str, why: str):
    raise ImportError(f"mcquic_hip.h: {why} in `{' '.join(decl.split())}`")


def _ctype(spec: str, decl: str, structs: dict, returned: bool = False):
    """The ctypes type of a C type written without its name (`const float* const*`); `structs`: the ones POINTER may name."""
    words = spec.replace("*", " * ").split()
    base = [w for w in words if w not in ("const", "*")]
    if len(base) != 1:
        _refuse(decl, f"cannot split `{spec.strip()}` into a type and a name")
    base, stars = base[0], words.count("*")
    if stars == 0:
        if base == "void" and returned:
            return None
        if base not in _SCALARS:
            _refuse(decl, f"unknown type `{base}`")
        return _SCALARS[base]
    if base in structs:
        return POINTER(structs[base]) if stars == 1 else c_void_p
    if base not in _POINTEES:
        _refuse(decl, f"unknown type `{base}`")
    return c_char_p if returned and base == "char" and stars == 1 else c_void_p


def _constants(text: str) -> dict:
    out = {}
    for line, name, value in re.findall(r"^([ \t]*#[ \t]*define[ \t]+(MCQ_\w+)[ \t]+(\S.*))$", text, re.M):
        value = "".join(value.split())
        m = _LITERAL.fullmatch(value)
        if m:
            out[name] = int(m.group(1) + m.group(2), 16 if m.group(2)[:2] in ("0x", "0X") else 10)
        elif re.fullmatch(r"\(\w+(\|\w+)*\)", value) and all(n in out for n in value[1:-1].split("|")):
            out[name] = 0
            for n in value[1:-1].split("|"):        # (MCQ_A | MCQ_B): flags defined above
                out[name] |= out[n]
        else:
            _refuse(line, "neither an integer literal nor an OR of earlier constants")
    return out


def _struct(name: str, body: str) -> type:
    fields = []
    for member in filter(None, (m.strip() for m in body.split(";"))):
        m = re.fullmatch(r"(.*?[\s*])(\w+(?:\s*,\s*\w+)*)", member, re.S)
        if not m:
            _refuse(member, f"cannot split this member of struct {name}")
        ctype = _ctype(m.group(1), f"struct {name} {{ {member}; }}", {})       # every pointer a c_void_p, struct pointers too
        fields += [(n.strip(), ctype) for n in m.group(2).split(",")]
    python_name = "".join(w.capitalize() for w in name.split("_")[1:])          # mcq_conv_desc -> ConvDesc
    return type(python_name, (Structure,), {"_fields_": fields, "__doc__": f"struct {name} (include/mcquic_hip.h)."})


def read(text: str):
    """(constants, structs, symbols) of a header's text: {MCQ_X: int}, {struct name: ctypes.Structure}, {mcq_f: (restype, argtypes)}."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#[ \t]*ifdef[ \t]+__cplusplus.*?^[ \t]*#[ \t]*endif.*?$", "", text, flags=re.S | re.M)   # extern "C" { ... }
    constants = _constants(text)
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    structs = {}

    def take_struct(m):
        if m.group(1) != m.group(3) or m.group(1) in structs:
            _refuse(m.group(0), "typedef struct NAME { ... } NAME; expected, once")
        structs[m.group(1)] = _struct(m.group(1), m.group(2))
        return ""
    text = re.sub(r"\btypedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;", take_struct, text)
    symbols = {}
    for decl in filter(None, (d.strip() for d in text.split(";"))):
        m = re.fullmatch(r"([\w\s*]+?)\b(mcq_\w+)\s*\(([^()]*)\)", decl)
        if not m or m.group(2) in symbols:
            _refuse(decl, "not a single `type mcq_name(arguments)` declaration")
        args = [a.strip() for a in m.group(3).split(",")]
        if args in ([""], ["void"]):
            args = []
        argtypes = []
        for a in args:
            named = re.fullmatch(r"(.*[\s*])\w+", a, re.S)
            if not named:
                _refuse(decl, f"cannot split argument `{a}`")
            argtypes.append(_ctype(named.group(1), decl, structs))
        symbols[m.group(2)] = (_ctype(m.group(1), decl, structs, returned=True), argtypes)
    return constants, structs, symbols
