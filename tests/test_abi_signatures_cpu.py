"""Every prototype of include/mhla_hip.h against _lib.SIGNATURES: return type and every parameter type, both ways (no built library, no GPU).

The ctypes lists are positional and written by hand; tools/record_launches.py and every caller go through them, so a wrong entry
corrupts a call without a diagnostic.  The header is the authority."""
import os
import re
from ctypes import c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_uint, c_void_p

from mhla_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VALUES = {"int": c_int, "int32_t": c_int32, "int64_t": c_int64, "float": c_float, "size_t": c_size_t, "unsigned": c_uint,
          "mhla_view": _lib.View, "mhla_mview": _lib.View, "void": None}


def ctype_of(decl):
    """The ctypes type of one C parameter or return type; a parameter's name, if it has one, is dropped."""
    decl = decl.strip()
    if "*" in decl:   # a pointer: a string where it points to char (the messages out, the report buffers in), else opaque
        return c_char_p if re.fullmatch(r"(const\s+)?char\s*\*\s*\w*", decl) else c_void_p
    words = [w for w in decl.split() if w != "const"]
    assert words and words[0] in VALUES, f"type of `{decl}` is not in the table"
    return VALUES[words[0]]


def prototypes(header):
    """name -> (restype, [argtypes]) of every function the header declares"""
    text = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#[^\n]*", " ", text, flags=re.M)
    text = re.sub(r"typedef\s+struct\s*\{.*?\}\s*\w+\s*;", " ", text, flags=re.S)
    text = re.sub(r"\benum\s*\w*\s*\{.*?\}\s*;", " ", text, flags=re.S)
    text = text.replace('extern "C" {', " ")
    out = {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split()).strip("} ")
        if not stmt:
            continue
        m = re.fullmatch(r"(.+?[\s*])(mhla_\w+)\s*\((.*)\)", stmt)
        assert m, f"not a prototype: `{stmt}`"
        ret, name, params = m.groups()
        assert name not in out, f"{name} is declared twice"
        out[name] = (ctype_of(ret), [] if params.strip() == "void" else [ctype_of(p) for p in params.split(",")])
    return out


def test_every_prototype_matches_its_ctypes_signature():
    protos = prototypes(open(os.path.join(ROOT, "include", "mhla_hip.h")).read())
    assert len(protos) >= 93, f"only {len(protos)} prototypes parsed"
    only_header, only_python = sorted(set(protos) - set(_lib.SIGNATURES)), sorted(set(_lib.SIGNATURES) - set(protos))
    assert not only_header, f"declared in include/mhla_hip.h, missing from _lib.SIGNATURES: {only_header}"
    assert not only_python, f"in _lib.SIGNATURES, not declared in include/mhla_hip.h: {only_python}"
    bad = []
    for name, (res, args) in protos.items():
        sres, sargs = _lib.SIGNATURES[name]
        if sres is not res:
            bad.append(f"{name}: returns {res}, SIGNATURES says {sres}")
        if len(sargs) != len(args):
            bad.append(f"{name}: {len(args)} parameters, SIGNATURES has {len(sargs)}")
            continue
        bad += [f"{name}: parameter {i} is {a}, SIGNATURES says {s}" for i, (a, s) in enumerate(zip(args, sargs)) if a is not s]
    assert not bad, "\n".join(bad)
