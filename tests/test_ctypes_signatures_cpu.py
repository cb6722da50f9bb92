"""The signature tables of the three ctypes views (binding.py, dv.py, yuv.py) against the prototypes of include/*.h: the
same functions, the same number of arguments, and every argument and return of the same kind (pointer, 32-bit or 64-bit
integer, float or double, void).  Reads the headers and the tables only: no library is opened, so none has to be built."""
import ctypes as C
import importlib
import os
import re

import pytest

from pkg import ROOT

# (module, header, prefix of the entry points, functions the header declares at the commit that added this test)
VIEWS = [("binding", "mi_rtjpeg.h", "mi_rtj_", 53), ("dv", "mi_dv.h", "mi_dv_", 39), ("yuv", "mi_yuv.h", "mi_yuv_", 15)]
INT32 = {"int", "unsigned", "int32_t", "uint32_t"}
INT64 = {"size_t", "int64_t", "uint64_t"}


def c_kind(decl):
    """the kind of a C return type or parameter (its name, if it has one, still on it)"""
    if "*" in decl or "[" in decl:
        return "pointer"
    words = [w for w in decl.split() if w != "const"]
    if words[0] == "unsigned" and words[1:2] in (["int"], ["long"]):
        del words[0]
    if words[:2] == ["long", "long"]:
        return "int", 8
    if words[0] in ("float", "double"):
        return "float", C.sizeof(C.c_double if words[0] == "double" else C.c_float)
    if words[0] in INT32 or words[0] in INT64:
        return "int", 4 if words[0] in INT32 else 8
    assert words[0] == "void" and len(words) == 1, decl
    return "void"


def ctypes_kind(t):
    if t is None:
        return "void"
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, (C._Pointer, C.Array)):
        return "pointer"
    if t in (C.c_float, C.c_double):
        return "float", C.sizeof(t)
    assert issubclass(t, C._SimpleCData) and t._type_ in "iIlLqQ", t
    return "int", C.sizeof(t)


def prototypes(header, prefix):
    """{name: (return kind, [argument kinds])} of every `ret name(args);` of the header whose name has the prefix"""
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", " ", txt)
    txt = re.sub(r"^[ \t]*#[^\n]*", " ", txt, flags=re.M)
    found = {}
    for stmt in txt.split(";"):
        m = re.search(r"([\w\s*]+?)\b(" + prefix + r"\w+)\s*\(([^()]*)\)\s*$", stmt)
        if not m:
            continue
        ret, name, args = m.group(1).strip(), m.group(2), m.group(3).strip()
        assert name not in found, name
        found[name] = (c_kind(ret), [] if args == "void" else [c_kind(a.strip()) for a in args.split(",")])
    return found


@pytest.mark.parametrize("module,header,prefix,count", VIEWS, ids=[v[0] for v in VIEWS])
def test_signature_table_matches_the_header(module, header, prefix, count):
    view = importlib.import_module("gmerlin-avdecoder_amd." + module)
    declared = prototypes(header, prefix)
    assert len(declared) >= count  # (an empty or a lame parse must not pass)
    assert set(view.SIGNATURES) == set(declared) == set(view.EXPORTS)
    assert len(view.EXPORTS) == len(declared)
    for name, (ret, args) in declared.items():
        restype, argtypes = view.SIGNATURES[name]
        assert len(argtypes) == len(args), name
        assert ctypes_kind(restype) == ret, name
        assert [ctypes_kind(t) for t in argtypes] == args, name

