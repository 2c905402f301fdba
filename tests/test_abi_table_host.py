"""CPU-only tests of the Python side of the C ABI: the prototype table of mygauhuman_amd/_lib.py and the ctypes struct mirrors
against include/gsr.h (every function, every parameter, every field; sizes and offsets from the host C compiler), and the
call() helper's contract."""
import ctypes as C
import os
import re
import subprocess

import pytest

from mygauhuman_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gsr.h")

STRUCT_RE = re.compile(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*\1\s*;", re.S)
BY_VALUE = {"int": "int", "unsigned": "unsigned", "float": "float", "double": "double", "size_t": "size_t",
            "long long": "long long", "gsr_stream_t": "pointer", "gsr_alloc_fn": "pointer"}
CTYPES_CLASS = {C.c_int: "int", C.c_uint: "unsigned", C.c_float: "float", C.c_double: "double", C.c_size_t: "size_t",
                C.c_longlong: "long long", C.c_void_p: "pointer", C.c_char_p: "pointer"}
RETURNS = {"int": C.c_int, "size_t": C.c_size_t, "const char *": C.c_char_p, "void": None}
MIRRORS = {"gsr_phase1_loss": _lib.Phase1LossStruct, "gsr_pbr_texture": _lib.PbrTexture, "gsr_pbr_shade": _lib.PbrShade,
           "gsr_bake_scene": _lib.BakeScene, "gsr_pbr_loss": _lib.PbrLoss, "gsr_ssim_crop": _lib.SsimCrop,
           "gsr_adam_array": _lib.AdamArray, "gsr_adam_group": _lib.AdamGroup, "gsr_adam_stats": _lib.AdamStats,
           "gsr_eval_slot": _lib.EvalSlot, "gsr_eval_view": _lib.EvalView}


def _header_text():
    """gsr.h without comments and preprocessor lines."""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    return "\n".join(line for line in text.splitlines() if not line.lstrip().startswith("#"))


def _header_structs():
    """{struct name: [field names in order]}"""
    out = {}
    for name, body in STRUCT_RE.findall(_header_text()):
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            for part in decl.split(","):
                fields.append(re.search(r"(\w+)\s*(\[[^\]]*\]\s*)*$", part.strip()).group(1))
        out[name] = fields
    return out


def _param_class(param):
    if "*" in param:
        return "pointer"
    words = [w for w in param.split() if w != "const"]
    return BY_VALUE[" ".join(words[:-1])]  # the last word is the parameter's name; an unknown type is a KeyError


def _header_functions():
    """{function name: (return type text, [parameter classes], last parameter is the gsr_stream_t)}"""
    text = STRUCT_RE.sub(" ", _header_text())
    text = re.sub(r"\benum\s*\{.*?\}\s*;", " ", text, flags=re.S)
    text = re.sub(r"\btypedef\b[^;]*;", " ", text)
    text = text.replace('extern "C" {', " ")
    out = {}
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split())
        if stmt in ("", "}"):
            continue
        m = re.fullmatch(r"(.+?)\b(gsr_\w+) ?\((.*)\)", stmt)
        assert m, f"cannot parse the declaration: {stmt}"
        ret, name, params = m.group(1).strip(), m.group(2), m.group(3).strip()
        params = [] if params == "void" else [p.strip() for p in params.split(",")]
        streamed = bool(params) and re.fullmatch(r"gsr_stream_t \w+", params[-1]) is not None
        assert name not in out, f"{name} is declared twice"
        out[name] = (ret, [_param_class(p) for p in params], streamed)
    return out


def _table_class(t):
    if t in CTYPES_CLASS:
        return CTYPES_CLASS[t]
    if isinstance(t, type) and issubclass(t, (C._Pointer, C._CFuncPtr)):
        return "pointer"
    return repr(t)


def test_table_matches_the_header():
    declared = _header_functions()
    assert len(declared) >= 100  # the parser found the declarations
    assert sorted(declared) == sorted(_lib.TABLE) == sorted(_lib.SYMBOLS)
    bad = []
    for name, (ret, params, streamed) in sorted(declared.items()):
        restype, argtypes, flag = _lib.TABLE[name]
        fn = getattr(_lib.lib, name)
        if ret not in RETURNS:
            bad.append(f"{name}: the header returns {ret!r}, which is none of {sorted(RETURNS)}")
        elif restype is not RETURNS[ret] or fn.restype is not RETURNS[ret]:
            bad.append(f"{name} returns: header {ret}, table {restype}, bound {fn.restype}")
        if flag is not streamed:
            bad.append(f"{name} trailing stream: header {streamed}, table {flag}")
        bound = list(fn.argtypes)   # what _load() gave the CDLL: the table's parameters and, when flagged, the stream
        if bound != list(argtypes) + [C.c_void_p] * bool(flag):
            bad.append(f"{name}: bound argtypes are not the table's")
        if len(bound) != len(params):
            bad.append(f"{name} parameter count: header {len(params)}, table {len(bound)}")
            continue
        for i, (want, t) in enumerate(zip(params, bound)):
            if _table_class(t) != want:
                bad.append(f"{name} parameter {i}: header {want}, table {_table_class(t)}")
    assert not bad, "\n".join(bad)


def test_struct_mirrors_match_the_header(tmp_path):
    structs = _header_structs()
    assert sorted(structs) == sorted(MIRRORS)
    mirrored = {v for v in vars(_lib).values() if isinstance(v, type) and issubclass(v, C.Structure) and v is not C.Structure}
    assert mirrored == set(MIRRORS.values())
    for name, fields in structs.items():
        assert [f for f, _ in MIRRORS[name]._fields_] == fields, name
    # sizes and offsets as the host C compiler lays the structs out
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "gsr.h"', 'int main(void) {']
    for name, fields in structs.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        lines += [f'  printf("{name}.{f} %zu\\n", offsetof({name}, {f}));' for f in fields]
    lines += ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = dict(line.split() for line in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    want = {}
    for name, fields in structs.items():
        want[name] = str(C.sizeof(MIRRORS[name]))
        want.update({f"{name}.{f}": str(getattr(MIRRORS[name], f).offset) for f in fields})
    assert got == want


def test_call_reports_the_status_under_the_function_name():
    with pytest.raises(_lib.GsrError, match=r"gsr_mark_visible failed \(-1\)"):
        _lib.call("gsr_mark_visible", None, -1, None, None, None, None, stream=0)


def test_call_refuses_a_function_without_a_stream():
    with pytest.raises(TypeError, match="gsr_sort_workspace_bytes"):
        _lib.call("gsr_sort_workspace_bytes", None, 1000)


def test_call_refuses_an_unknown_name():
    with pytest.raises(AttributeError, match="gsr_nope"):
        _lib.call("gsr_nope", None)
