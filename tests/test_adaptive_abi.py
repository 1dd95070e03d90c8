"""CPU: the adaptive-sampling surface of the C-ABI (ABI version 10): the header, the ctypes mirror and the library
agree on the new entry points, and the three new structs have gcc's layout."""
import ctypes as C
import re
import subprocess
from pathlib import Path

from computational_ray_tracer_amd import capi

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ["rt_adaptive_begin", "rt_adaptive_step", "rt_adaptive_read", "rt_adaptive_end", "rt_render_adaptive",
               "rt_debug_adaptive_select"]
NEW_STRUCTS = ["rt_moment", "rt_adaptive_desc", "rt_adaptive_info"]


def test_abi_version_is_10():
    text = (ROOT / "include" / "rtmi355x.h").read_text()
    assert re.search(r"^#define RT_ABI_VERSION 10$", text, re.M)
    assert capi.ABI_VERSION == 10
    assert capi.load_library().rt_abi_version() == 10


def test_header_ctypes_and_library_agree_on_the_new_symbols():
    text = (ROOT / "include" / "rtmi355x.h").read_text()
    declared = set(re.findall(r"^\s*int\s+(rt_\w+)\s*\(", text, re.M))
    lib = capi.load_library()
    for s in NEW_SYMBOLS:
        assert s in declared, s
        assert s in capi.EXPORTS, s
        f = getattr(lib, s)              # AttributeError: the library does not export it
        assert f.restype is C.c_int and f.argtypes, s   # load_library gave it a signature
    # the signatures' struct arguments are the mirrors below
    assert lib.rt_adaptive_begin.argtypes[1]._type_ is capi.rt_adaptive_desc
    assert lib.rt_adaptive_step.argtypes[1]._type_ is capi.rt_adaptive_info
    assert lib.rt_adaptive_read.argtypes[2]._type_ is capi.rt_moment
    assert lib.rt_render_adaptive.argtypes[3]._type_ is capi.rt_moment


def test_new_struct_sizes_match_header_layout(tmp_path):
    """Compile the header with gcc and compare the new structs' sizes and field offsets with the ctypes mirrors."""
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "rtmi355x.h"', "int main(void) {"]
    for s in NEW_STRUCTS:
        lines.append(f'printf("{s} %zu\\n", sizeof({s}));')
        for f, _ in getattr(capi, s)._fields_:
            lines.append(f'printf("{s}.{f} %zu\\n", offsetof({s}, {f}));')
    lines += ["return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    got = dict(l.split() for l in out.split("\n") if l)
    for s in NEW_STRUCTS:
        st = getattr(capi, s)
        assert int(got[s]) == C.sizeof(st), s
        for f, _ in st._fields_:
            assert int(got[f"{s}.{f}"]) == getattr(st, f).offset, f"{s}.{f}"
    assert C.sizeof(capi.rt_moment) == 8 and C.sizeof(capi.rt_adaptive_desc) == 32
    assert C.sizeof(capi.rt_adaptive_info) == 24 and capi.rt_adaptive_info.samples.offset == 16


def test_null_context_is_an_argument_error():
    """Host-only behaviour of the new entries (no device needed): a NULL context is RT_E_ARG, never a crash."""
    lib = capi.load_library()
    d = capi.rt_adaptive_desc()
    assert lib.rt_adaptive_begin(None, C.byref(d)) == capi.RT_E_ARG
    assert lib.rt_adaptive_step(None, None) == capi.RT_E_ARG
    assert lib.rt_adaptive_read(None, None, None, None, None, None) == capi.RT_E_ARG
    assert lib.rt_adaptive_end(None) == capi.RT_E_ARG
    assert lib.rt_render_adaptive(None, C.byref(d), None, None, None) == capi.RT_E_ARG
    assert lib.rt_debug_adaptive_select(None, C.byref(d), None, None, None, None, None) == capi.RT_E_ARG
