"""CPU: the temporal stage's surface of the C-ABI: the header, the ctypes mirror and the library agree
on the new entry points, the three structs have gcc's layout, the ABI version stays 10, and every new entry runs inside
the exception firewall."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

from computational_ray_tracer_amd import capi

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ["rt_render_features_pos", "rt_temporal_accumulate", "rt_temporal_begin", "rt_temporal_frame",
               "rt_temporal_reset", "rt_temporal_end"]
NEW_STRUCTS = ["rt_position", "rt_temporal_desc", "rt_temporal_info"]


def null_calls(lib):
    """Every new entry with a NULL context (no device needed)."""
    d, ad = capi.rt_temporal_desc(), capi.rt_adaptive_desc()
    return {
        "rt_render_features_pos": lambda: lib.rt_render_features_pos(None, 0, 1, None, None),
        "rt_temporal_accumulate": lambda: lib.rt_temporal_accumulate(None, C.byref(d), 1, 1, *([None] * 12)),
        "rt_temporal_begin": lambda: lib.rt_temporal_begin(None, C.byref(d)),
        "rt_temporal_frame": lambda: lib.rt_temporal_frame(None, C.byref(ad), None, None, None, None),
        "rt_temporal_reset": lambda: lib.rt_temporal_reset(None),
        "rt_temporal_end": lambda: lib.rt_temporal_end(None),
    }


def test_abi_version_stays_10():
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
    assert [a._type_ for a in lib.rt_render_features_pos.argtypes[3:]] == [capi.rt_feature, capi.rt_position]
    acc = lib.rt_temporal_accumulate.argtypes
    assert len(acc) == 16 and acc[1]._type_ is capi.rt_temporal_desc
    cur = [capi.rt_pixel, capi.rt_moment, capi.rt_feature, capi.rt_position]
    assert [a._type_ for a in acc[4:16]] == cur + cur + [C.c_float, capi.rt_pixel, capi.rt_moment,
                                                         capi.rt_temporal_info]
    assert [a._type_ for a in lib.rt_temporal_frame.argtypes[1:]] == [
        capi.rt_adaptive_desc, capi.rt_denoise_desc, C.c_float, capi.rt_pixel, capi.rt_temporal_info]
    assert lib.rt_temporal_begin.argtypes[1]._type_ is capi.rt_temporal_desc


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
    assert C.sizeof(capi.rt_position) == 16 and C.sizeof(capi.rt_temporal_desc) == 32
    assert C.sizeof(capi.rt_temporal_info) == 16


def test_null_context_is_an_argument_error():
    """Host-only behaviour of the new entries: a NULL context is RT_E_ARG, never a crash."""
    for name, call in null_calls(capi.load_library()).items():
        assert call() == capi.RT_E_ARG, name


@pytest.mark.parametrize("kind,code", [("bad_alloc", capi.RT_E_OOM), ("runtime", capi.RT_E_STATE),
                                       ("other", capi.RT_E_STATE)])
def test_new_entries_run_inside_the_firewall(monkeypatch, kind, code):
    """RTMI_FAULT_INJECT throws inside every guarded entry: the new ones come back with a status."""
    lib = capi.load_library()
    monkeypatch.setenv("RTMI_FAULT_INJECT", kind)
    for name, call in null_calls(lib).items():
        assert call() == code, name


def test_python_defaults_match_the_reference_module():
    """Renderer.temporal_*'s defaults are the ones the CPU quality test froze (tests/temporal_reference.py)."""
    import temporal_reference as ref
    from computational_ray_tracer_amd.renderer import TEMPORAL_DEFAULTS
    assert TEMPORAL_DEFAULTS == ref.DEFAULTS
