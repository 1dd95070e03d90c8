"""CPU: the denoiser's surface of the C-ABI: the header, the ctypes mirror and the library agree on
the three entry points, the two structs have gcc's layout, and the addition leaves the ABI version at 10."""
import ctypes as C
import re
import subprocess
from pathlib import Path

from computational_ray_tracer_amd import capi

ROOT = Path(__file__).resolve().parents[1]
NEW_SYMBOLS = ["rt_render_features", "rt_denoise", "rt_adaptive_denoise"]
NEW_STRUCTS = ["rt_feature", "rt_denoise_desc"]


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
    assert lib.rt_render_features.argtypes[3]._type_ is capi.rt_feature
    assert lib.rt_denoise.argtypes[1]._type_ is capi.rt_denoise_desc
    assert [a._type_ for a in lib.rt_denoise.argtypes[4:9]] == [capi.rt_pixel, capi.rt_moment, capi.rt_feature,
                                                                capi.rt_pixel, C.c_float]
    assert lib.rt_adaptive_denoise.argtypes[1]._type_ is capi.rt_denoise_desc
    assert lib.rt_adaptive_denoise.argtypes[2]._type_ is capi.rt_pixel


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
    assert C.sizeof(capi.rt_feature) == 16 and C.sizeof(capi.rt_denoise_desc) == 32


def test_null_context_is_an_argument_error():
    """Host-only behaviour of the new entries (no device needed): a NULL context is RT_E_ARG, never a crash."""
    lib = capi.load_library()
    d = capi.rt_denoise_desc()
    assert lib.rt_render_features(None, 0, 1, None) == capi.RT_E_ARG
    assert lib.rt_denoise(None, C.byref(d), 1, 1, None, None, None, None, None) == capi.RT_E_ARG
    assert lib.rt_adaptive_denoise(None, C.byref(d), None) == capi.RT_E_ARG


def test_python_defaults_match_the_reference_module():
    """Renderer.denoise's defaults are the ones the CPU usefulness test froze (tests/denoise_reference.py)."""
    import denoise_reference as ref
    from computational_ray_tracer_amd.renderer import DENOISE_DEFAULTS
    assert DENOISE_DEFAULTS == ref.DEFAULTS
