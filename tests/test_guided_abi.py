"""CPU: the guided temporal frame's surface of the C-ABI: the header, the ctypes mirror and the library
agree on rt_temporal_frame_guided and rt_temporal_block_error, the ABI version stays 10, rt_temporal_desc keeps its
layout (the feature is an entry point, not a flag), and both entries run inside the exception firewall."""
import ctypes as C
import re
import subprocess
from pathlib import Path

import pytest

from computational_ray_tracer_amd import capi

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "rtmi355x.h").read_text()
P = C.POINTER


def test_header_ctypes_and_library_agree():
    assert re.search(r"^#define RT_ABI_VERSION 10$", HEADER, re.M) and capi.ABI_VERSION == 10
    for name in ("rt_temporal_frame_guided", "rt_temporal_block_error"):
        assert re.search(r"^\s*int\s+%s\s*\(" % name, HEADER, re.M), name
        assert name in capi.EXPORTS
    lib = capi.load_library()
    assert lib.rt_abi_version() == 10
    f = lib.rt_temporal_frame_guided               # AttributeError: the library does not export it
    assert f.restype is C.c_int and f.argtypes[0] is C.c_void_p
    assert [a._type_ for a in f.argtypes[1:]] == [capi.rt_adaptive_desc, capi.rt_denoise_desc, C.c_float, capi.rt_pixel,
                                                  capi.rt_temporal_info, capi.rt_adaptive_info]
    g = lib.rt_temporal_block_error
    assert g.restype is C.c_int and g.argtypes[0] is C.c_void_p and g.argtypes[3:5] == [C.c_int, C.c_int]
    assert [a._type_ for a in g.argtypes[1:3]] == [capi.rt_temporal_desc, capi.rt_adaptive_desc]
    assert [a._type_ for a in g.argtypes[5:]] == [capi.rt_pixel, capi.rt_moment, capi.rt_feature, capi.rt_position,
                                                  capi.rt_pixel, capi.rt_moment, capi.rt_feature, capi.rt_position,
                                                  C.c_float, C.c_float, C.c_int32]


def test_temporal_desc_layout_is_unchanged(tmp_path):
    """gcc's layout of the header: rt_temporal_desc is 32 B and ends in three reserved words."""
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "rtmi355x.h"', "int main(void) {",
             "rt_temporal_desc d;",
             'printf("%zu %zu %zu\\n", sizeof(rt_temporal_desc), offsetof(rt_temporal_desc, reserved), '
             "sizeof(d.reserved) / sizeof(d.reserved[0]));", "return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [32, 20, 3]
    assert got == [C.sizeof(capi.rt_temporal_desc), capi.rt_temporal_desc.reserved.offset,
                   len(capi.rt_temporal_desc().reserved)]


def null_calls(lib):
    return {
        "rt_temporal_frame_guided": lambda: lib.rt_temporal_frame_guided(None, None, None, None, None, None, None),
        "rt_temporal_block_error": lambda: lib.rt_temporal_block_error(None, None, None, 8, 8, *([None] * 11)),
    }


def test_null_context_is_an_argument_error():
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
