"""CPU: the specular-chain guide pass's surface of the C-ABI: the header, the ctypes mirror and the
library agree on rt_render_features_chain, chain_depth took the place of the descriptors' first reserved word without
moving anything, the ABI version stays 10, and the new entry runs inside the exception firewall."""
import ctypes as C
import re
import subprocess
from pathlib import Path

from computational_ray_tracer_amd import capi
from computational_ray_tracer_amd.renderer import CHAIN_DEFAULTS, Renderer

ROOT = Path(__file__).resolve().parents[1]
HEADER = (ROOT / "include" / "rtmi355x.h").read_text()


def test_header_ctypes_and_library_agree():
    assert re.search(r"^#define RT_ABI_VERSION 10$", HEADER, re.M) and capi.ABI_VERSION == 10
    assert re.search(r"^#define RT_CHAIN_MAX 4$", HEADER, re.M) and capi.RT_CHAIN_MAX == 4
    assert re.search(r"^\s*int\s+rt_render_features_chain\s*\(", HEADER, re.M)
    assert "rt_render_features_chain" in capi.EXPORTS
    lib = capi.load_library()
    f = lib.rt_render_features_chain                 # AttributeError: the library does not export it
    assert f.restype is C.c_int and f.argtypes[1:4] == [C.c_int, C.c_int, C.c_int]
    assert [a._type_ for a in f.argtypes[4:]] == [capi.rt_feature, capi.rt_position]
    assert lib.rt_abi_version() == 10


def test_chain_depth_replaces_the_first_reserved_word(tmp_path):
    """gcc's layout of the header: both descriptors stay 32 B and chain_depth sits where reserved[0] sat."""
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "rtmi355x.h"', "int main(void) {",
             'printf("%zu %zu %zu %zu\\n", sizeof(rt_denoise_desc), offsetof(rt_denoise_desc, chain_depth), '
             "sizeof(rt_temporal_desc), offsetof(rt_temporal_desc, chain_depth));", "return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [32, 28, 32, 16]
    assert got == [C.sizeof(capi.rt_denoise_desc), capi.rt_denoise_desc.chain_depth.offset,
                   C.sizeof(capi.rt_temporal_desc), capi.rt_temporal_desc.chain_depth.offset]


def test_null_context_and_descriptor_defaults():
    lib = capi.load_library()
    assert lib.rt_render_features_chain(None, 0, 1, 1, None, None) == capi.RT_E_ARG
    assert CHAIN_DEFAULTS == dict(chain_depth=0)
    assert Renderer._denoise_desc().chain_depth == 0 and Renderer._temporal_desc().chain_depth == 0
    assert Renderer._denoise_desc(chain_depth=3).chain_depth == 3 and Renderer._temporal_desc(chain_depth=2).chain_depth == 2
    assert list(Renderer._temporal_desc(chain_depth=2).reserved) == [0, 0, 0]
