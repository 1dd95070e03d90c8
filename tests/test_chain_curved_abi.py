"""CPU: RT_CHAIN_CURVED in the C header, its ctypes mirror and the Python binding (DESIGN.md §3e "curved").  The flag
rides in the existing chain_depth fields: no struct, export or ABI version changes."""
import ctypes as C
import inspect
import re
from pathlib import Path

import pytest

from computational_ray_tracer_amd import capi, renderer
from computational_ray_tracer_amd.renderer import CHAIN_CURVED_DEFAULT, CHAIN_DEFAULTS, Renderer

HEADER = (Path(__file__).resolve().parents[1] / "include" / "rtmi355x.h").read_text()


def test_header_and_mirror():
    assert re.search(r"^#define RT_CHAIN_CURVED 0x100$", HEADER, re.M) and capi.RT_CHAIN_CURVED == 0x100
    assert capi.RT_CHAIN_CURVED > capi.RT_CHAIN_MAX and capi.RT_CHAIN_CURVED & capi.RT_CHAIN_MAX == 0
    assert re.search(r"^#define RT_ABI_VERSION 10$", HEADER, re.M)
    assert C.sizeof(capi.rt_denoise_desc) == 32 and C.sizeof(capi.rt_temporal_desc) == 32


def test_descriptors_carry_the_flag_in_chain_depth():
    d = Renderer._denoise_desc(chain_depth=2, chain_curved=True)
    assert d.chain_depth == 0x102
    assert Renderer._denoise_desc(chain_depth=2).chain_depth == 2
    assert Renderer._denoise_desc(chain_depth=2, chain_curved=False).chain_depth == 2
    assert Renderer._denoise_desc(chain_curved=True).chain_depth == 0x100
    t = Renderer._temporal_desc(chain_depth=4, chain_curved=True)
    assert t.chain_depth == 0x104 and list(t.reserved) == [0, 0, 0]
    assert list(Renderer._temporal_desc(chain_depth=1).reserved) == [0, 0, 0]
    assert Renderer._temporal_desc().chain_depth == 0 and Renderer._denoise_desc().chain_depth == 0


def test_defaults_and_signatures():
    assert CHAIN_CURVED_DEFAULT is False and CHAIN_DEFAULTS == dict(chain_depth=0)
    assert renderer.chain_arg(3) == 3 and renderer.chain_arg(3, True) == 3 | capi.RT_CHAIN_CURVED
    sig = inspect.signature(Renderer.render_features_chain)
    assert sig.parameters["chain_curved"].default is False
    with pytest.raises(TypeError, match="unknown denoise parameters"):
        Renderer._denoise_desc(chain_curve=True)
    with pytest.raises(TypeError, match="unknown temporal parameters"):
        Renderer._temporal_desc(curved=True)
