"""CPU: the media's part of the C ABI (include/rtmi355x.h): rt_medium's size and offsets against a
gcc-compiled probe, rt_material and the ABI version unchanged (the addition is additive), the new symbols exported,
listed and guarded, and the Python mirror's helpers."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np

from computational_ray_tracer_amd import capi, scene

ROOT = Path(__file__).resolve().parents[1]
NEW = ("rt_scene_set_media", "rt_medium_transmittance", "rt_debug_medium_eval", "rt_debug_medium_stats")


def test_struct_and_version_through_gcc(tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "rtmi355x.h"\nint main(void) {\n'
                   'printf("%zu %zu %zu %zu %d\\n", sizeof(rt_medium), offsetof(rt_medium, sigmoid), '
                   'offsetof(rt_medium, sigma), sizeof(rt_material), RT_ABI_VERSION);\nreturn 0; }\n')
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c11", "-I", str(ROOT / "include"), str(src), "-o", str(exe)], check=True)
    out = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert out[0] == 16 == C.sizeof(capi.rt_medium)
    assert out[1] == 0 == capi.rt_medium.sigmoid.offset and out[2] == 12 == capi.rt_medium.sigma.offset
    assert out[3] == 24 == C.sizeof(capi.rt_material)
    assert out[4] == 10 == capi.ABI_VERSION


def test_symbols_exported_and_listed():
    lib = capi.load_library()
    assert lib.rt_abi_version() == 10
    for s in NEW:
        assert s in capi.EXPORTS and hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s


def test_python_helpers():
    m = scene.Medium((0.0, 0.02, -11.6), 0.01)
    arr = scene.media_array([None, m])
    assert arr[0].sigma == 0.0 and tuple(arr[0].sigmoid) == (0.0, 0.0, 0.0)
    assert arr[1].sigma == np.float32(0.01) and arr[1].sigmoid[2] == np.float32(-11.6)
    a = scene.absorbing((0.5, 0.5, 0.5), 2.0)
    assert a.sigma == 2.0 and a.sigmoid == (0.0, 0.0, 0.0)                       # the uniform branch: S = 1/2
    t = scene.medium_transmittance(a, np.full((1, 8), 550.0), [1.0])
    assert t.shape == (1, 8) and np.all(t == np.float32(np.exp(-1.0)))
    # a colour's complement comes out: a medium that absorbs blue passes more red than blue
    b = scene.absorbing((0.1, 0.1, 0.9), 1.0)
    t = scene.medium_transmittance(b, np.array([[450.0] * 4 + [650.0] * 4]), [2.0])
    assert t[0, 0] < 0.5 * t[0, 7]


def test_host_entries_are_guarded():
    lib = capi.load_library()
    F = C.POINTER(C.c_float)
    m = (capi.rt_medium * 1)()
    m[0].sigma = 1.0
    lam, ln, out = np.full(8, 500.0, np.float32), np.ones(1, np.float32), np.full(8, -1.0, np.float32)
    p = lambda x: x.ctypes.data_as(F)
    assert lib.rt_medium_transmittance(m, 1, p(lam), p(ln), p(out)) == capi.RT_OK
    assert np.all(out == np.float32(np.exp(-0.5)))
    assert lib.rt_medium_transmittance(None, 0, None, None, None) == capi.RT_OK           # n == 0 reads nothing
    assert lib.rt_medium_transmittance(m, -1, p(lam), p(ln), p(out)) == capi.RT_E_ARG
    for k in range(4):
        args = [m, p(lam), p(ln), p(out)]
        args[k] = None
        assert lib.rt_medium_transmittance(args[0], 1, *args[1:]) == capi.RT_E_ARG, k
    # the context entries reject a NULL context before anything else
    assert lib.rt_scene_set_media(None, m, 1) == capi.RT_E_ARG
    assert lib.rt_debug_medium_eval(None, m, 1, p(lam), p(ln), p(out)) == capi.RT_E_ARG
    assert lib.rt_debug_medium_stats(None, None, None) == capi.RT_E_ARG
