"""CPU: the single-leaf cluster cull's FMA form (csrc/rt_cull.h cluster_hit_fma, RT_CULL_FMA) is conservative, and the
four packed Cornell kernels fit 96 VGPRs (5 waves per SIMD).

tests/cluster_cull_driver.cpp includes rt_cull.h alone and is built with the host compiler, plain and with ASan + UBSan
(nothing is loaded into Python).  It restates leaf_clusters on the Cornell box's 36 triangles (18 boxes, pad 1e-5 ext +
1e-3 + 2^-22 |centre|) and draws 240 000 seeded segments with origins up to the guard radius (8 extents): general directions, every
pattern of zero direction components, origins on box face planes, components so small that o / d overflows, segments
aimed at box corners, edges and faces, segments along box edges; tMax finite or FLT_MAX.  Whenever the float64 segment
meets the UNPADDED bounds of a cluster's triangles, the FMA form must answer true: no exceptions, no skipped cases; the
same on the box moved 107 extents away from the coordinate origin, where the pad's centre term carries the bound.  How
often the FMA form and the subtract-multiply form disagree is printed, not asserted.

The register bounds are read from the built library's code-object metadata as tests/test_kernel_resources.py reads
them."""
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest

from computational_ray_tracer_amd import scene
from test_kernel_resources import NS, vgprs  # noqa: F401  (vgprs: the module-scoped fixture)

ROOT = Path(__file__).resolve().parents[1]
DRIVER = ROOT / "tests" / "cluster_cull_driver.cpp"
HIP_INCLUDE = os.environ.get("ROCM_PATH", "/opt/rocm") + "/include"
REPORTS = ("AddressSanitizer", "runtime error:", "LeakSanitizer")
SEGMENTS = 240000
SEED = 20261
OFFSET = (-60000.0, 25000.0, 3000.0)

# the four packed single-leaf kernels: all under the 96-VGPR line
PACKED = {
    NS + "12k_path_shadeILi1ELb0ELb1EEE": 96,          # k_path_shade<1, false, true>: depth 0 (was 105)
    NS + "15k_trace_closestILi1ELb0ELb1ELb1EEE": 96,   # k_trace_closest<1, false, true, true>: bounce depths (was 99)
    NS + "12k_path_shadeILi1ELb1ELb1EEE": 96,          # k_path_shade<1, true, true>: bounce depths (was 94)
    NS + "15k_trace_closestILi1ELb0ELb0ELb1EEE": 96,   # k_trace_closest<1, false, false, true>: depth 0 (was 91)
}


def _build(out, *flags):
    cmd = ["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-fno-fast-math", "-D__HIP_PLATFORM_AMD__",
           "-I" + HIP_INCLUDE, *flags, "-o", str(out), str(DRIVER)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def _run(exe, tris, env_extra=None, offset=()):
    env = {k: v for k, v in os.environ.items() if not k.startswith("RTMI_")}
    env.update(env_extra or {})
    r = subprocess.run([str(exe), str(tris), str(SEED), str(SEGMENTS), *map(str, offset)], capture_output=True,
                       text=True, timeout=300, env=env)
    assert r.returncode == 0 and not any(s in r.stdout + r.stderr for s in REPORTS), (r.stdout + r.stderr)[-4000:]
    return r.stdout


@pytest.fixture(scope="module")
def cornell_tris(tmp_path_factory):
    """The Cornell leaf's triangles in world space (object space with y and z swapped), float32, one per line."""
    m = scene.cornell_box()
    tri = np.asarray(m.positions, np.float32)[np.asarray(m.indices, np.int64)][:, :, [0, 2, 1]]
    assert tri.shape == (36, 3, 3)
    path = tmp_path_factory.mktemp("cull") / "cornell.txt"
    np.savetxt(path, tri.reshape(36, 9), fmt="%.9g")
    return path


@pytest.fixture(scope="module")
def plain_exe(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("cull_bin") / "cluster_cull")


@pytest.fixture(scope="module")
def plain_output(plain_exe, cornell_tris):
    return _run(plain_exe, cornell_tris)


def _counts(text):
    return {k: int(v) for k, v in (line.split() for line in text.splitlines() if not line.startswith("miss_fma"))}


def test_fma_form_never_rejects_a_box_the_segment_meets(plain_output):
    c = _counts(plain_output)
    print("\n" + plain_output)
    assert c["clusters"] == 18 and c["segments"] == SEGMENTS and c["tests"] == 18 * SEGMENTS
    assert all(c[f"class{k}"] == SEGMENTS // 6 for k in range(6))
    assert all(c[f"zeros{k}"] > 1000 for k in range(1, 7)) and c["zeros7"] == 0   # every zero pattern, many times
    assert c["ref_hits"] > 0.05 * c["tests"]                # the reference meets many boxes ...
    assert c["fma_true"] < 0.6 * c["tests"]                 # ... and the cull still rejects most pairs
    assert c["violations_fma"] == 0, plain_output
    assert c["violations_old"] == 0                         # (the subtract-multiply form: the same property)
    print(f"FMA form and subtract-multiply form disagree on {c['disagree']} of {c['tests']} (segment, box) pairs")


def test_scene_far_from_the_coordinate_origin(plain_exe, cornell_tris):
    """The same box moved to (-60000, 25000, 3000), 107 extents from the coordinate origin: the FMA form's error grows
    with |o|, 3 * 2^-24 * 6e4 = 0.011 here against the 0.0066 of 1e-5 ext + 1e-3; leaf_clusters' pad term 2^-22 |centre|
    (restated by the driver) covers that worst case, and the cull still rejects most (segment, box) pairs.  (The
    worst case is a bound, not what these segments reach: a driver without the term passes them too.  The case pins
    that the property holds off-origin with the pad as built, and that the cull is not switched off there.)"""
    out = _run(plain_exe, cornell_tris, offset=OFFSET)
    c = _counts(out)
    print("\n" + out)
    assert c["clusters"] == 18 and c["tests"] == 18 * SEGMENTS
    assert 20000 < c["pad_e6"] < 22000                       # 0.0066 + 2^-22 * 6e4 = 0.0209
    assert c["ref_hits"] > 0.05 * c["tests"] and c["fma_true"] < 0.6 * c["tests"]
    assert c["violations_fma"] == 0, out


def test_same_under_sanitizers(tmp_path, cornell_tris, plain_output):
    exe = _build(tmp_path / "cluster_cull_asan", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                 "-fno-sanitize-recover=undefined")
    assert _run(exe, cornell_tris, {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0"}) == plain_output


@pytest.mark.parametrize("prefix", sorted(PACKED))
def test_packed_cornell_kernels_fit_five_waves(vgprs, prefix):  # noqa: F811
    names = [n for n in vgprs if n.startswith(prefix)]
    assert len(names) == 1, f"{prefix}: {names}"
    v = vgprs[names[0]]
    print(f"{names[0][:60]}: {v} VGPRs (bound {PACKED[prefix]})")
    assert v <= PACKED[prefix]
