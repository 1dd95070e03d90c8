"""CPU: the render pass's decisions (csrc/rt_pass_plan.h: batch sizing, the path pass's plan, the per-depth answers).
tests/pass_plan_driver.cpp includes that header alone, is built with the host compiler (plain, and with ASan + UBSan;
nothing is loaded into Python) and prints the plans of the cases below.  The expected values are literals worked out
by hand from the host pass as it stood before the plan header existed (render_device_body / features_device /
hit_pack_active / ensure_workspace of commit 576b4d1), not from the header."""
import os
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
DRIVER = ROOT / "tests" / "pass_plan_driver.cpp"
HIP_INCLUDE = os.environ.get("ROCM_PATH", "/opt/rocm") + "/include"
REPORTS = ("AddressSanitizer", "runtime error:", "LeakSanitizer")

REF, PATH, MIS = 0, 1, 2
HD = 1920 * 1080  # 2 073 600 pixels; 16 Mi / HD = 8.09, 32 Mi / HD = 16.18

# the Cornell-like base: one leaf, simple path, 1 light, 36 triangles, depth 5, indices [0, 16)
CORNELL = dict(qcap=1, n_tris=36, n_lights=1, n_emit_tris=2, coop_ok=0, integ=PATH, max_depth=5, n_work=HD, ib=0, ie=16)
# a multi-level simple scene (qcap 0: BFS ring, 16: register FIFO), indices [0, 32)
MULTI = dict(qcap=0, n_tris=100000, n_lights=1, n_emit_tris=2, coop_ok=1, integ=PATH, max_depth=5, n_work=HD, ib=0, ie=32)
# ... and a mixed one (4 lights) once `full` is raised by the scene, the integrator or live textures
MIXED = dict(MULTI, n_lights=4)

SIMPLE_DEPTHS = {  # single leaf, packing: depth 0 carries the hit word, bounces the packed hit queue, depth 5 stops
    0: dict(traced=1, efilter=0, sort=0, next_keys=0, hit_compact=0, hit_pack=0, pack0=1, trace_fallback=0,
            nee_fallback=0, shadow=0),
    2: dict(traced=1, efilter=0, sort=0, hit_compact=1, hit_pack=1, pack0=0, shadow=0),
    4: dict(traced=1, efilter=0, sort=0, hit_compact=1, hit_pack=1, pack0=0),
    5: dict(traced=0),
}
UNPACKED_DEPTHS = {0: dict(traced=1, hit_compact=0, hit_pack=0, pack0=0), 2: dict(hit_compact=1, hit_pack=0, pack0=0),
                   4: dict(hit_compact=1, hit_pack=0, pack0=0), 5: dict(traced=0)}
NO_COMPACT_DEPTHS = {0: dict(traced=1, hit_compact=0, hit_pack=0, pack0=0), 2: dict(hit_compact=0, hit_pack=0, pack0=0),
                     4: dict(hit_compact=0, hit_pack=0, pack0=0), 5: dict(traced=0)}
HD8 = dict(B=8, nmax=16588800, nsh=1, ncap=16588800, nbatch=2, dyn=0, trace_fallback=0)      # 8 HD = 64 x 259 200
HD16 = dict(B=16, nmax=33177600, nsh=8, ncap=33177600, nbatch=2, dyn=1)                      # 16 HD / 8 = 64 x 64 800


def multi_depths(sort=1, fallback=0, shadow=0):
    return {0: dict(traced=1, efilter=0, sort=0, next_keys=sort, hit_compact=0, pack0=0, trace_fallback=fallback,
                    nee_fallback=0, shadow=shadow),
            2: dict(traced=1, efilter=0, sort=sort, next_keys=sort, trace_fallback=fallback, shadow=shadow),
            4: dict(traced=1, efilter=0, sort=sort, next_keys=sort, hit_compact=0, trace_fallback=fallback, shadow=shadow),
            5: dict(traced=0)}


def mixed_depths(efilter=1, sort=1, nee_fallback=0, fallback=0):
    # the last depth is traced; the emitter filter runs there alone and takes the place of the sort
    return {0: dict(traced=1, efilter=0, sort=0, next_keys=sort, nee_fallback=nee_fallback, trace_fallback=fallback,
                    shadow=0),
            2: dict(traced=1, efilter=0, sort=sort, next_keys=sort, nee_fallback=nee_fallback, shadow=0),
            4: dict(traced=1, efilter=0, sort=sort, next_keys=sort, nee_fallback=nee_fallback),
            5: dict(traced=1, efilter=efilter, sort=sort if not efilter else 0, next_keys=0, hit_compact=0,
                    nee_fallback=nee_fallback, trace_fallback=fallback, shadow=0)}


MIXED_PATH = dict(lanes=2, sort_rays=1, sort_nee=1, org_major=0, hit_compact=0, hit_pack=0, hit_d=0, lean=2, shq=0,
                  defer=0, nee=1, bins=1, records=1, rec_fs=1, rec_ss=8, rec_rng8=0)
MULTI_PATH = dict(lanes=2, sort_rays=1, sort_nee=0, org_major=1, hit_compact=0, hit_pack=0, hit_d=0, lean=1, shq=1,
                  defer=1, nee=0, bins=0, ml=0, records=1, rec_fs=1, rec_ss=8, rec_rng8=0)

# name -> (fields, batch line, path line or None, {depth: depth line}); every dict lists only what the case pins
CASES = {
    "cornell": (CORNELL, dict(HD8, path=1, mis=0, full=0),
                dict(lanes=2, sort_rays=0, sort_nee=0, hit_compact=1, hit_pack=1, hit_d=0, lean=1, shq=0, defer=0, nee=0,
                     bins=0, ml=0, records=0, rec_fs=16588800, rec_ss=1, rec_rng8=1), SIMPLE_DEPTHS),
    "tris65": (dict(CORNELL, n_tris=65), HD8, dict(hit_compact=1, hit_pack=0, hit_d=1), UNPACKED_DEPTHS),
    "tris64": (dict(CORNELL, n_tris=64), HD8, dict(hit_compact=1, hit_pack=1, hit_d=0), SIMPLE_DEPTHS),
    # RTMI_BATCH_SAMPLES = 10 HD: B = 10, 20 736 000 samples > 2^24 = 16 777 216
    "slots": (dict(CORNELL, **{"k.batch_samples": 10 * HD}), dict(B=10, nmax=20736000, ncap=20736000, nbatch=2),
              dict(hit_compact=1, hit_pack=0, hit_d=1, rec_fs=20736000), UNPACKED_DEPTHS),
    "compact0": (dict(CORNELL, **{"k.hit_compact": 0}), HD8, dict(hit_compact=0, hit_pack=0, hit_d=0), NO_COMPACT_DEPTHS),
    "pack0": (dict(CORNELL, **{"k.hit_pack": 0}), HD8, dict(hit_compact=1, hit_pack=0, hit_d=1), UNPACKED_DEPTHS),
    "mesh_light": (dict(CORNELL, mesh_light=1), HD8, dict(ml=1, hit_pack=1), SIMPLE_DEPTHS),
    # multi-level simple scenes
    "multi_ring": (MULTI, dict(HD16, path=1, mis=0, full=0, trace_fallback=0), MULTI_PATH, multi_depths()),
    "multi_fifo": (dict(MULTI, qcap=16), dict(HD16, full=0, trace_fallback=0), MULTI_PATH, multi_depths()),
    "multi_nocoop": (dict(MULTI, coop_ok=0), dict(HD16, trace_fallback=1), MULTI_PATH,
                     multi_depths(fallback=1, shadow=1)),
    "multi_fifo_nocoop": (dict(MULTI, qcap=16, coop_ok=0), dict(HD16, trace_fallback=1), MULTI_PATH,
                          multi_depths(fallback=1, shadow=1)),
    "multi_shadowq": (dict(MULTI, **{"k.shadow_queue": 1}), HD16, dict(MULTI_PATH, defer=0),
                      multi_depths(fallback=0, shadow=1)),
    "multi_nosort": (dict(MULTI, **{"k.sort_rays": 0}), HD16, dict(MULTI_PATH, sort_rays=0), multi_depths(sort=0)),
    "multi_major0": (dict(MULTI, **{"k.sort_org_major": 0}), HD16, dict(MULTI_PATH, org_major=0), multi_depths()),
    # multi-level mixed scenes
    "mixed_scene": (dict(MIXED, scene_full=1), dict(HD16, path=1, mis=0, full=1), MIXED_PATH, mixed_depths()),
    "mixed_mis": (dict(MIXED, integ=MIS), dict(HD16, path=1, mis=1, full=1), MIXED_PATH, mixed_depths()),
    "mixed_tex": (dict(MIXED, textures=1), dict(HD16, path=1, mis=0, full=1), MIXED_PATH, mixed_depths()),
    "mixed_fifo": (dict(MIXED, scene_full=1, qcap=16), dict(HD16, full=1), MIXED_PATH, mixed_depths()),
    "mixed_dark": (dict(MIXED, scene_full=1, n_lights=0), dict(HD16, full=1),
                   dict(MIXED_PATH, nee=0, bins=0, sort_nee=0), mixed_depths()),
    "mixed_nobins": (dict(MIXED, scene_full=1, **{"k.mat_bins": 0}), HD16, dict(MIXED_PATH, bins=0), mixed_depths()),
    "mixed_noneesort": (dict(MIXED, scene_full=1, **{"k.sort_nee": 0}), HD16, dict(MIXED_PATH, sort_nee=0),
                        mixed_depths()),
    "mixed_nosort": (dict(MIXED, scene_full=1, **{"k.sort_rays": 0}), HD16, dict(MIXED_PATH, sort_rays=0, sort_nee=0),
                     mixed_depths(sort=0)),
    "mixed_major1": (dict(MIXED, scene_full=1, **{"k.sort_org_major": 1}), HD16, dict(MIXED_PATH, org_major=1),
                     mixed_depths()),
    "mixed_nofilter": (dict(MIXED, scene_full=1, **{"k.emit_filter": 0}), HD16, MIXED_PATH, mixed_depths(efilter=0)),
    "mixed_noemit": (dict(MIXED, scene_full=1, n_emit_tris=-1), HD16, MIXED_PATH, mixed_depths(efilter=0)),
    "mixed_emit0": (dict(MIXED, scene_full=1, n_emit_tris=0), HD16, MIXED_PATH, mixed_depths(efilter=1)),
    "mixed_nocoop": (dict(MIXED, scene_full=1, coop_ok=0), dict(HD16, trace_fallback=1), MIXED_PATH,
                     mixed_depths(nee_fallback=1, fallback=1)),
    "mixed_dark_nocoop": (dict(MIXED, scene_full=1, coop_ok=0, n_lights=0), dict(HD16, trace_fallback=1),
                          dict(MIXED_PATH, nee=0, bins=0, sort_nee=0), mixed_depths(nee_fallback=0, fallback=1)),
    "mixed_depth0": (dict(MIXED, scene_full=1, max_depth=0), HD16, MIXED_PATH,
                     {0: dict(traced=1, efilter=0, sort=0, next_keys=0, nee_fallback=0)}),
    # one leaf, MIS: the general kernels with NEE, no bins, no sort, no hit queue; the last depth is traced and filtered
    "leaf_mis": (dict(CORNELL, integ=MIS), dict(HD8, path=1, mis=1, full=1),
                 dict(lanes=2, sort_rays=0, sort_nee=0, hit_compact=0, hit_pack=0, hit_d=0, lean=2, shq=0, nee=1, bins=0,
                      records=0, rec_fs=16588800, rec_ss=1, rec_rng8=0),
                 {0: dict(traced=1, efilter=0, sort=0, next_keys=0, hit_compact=0, pack0=0, nee_fallback=0, shadow=0),
                  2: dict(traced=1, efilter=0, sort=0, hit_compact=0, hit_pack=0, nee_fallback=0),
                  4: dict(traced=1, efilter=0, sort=0, hit_compact=0),
                  5: dict(traced=1, efilter=1, sort=0, next_keys=0, hit_compact=0, trace_fallback=0, nee_fallback=0)}),
    # the reference integrator: the same sizing
    "reference": (dict(CORNELL, integ=REF), dict(HD8, path=0, mis=0, full=0), None, {}),
    "reference_multi": (dict(MULTI, integ=REF, scene_full=1), dict(HD16, path=0, mis=0, full=1), None, {}),
    # batch-sizing edges
    "big_list": (dict(CORNELL, n_work=20000000, ie=3), dict(B=1, nmax=20000000, ncap=20000000, nbatch=3),
                 dict(lanes=2, hit_pack=0, hit_compact=1), UNPACKED_DEPTHS),
    "short_range": (dict(CORNELL, n_work=1000, ib=2, ie=5), dict(B=3, nmax=3000, nsh=1, ncap=3008, nbatch=1),
                    dict(lanes=1, hit_pack=1, rec_fs=3000), SIMPLE_DEPTHS),
    "short_shards": (dict(MULTI, n_work=1000, ib=0, ie=3), dict(B=3, nmax=3000, nsh=8, ncap=3072, nbatch=1),
                     dict(MULTI_PATH, lanes=1), multi_depths()),
    "ragged": (dict(CORNELL, ie=20), dict(HD8, nbatch=3), dict(lanes=2), SIMPLE_DEPTHS),
    "ragged_lanes4": (dict(CORNELL, ie=20, **{"k.lanes": 4}), dict(HD8, nbatch=3), dict(lanes=3), SIMPLE_DEPTHS),
    "lanes_cap": (dict(CORNELL, ie=40, **{"k.lanes": 9}), dict(HD8, nbatch=5), dict(lanes=4), SIMPLE_DEPTHS),
    "lanes_knob1": (dict(CORNELL, ie=40, **{"k.lanes": 1}), dict(HD8, nbatch=5), dict(lanes=1), SIMPLE_DEPTHS),
    "depth0": (dict(CORNELL, max_depth=0), HD8, dict(hit_pack=1),
               {0: dict(traced=1, efilter=0, sort=0, hit_compact=0, pack0=1)}),
    "depth1": (dict(CORNELL, max_depth=1), HD8, dict(hit_pack=1), {0: dict(traced=1, pack0=1), 1: dict(traced=0)}),
    "empty_range": (dict(CORNELL, ib=4, ie=4), dict(nbatch=0, path=1), None, {}),
    "empty_list": (dict(CORNELL, n_work=0), dict(nbatch=0), None, {}),
}


def _build(out, *flags):
    cmd = ["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + HIP_INCLUDE, *flags, "-o", str(out), str(DRIVER)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def _run(exe, env_extra=None, cases=CASES):
    env = {k: v for k, v in os.environ.items() if not k.startswith("RTMI_")}
    env.update(env_extra or {})
    args = [name + ":" + ",".join(f"{k}={v}" for k, v in spec[0].items()) for name, spec in cases.items()]
    r = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and not any(s in r.stdout + r.stderr for s in REPORTS), (r.stdout + r.stderr)[-4000:]
    return r.stdout


def _parse(text):
    plans, cur = {}, None
    for line in text.splitlines():
        head, *kv = line.split()
        if head == "case":
            cur = plans.setdefault(kv[0], {"depth": {}})
            continue
        if head == "depth":
            depth, *kv = kv
        fields = {k: int(v) for k, v in (item.split("=") for item in kv)}
        if head == "depth":
            cur["depth"][int(depth)] = fields
        else:
            cur[head] = fields
    return plans


@pytest.fixture(scope="module")
def plain_output(tmp_path_factory):
    return _run(_build(tmp_path_factory.mktemp("pass_plan") / "pass_plan"))


@pytest.fixture(scope="module")
def plans(plain_output):
    return _parse(plain_output)


@pytest.mark.parametrize("name", list(CASES))
def test_plan(plans, name):
    fields, batch, path, depths = CASES[name]
    got = plans[name]
    assert {k: got["batch"][k] for k in batch} == batch
    if path is None:
        assert "path" not in got or not got["batch"]["nbatch"]
    else:
        assert {k: got["path"][k] for k in path} == path
    assert sorted(got["depth"]) == (list(range(fields["max_depth"] + 1)) if "path" in got else [])
    for depth, want in depths.items():
        assert {k: got["depth"][depth][k] for k in want} == want, depth


def test_depths_asserted():
    """Every path case pins depth 0, a middle depth, max_depth - 1 and max_depth (where the scene has them)."""
    for name, (fields, _, path, depths) in CASES.items():
        if path is None:
            continue
        md = fields["max_depth"]
        want = {0, md} | ({md - 1, md // 2} if md >= 4 else set())
        assert want <= set(depths), name


def test_same_under_sanitizers(tmp_path, plain_output):
    """The same program under ASan + UBSan (built like tests/sanitize's drivers): no report, the same output."""
    exe = _build(tmp_path / "pass_plan_asan", "-g", "-O1", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                 "-fno-sanitize-recover=undefined")
    assert _run(exe, {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0"}) == plain_output


def test_knobs_come_from_the_environment(tmp_path_factory, plans):
    """read_knobs feeds the plan: the RTMI_* variables give what the same values give as fields."""
    exe = tmp_path_factory.mktemp("pass_plan_env") / "pass_plan"
    _build(exe)
    env = {"RTMI_BATCH_SAMPLES": str(10 * HD), "RTMI_LANES": "9", "RTMI_HIT_COMPACT": "1"}
    got = _parse(_run(exe, env, {"cornell": CASES["cornell"]}))["cornell"]
    assert {k: got["batch"][k] for k in ("B", "nmax", "nbatch")} == dict(B=10, nmax=20736000, nbatch=2)
    assert got["path"]["hit_pack"] == 0 and got["path"]["hit_d"] == 1 and got["path"]["lanes"] == 2
    env = {"RTMI_SORT": "0", "RTMI_SHADOW_QUEUE": "1", "RTMI_MAT_BINS": "0", "RTMI_EMIT_FILTER": "0",
           "RTMI_SORT_NEE": "0", "RTMI_HIT_PACK": "0", "RTMI_LANES": "1"}
    got = _parse(_run(exe, env, {k: CASES[k] for k in ("cornell", "multi_ring", "mixed_scene")}))
    assert got["cornell"]["path"]["hit_pack"] == 0 and got["cornell"]["path"]["lanes"] == 1
    assert got["multi_ring"]["path"]["sort_rays"] == 0 and got["multi_ring"]["path"]["defer"] == 0
    assert got["mixed_scene"]["path"]["bins"] == 0 and got["mixed_scene"]["path"]["sort_nee"] == 0
    assert got["mixed_scene"]["depth"][5]["efilter"] == 0
