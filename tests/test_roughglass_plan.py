"""CPU: what a rough-glass material (RT_MAT_ROUGH_DIELECTRIC) changes in the render pass's plan
(csrc/rt_pass_plan.h): `rgl` selects RGH level 3 and implies `rgh`, the launchers' word gets bit 4 beside bit 2, a rough
glass sits in material class 0, and the NEE record is level 2's.  A small program of its own includes the header alone and
is built with the host compiler; the expected values are literals."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
HIP_INCLUDE = os.environ.get("ROCM_PATH", "/opt/rocm") + "/include"

SOURCE = r"""
#include <cstdio>
#include "rt_pass_plan.h"
using namespace rtmi;
static void show(const char* name, bool multi, int integ, bool rough, bool conductor, bool glass, bool env, bool mesh,
                 int n_lights) {
    PassFacts f;
    f.qcap = multi ? 0 : 1; f.n_tris = multi ? 100000 : 36; f.n_lights = n_lights; f.n_emit_tris = 2; f.coop_ok = multi;
    f.scene_full = true;
    f.mesh_light = mesh; f.environment = env; f.rough = rough; f.conductor = conductor; f.rough_dielectric = glass;
    f.integ = (PassIntegrator)integ; f.max_depth = 5; f.n_work = 1920 * 1080; f.ib = 0; f.ie = 16;
    const Knobs kn;
    const BatchPlan b = plan_batches(f, kn);
    const PathPlan p = plan_path(f, kn, b);
    std::printf("%s rgh=%d cnd=%d rgl=%d ml=%d level=%d extra=%d | full=%d B=%d nsh=%d lanes=%d sort=%d sort_nee=%d nee=%d "
                "bins=%d lean=%d env=%d emit_filter=%d records=%d hit_compact=%d nee_fallback=%d shadow=%d\n", name,
                (int)p.rgh, (int)p.cnd, (int)p.rgl, p.ml, rgh_level(p), nee_extra_f4(rgh_level(p), n_lights), (int)b.full,
                b.B, b.nsh, p.lanes, (int)p.sort_rays, (int)p.sort_nee, (int)p.nee, (int)p.bins, p.lean, (int)p.env,
                (int)p.emit_filter, (int)p.records, (int)p.hit_compact, (int)p.nee_fallback, (int)p.shadow);
}
int main() {
    for (int multi = 0; multi < 2; ++multi) {
        const char* names[5] = {multi ? "m_none" : "s_none", multi ? "m_rough" : "s_rough", multi ? "m_cnd" : "s_cnd",
                                multi ? "m_glass" : "s_glass", multi ? "m_all" : "s_all"};
        for (int v = 0; v < 5; ++v) show(names[v], multi, kIntegPath, v == 1 || v == 4, v == 2 || v == 4, v >= 3, false, false, 5);
    }
    show("env_mesh_glass", true, kIntegPathMis, false, false, true, true, true, 3);
    show("reference_glass", true, kIntegReference, true, true, true, false, false, 0);
    const PathPlan d;
    std::printf("defaults %d %d %d %d\n", (int)d.rgh, (int)d.cnd, (int)d.rgl, rgh_level(d));
    std::printf("classes %d%d%d%d%d%d %d%d%d%d%d%d\n", material_class(0, false), material_class(1, false),
                material_class(2, false), material_class(3, false), material_class(4, false), material_class(5, false),
                material_class(0, true), material_class(1, true), material_class(2, true), material_class(3, true),
                material_class(4, true), material_class(5, true));
    std::printf("facts %d%d%d%d%d%d %d | %d%d %d%d\n", (int)rough_dielectric_fact(0, false), (int)rough_dielectric_fact(1, false),
                (int)rough_dielectric_fact(2, false), (int)rough_dielectric_fact(3, false), (int)rough_dielectric_fact(4, false),
                (int)rough_dielectric_fact(5, false), (int)rough_dielectric_fact(5, true), (int)rough_fact(5, false),
                (int)conductor_fact(5, false), (int)rough_fact(3, false), (int)conductor_fact(4, false));
    std::printf("extra %d %d %d %d %d %d\n", nee_extra_f4(3, 1), nee_extra_f4(3, 4), nee_extra_f4(3, 5), nee_extra_f4(3, 0),
                nee_extra_f4(2, 5), nee_extra_f4(1, 5));
    return 0;
}
"""


def test_rough_glass_in_the_pass_plan(tmp_path):
    src = tmp_path / "roughglass_plan.cpp"
    src.write_text(SOURCE)
    exe = tmp_path / "roughglass_plan"
    r = subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + HIP_INCLUDE,
                        "-I" + str(ROOT / "computational_ray_tracer_amd" / "csrc"), "-o", str(exe), str(src)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith("RTMI_")}
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, env=env)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    got = {l.split()[0]: (l.split(" | ")[0].split()[1:], l.split(" | ")[1]) for l in lines if " | " in l and "=" in l}
    for pre in ("s", "m"):
        # none, rough, conductor, rough glass, all three: rgl implies rgh and not cnd; ml bits 2, 3 and 4; level 3's record
        # is level 2's (5 lights: the tail and two float4s of wo.h)
        assert got[pre + "_none"][0] == ["rgh=0", "cnd=0", "rgl=0", "ml=0", "level=0", "extra=0"]
        assert got[pre + "_rough"][0] == ["rgh=1", "cnd=0", "rgl=0", "ml=4", "level=1", "extra=1"]
        assert got[pre + "_cnd"][0] == ["rgh=1", "cnd=1", "rgl=0", "ml=12", "level=2", "extra=3"]
        assert got[pre + "_glass"][0] == ["rgh=1", "cnd=0", "rgl=1", "ml=20", "level=3", "extra=3"]
        assert got[pre + "_all"][0] == ["rgh=1", "cnd=1", "rgl=1", "ml=28", "level=3", "extra=3"]
        # every other decision is what it is without one
        for v in ("_rough", "_cnd", "_glass", "_all"):
            assert got[pre + v][1] == got[pre + "_none"][1], pre + v
    assert got["env_mesh_glass"][0] == ["rgh=1", "cnd=0", "rgl=1", "ml=23", "level=3", "extra=2"]
    # the reference integrator sees no material
    assert got["reference_glass"][0] == ["rgh=0", "cnd=0", "rgl=0", "ml=0", "level=0", "extra=0"]
    assert "defaults 0 0 0 0" in lines
    # material classes by (type, emissive): a rough glass sits with Lambert, rough and conductor in class 0
    assert "classes 011000 000000" in lines
    # the scene's facts: a non-emissive type 5 alone is a rough glass, and it is neither rough nor a conductor
    assert "facts 000001 0 | 00 11" in lines
    assert "extra 2 2 3 1 3 1" in lines
