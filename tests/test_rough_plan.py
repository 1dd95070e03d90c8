"""CPU: what a rough material (RT_MAT_ROUGH) changes in the render pass's plan (csrc/rt_pass_plan.h): the
launchers' word gets bit 2 and `rgh` selects the RGH instantiations, a rough material sits in material class 0, the
Lambert bin, and every other decision is what it is for the same scene without one.  A small program of its own
includes the header alone and is built with the host compiler; the expected values are literals."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
HIP_INCLUDE = os.environ.get("ROCM_PATH", "/opt/rocm") + "/include"

SOURCE = r"""
#include <cstdio>
#include "rt_pass_plan.h"
using namespace rtmi;
static void show(const char* name, bool multi, int integ, bool rough, bool env, bool mesh, int n_lights) {
    PassFacts f;
    f.qcap = multi ? 0 : 1; f.n_tris = multi ? 100000 : 36; f.n_lights = n_lights; f.n_emit_tris = 2; f.coop_ok = multi;
    f.scene_full = true;   // (a rough material is not diffuse: the upload's full flag is set with or without it here)
    f.mesh_light = mesh; f.environment = env; f.rough = rough;
    f.integ = (PassIntegrator)integ; f.max_depth = 5; f.n_work = 1920 * 1080; f.ib = 0; f.ie = 16;
    const Knobs kn;
    const BatchPlan b = plan_batches(f, kn);
    const PathPlan p = plan_path(f, kn, b);
    std::printf("%s rgh=%d ml=%d | full=%d B=%d nsh=%d lanes=%d sort=%d sort_nee=%d nee=%d bins=%d lean=%d env=%d "
                "emit_filter=%d records=%d hit_compact=%d nee_fallback=%d shadow=%d", name, (int)p.rgh, p.ml, (int)b.full,
                b.B, b.nsh, p.lanes, (int)p.sort_rays, (int)p.sort_nee, (int)p.nee, (int)p.bins, p.lean, (int)p.env,
                (int)p.emit_filter, (int)p.records, (int)p.hit_compact, (int)p.nee_fallback, (int)p.shadow);
    for (int d = 0; d <= 6; ++d) std::printf(" d%d=%d%d%d%d", d, (int)p.at(d).traced, (int)p.at(d).env_miss,
                                             (int)p.at(d).efilter, (int)p.at(d).sort);
    std::printf("\n");
}
int main() {
    show("cornell2", false, kIntegPathMis, false, false, false, 2);
    show("cornell2_rough", false, kIntegPathMis, true, false, false, 2);
    show("mixed", true, kIntegPath, false, false, false, 4);
    show("mixed_rough", true, kIntegPath, true, false, false, 4);
    show("env_mesh", true, kIntegPathMis, false, true, true, 3);
    show("env_mesh_rough", true, kIntegPathMis, true, true, true, 3);
    show("reference", true, kIntegReference, false, false, false, 0);
    show("reference_rough", true, kIntegReference, true, false, false, 0);
    std::printf("classes %d%d%d%d %d%d%d%d\n", material_class(0, false), material_class(1, false), material_class(2, false),
                material_class(3, false), material_class(0, true), material_class(1, true), material_class(2, true),
                material_class(3, true));
    std::printf("facts %d%d%d%d %d\n", (int)rough_fact(0, false), (int)rough_fact(1, false), (int)rough_fact(2, false),
                (int)rough_fact(3, false), (int)rough_fact(3, true));
    return 0;
}
"""


def test_rough_material_in_the_pass_plan(tmp_path):
    src = tmp_path / "rough_plan.cpp"
    src.write_text(SOURCE)
    exe = tmp_path / "rough_plan"
    r = subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + HIP_INCLUDE,
                        "-I" + str(ROOT / "computational_ray_tracer_amd" / "csrc"), "-o", str(exe), str(src)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith("RTMI_")}
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, env=env)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    got = {l.split()[0]: (l.split(" | ")[0].split()[1:], l.split(" | ")[1]) for l in lines if " | " in l}
    # RGH and the launchers' word: bit 2 with a rough material, beside the mesh (1) and environment (2) bits
    assert got["cornell2"][0] == ["rgh=0", "ml=0"] and got["cornell2_rough"][0] == ["rgh=1", "ml=4"]
    assert got["mixed"][0] == ["rgh=0", "ml=0"] and got["mixed_rough"][0] == ["rgh=1", "ml=4"]
    assert got["env_mesh"][0] == ["rgh=0", "ml=3"] and got["env_mesh_rough"][0] == ["rgh=1", "ml=7"]
    # the reference integrator sees no material
    assert got["reference"][0] == ["rgh=0", "ml=0"] and got["reference_rough"][0] == ["rgh=0", "ml=0"]
    # everything else is equal with and without one
    for name in ("cornell2", "mixed", "env_mesh", "reference"):
        assert got[name][1] == got[name + "_rough"][1], name
    # and is what it was (the mixed multi-level scene: bins, both sorts, the last depth's emitter filter)
    assert got["mixed"][1].startswith("full=1 B=16 nsh=8 lanes=1 sort=1 sort_nee=1 nee=1 bins=1 lean=2 env=0 emit_filter=1 "
                                      "records=1 hit_compact=0 nee_fallback=0 shadow=0 d0=1000 d1=1001")
    assert got["cornell2"][1].startswith("full=1 B=8 nsh=1 lanes=2 sort=0 sort_nee=0 nee=1 bins=0 lean=2 env=0 "
                                         "emit_filter=1 records=0 hit_compact=0")
    # material classes by (type, emissive): rough sits with Lambert in class 0; an emitter of any type is class 0
    assert "classes 0110 0000" in lines
    # the scene's rough fact: a non-emissive type 3 alone
    assert "facts 0001 0" in lines
