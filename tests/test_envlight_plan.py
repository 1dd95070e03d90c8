"""CPU: what a bound environment light changes in the render pass's plan (csrc/rt_pass_plan.h): the scene
becomes `full`, the launchers' tabled-light word gets bit 1, every traced depth ends with the miss stage, the last
depth's emitter filter is off — and nothing changes without one.  A small program of its own includes the header alone
and is built with the host compiler; the expected values are literals."""
import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
HIP_INCLUDE = os.environ.get("ROCM_PATH", "/opt/rocm") + "/include"

SOURCE = r"""
#include <cstdio>
#include "rt_pass_plan.h"
using namespace rtmi;
static void show(const char* name, bool multi, int integ, bool env, bool mesh, int n_lights) {
    PassFacts f;
    f.qcap = multi ? 0 : 1; f.n_tris = multi ? 100000 : 36; f.n_lights = n_lights; f.n_emit_tris = 2; f.coop_ok = multi;
    f.mesh_light = mesh; f.environment = env;
    f.integ = (PassIntegrator)integ; f.max_depth = 5; f.n_work = 1920 * 1080; f.ib = 0; f.ie = 16;
    const Knobs kn;
    const BatchPlan b = plan_batches(f, kn);
    const PathPlan p = plan_path(f, kn, b);
    std::printf("%s full=%d env=%d ml=%d nee=%d bins=%d lean=%d emit_filter=%d", name, (int)b.full, (int)p.env, p.ml,
                (int)p.nee, (int)p.bins, p.lean, (int)p.emit_filter);
    for (int d = 0; d <= 6; ++d) std::printf(" d%d=%d%d%d", d, (int)p.at(d).traced, (int)p.at(d).env_miss, (int)p.at(d).efilter);
    std::printf("\n");
}
int main() {
    show("cornell", false, kIntegPath, false, false, 1);
    show("cornell_env", false, kIntegPath, true, false, 2);
    show("cornell_env_only", false, kIntegPath, true, false, 1);
    show("mixed", true, kIntegPathMis, false, false, 4);
    show("mixed_env", true, kIntegPathMis, true, false, 5);
    show("mesh_env", true, kIntegPath, true, true, 2);
    show("reference_env", false, kIntegReference, true, false, 2);
    return 0;
}
"""


def test_environment_in_the_pass_plan(tmp_path):
    src = tmp_path / "env_plan.cpp"
    src.write_text(SOURCE)
    exe = tmp_path / "env_plan"
    r = subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + HIP_INCLUDE,
                        "-I" + str(ROOT / "computational_ray_tracer_amd" / "csrc"), "-o", str(exe), str(src)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith("RTMI_")}
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, env=env)
    assert out.returncode == 0, out.stderr
    got = {l.split()[0]: dict(kv.split("=") for kv in l.split()[1:]) for l in out.stdout.splitlines()}
    depths = lambda traced_to, miss, filt_at=None: {
        f"d{d}": f"{int(d <= traced_to)}{int(miss and d <= traced_to)}{int(d == filt_at)}" for d in range(7)}
    # the simple path stops before its last depth (only emitter hits could count there) and has no miss stage
    assert got["cornell"] == dict(full="0", env="0", ml="0", nee="0", bins="0", lean="1", emit_filter="0", **depths(4, False))
    # a map: the general kernels, the environment's bit, depths 0..5 all traced, each with the miss stage, no filter
    want_env = dict(full="1", env="1", ml="2", nee="1", bins="0", lean="2", emit_filter="0", **depths(5, True))
    assert got["cornell_env"] == want_env and got["cornell_env_only"] == want_env
    assert got["mixed"] == dict(full="1", env="0", ml="0", nee="1", bins="1", lean="2", emit_filter="1",
                                **depths(5, False, filt_at=5))
    assert got["mixed_env"] == dict(full="1", env="1", ml="2", nee="1", bins="1", lean="2", emit_filter="0",
                                    **depths(5, True))
    assert got["mesh_env"]["ml"] == "3" and got["mesh_env"]["env"] == "1"
    # the reference integrator ignores the map: no path plan step carries it
    assert got["reference_env"]["env"] == "0" and got["reference_env"]["ml"] == "0"
    assert all(v[1] == "0" for k, v in got["reference_env"].items() if k.startswith("d"))
