"""CPU: what a bound medium (rt_scene_set_media) changes in the render pass's plan (csrc/rt_pass_plan.h):
`med` follows the `media` fact under a path integrator, `absorb` is set at depths 1 .. max_depth, never at depth 0 and
never on an emitter-filtered depth, and every other decision is what it is without media.  A small program of its own
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
static void show(const char* name, bool multi, int integ, bool media, bool env, bool glass, int max_depth) {
    PassFacts f;
    f.qcap = multi ? 0 : 1; f.n_tris = multi ? 100000 : 36; f.n_lights = 2; f.n_emit_tris = 2; f.coop_ok = multi;
    f.scene_full = true;  // (a media-bearing material is a glass)
    f.environment = env; f.rough_dielectric = glass; f.media = media;
    f.integ = (PassIntegrator)integ; f.max_depth = max_depth; f.n_work = 1920 * 1080; f.ib = 0; f.ie = 16;
    const Knobs kn;
    const BatchPlan b = plan_batches(f, kn);
    const PathPlan p = plan_path(f, kn, b);
    std::printf("%s med=%d absorb=", name, (int)p.med);
    for (int d = 0; d <= max_depth + 1; ++d) std::printf("%d", (int)p.at(d).absorb);
    std::printf(" | path=%d mis=%d full=%d B=%d nsh=%d ncap=%zu nbatch=%d dyn=%d tfb=%d lanes=%d sort=%d sort_nee=%d org=%d "
                "hc=%d hp=%d lean=%d shq=%d defer=%d nee=%d bins=%d ml=%d rgh=%d cnd=%d env=%d rgl=%d records=%d fs=%zu ss=%u "
                "rng8=%d md=%d pfull=%d ef=%d ptfb=%d nfb=%d shadow=%d depths=", (int)b.path, (int)b.mis, (int)b.full, b.B,
                b.nsh, b.ncap, b.nbatch, (int)b.dyn, (int)b.trace_fallback, p.lanes, (int)p.sort_rays, (int)p.sort_nee,
                p.org_major, (int)p.hit_compact, (int)p.hit_pack, p.lean, (int)p.shq, p.defer, (int)p.nee, (int)p.bins, p.ml,
                (int)p.rgh, (int)p.cnd, (int)p.env, (int)p.rgl, (int)p.records, p.rec_fs, p.rec_ss, p.rec_rng8, p.max_depth,
                (int)p.full, (int)p.emit_filter, (int)p.trace_fallback, (int)p.nee_fallback, (int)p.shadow);
    for (int d = 0; d <= max_depth + 1; ++d) {
        const DepthPlan q = p.at(d);
        std::printf("[%d%d%d%d%d%d%d%d%d%d%d]", (int)q.traced, (int)q.efilter, (int)q.sort, (int)q.next_keys,
                    (int)q.hit_compact, (int)q.hit_pack, (int)q.pack0, (int)q.trace_fallback, (int)q.nee_fallback,
                    (int)q.shadow, (int)q.env_miss);
    }
    std::printf("\n");
}
int main() {
    for (int multi = 0; multi < 2; ++multi)
        for (int media = 0; media < 2; ++media) {
            char name[32];
            std::snprintf(name, sizeof name, "%s_path_%d", multi ? "m" : "s", media);
            show(name, multi, kIntegPath, media, false, false, 5);
            std::snprintf(name, sizeof name, "%s_mis_%d", multi ? "m" : "s", media);
            show(name, multi, kIntegPathMis, media, false, true, 3);
            std::snprintf(name, sizeof name, "%s_env_%d", multi ? "m" : "s", media);
            show(name, multi, kIntegPathMis, media, true, true, 5);
            std::snprintf(name, sizeof name, "%s_ref_%d", multi ? "m" : "s", media);
            show(name, multi, kIntegReference, media, false, false, 5);
            std::snprintf(name, sizeof name, "%s_d1_%d", multi ? "m" : "s", media);
            show(name, multi, kIntegPath, media, false, false, 1);
        }
    const PathPlan d;
    std::printf("defaults %d %d\n", (int)d.med, (int)d.at(1).absorb);
    return 0;
}
"""


def test_media_in_the_pass_plan(tmp_path):
    src = tmp_path / "medium_plan.cpp"
    src.write_text(SOURCE)
    exe = tmp_path / "medium_plan"
    r = subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I" + HIP_INCLUDE,
                        "-I" + str(ROOT / "computational_ray_tracer_amd" / "csrc"), "-o", str(exe), str(src)],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith("RTMI_")}
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, env=env)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.splitlines()
    got = {l.split()[0]: (l.split(" | ")[0].split()[1:], l.split(" | ")[1]) for l in lines if " | " in l}
    for pre in ("s", "m"):
        # without media: never
        for v in ("path", "mis", "env", "ref", "d1"):
            head = got[f"{pre}_{v}_0"][0]
            assert head[0] == "med=0" and set(head[1].split("=")[1]) == {"0"}, (pre, v, head)
        # the emitter filter runs on the last depth of a scene with lights and no environment: depths 1 .. max_depth - 1
        # absorb, depth 0 and the filtered depth max_depth do not (one entry past max_depth: not traced)
        assert got[f"{pre}_path_1"][0] == ["med=1", "absorb=0111100"]
        assert got[f"{pre}_mis_1"][0] == ["med=1", "absorb=01100"]
        assert "ef=1" in got[f"{pre}_path_1"][1] and "ef=1" in got[f"{pre}_mis_1"][1]
        # an environment light switches the filter off: depths 1 .. max_depth absorb
        assert got[f"{pre}_env_1"][0] == ["med=1", "absorb=0111110"]
        assert "ef=0" in got[f"{pre}_env_1"][1]
        # max_depth 1 with the filter: depth 1 is the filtered one
        assert got[f"{pre}_d1_1"][0] == ["med=1", "absorb=000"]
        # the reference integrator ignores media
        assert got[f"{pre}_ref_1"][0] == ["med=0", "absorb=0000000"]
        # every other field of BatchPlan, PathPlan and DepthPlan is equal with and without media
        for v in ("path", "mis", "env", "ref", "d1"):
            assert got[f"{pre}_{v}_1"][1] == got[f"{pre}_{v}_0"][1], (pre, v)
    assert "defaults 0 0" in lines


def test_the_printed_fields_are_all_of_them():
    """The program above prints every field of PathPlan and DepthPlan: a field added to either must be added there."""
    import re
    text = (ROOT / "computational_ray_tracer_amd" / "csrc" / "rt_pass_plan.h").read_text()

    def fields(struct):
        body = text.split(f"struct {struct} {{")[1].split("\n};")[0]
        body = re.sub(r"//[^\n]*", "", body)
        body = body.split("bool hit_d()")[0] if struct == "PathPlan" else body
        names = []
        for decl in re.findall(r"^\s*(?:bool|int|size_t|unsigned)\s+([^;()]+);", body, re.M):
            names += [re.sub(r"\s*=.*", "", p).strip() for p in re.split(r",(?![^{]*})", decl)]
        return names
    assert len(fields("DepthPlan")) == 12, fields("DepthPlan")       # 11 printed + absorb
    assert len(fields("PathPlan")) == 27, fields("PathPlan")         # 26 printed after the bar + med
