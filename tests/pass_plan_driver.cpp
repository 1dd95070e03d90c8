// Prints the pass plans of rt_pass_plan.h for the cases of tests/test_pass_plan.py.  Host only: no HIP library.
// Each argument is one case, "name:key=value,key=value,...": the keys are PassFacts' fields and, with a "k." prefix,
// Knobs' fields over read_knobs() of the environment.  Per case: a `batch` line, for a path integrator a `path` line
// and one `depth` line for every depth 0..max_depth.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../computational_ray_tracer_amd/csrc/rt_pass_plan.h"

using namespace rtmi;

static bool set_field(PassFacts& f, Knobs& k, const std::string& key, long v) {
    if (key == "qcap") f.qcap = (int)v;
    else if (key == "n_tris") f.n_tris = (int)v;
    else if (key == "n_lights") f.n_lights = (int)v;
    else if (key == "n_emit_tris") f.n_emit_tris = (int)v;
    else if (key == "coop_ok") f.coop_ok = (int)v;
    else if (key == "scene_full") f.scene_full = v != 0;
    else if (key == "textures") f.textures = v != 0;
    else if (key == "mesh_light") f.mesh_light = v != 0;
    else if (key == "integ") f.integ = (PassIntegrator)v;
    else if (key == "max_depth") f.max_depth = (int)v;
    else if (key == "n_work") f.n_work = (int)v;
    else if (key == "ib") f.ib = (int)v;
    else if (key == "ie") f.ie = (int)v;
    else if (key == "k.lanes") k.lanes = (int)v;
    else if (key == "k.shadow_queue") k.shadow_queue = (int)v;
    else if (key == "k.sort_rays") k.sort_rays = (int)v;
    else if (key == "k.sort_org_major") k.sort_org_major = (int)v;
    else if (key == "k.sort_nee") k.sort_nee = (int)v;
    else if (key == "k.mat_bins") k.mat_bins = (int)v;
    else if (key == "k.emit_filter") k.emit_filter = (int)v;
    else if (key == "k.hit_compact") k.hit_compact = (int)v;
    else if (key == "k.hit_pack") k.hit_pack = (int)v;
    else if (key == "k.batch_samples") k.batch_samples = (size_t)v;
    else return false;
    return true;
}

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        const std::string arg = argv[a];
        const size_t colon = arg.find(':');
        if (colon == std::string::npos) { std::fprintf(stderr, "bad case: %s\n", argv[a]); return 2; }
        PassFacts f;
        Knobs k = read_knobs();
        size_t pos = colon + 1;
        while (pos < arg.size()) {
            size_t end = arg.find(',', pos);
            if (end == std::string::npos) end = arg.size();
            const std::string kv = arg.substr(pos, end - pos);
            const size_t eq = kv.find('=');
            if (eq == std::string::npos || !set_field(f, k, kv.substr(0, eq), std::atol(kv.c_str() + eq + 1))) {
                std::fprintf(stderr, "bad field: %s\n", kv.c_str());
                return 2;
            }
            pos = end + 1;
        }
        const BatchPlan b = plan_batches(f, k);
        std::printf("case %s\n", arg.substr(0, colon).c_str());
        std::printf("batch path=%d mis=%d full=%d B=%d nmax=%zu nsh=%d ncap=%zu nbatch=%d dyn=%d trace_fallback=%d\n",
                    b.path, b.mis, b.full, b.B, b.nmax, b.nsh, b.ncap, b.nbatch, b.dyn, b.trace_fallback);
        if (!b.path) continue;
        const PathPlan p = plan_path(f, k, b);
        std::printf("path lanes=%d sort_rays=%d sort_nee=%d org_major=%d hit_compact=%d hit_pack=%d hit_d=%d lean=%d "
                    "shq=%d defer=%d nee=%d bins=%d ml=%d records=%d rec_fs=%zu rec_ss=%u rec_rng8=%d\n",
                    p.lanes, p.sort_rays, p.sort_nee, p.org_major, p.hit_compact, p.hit_pack, p.hit_d(), p.lean, p.shq,
                    p.defer, p.nee, p.bins, p.ml, p.records, p.rec_fs, p.rec_ss, p.rec_rng8);
        for (int depth = 0; depth <= f.max_depth; ++depth) {
            const DepthPlan d = p.at(depth);
            std::printf("depth %d traced=%d efilter=%d sort=%d next_keys=%d hit_compact=%d hit_pack=%d pack0=%d "
                        "trace_fallback=%d nee_fallback=%d shadow=%d\n",
                        depth, d.traced, d.efilter, d.sort, d.next_keys, d.hit_compact, d.hit_pack, d.pack0,
                        d.trace_fallback, d.nee_fallback, d.shadow);
        }
    }
    return 0;
}
