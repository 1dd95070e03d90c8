// The decisions of one render pass as values: the knobs of the environment, the batch sizing the render and the feature
// pass share, and what the path pass does per pass (PathPlan) and per depth (DepthPlan).  Plain integer and boolean
// logic over a few scene facts: no HIP runtime call, no rt_ctx, so tests/test_pass_plan.py runs it on the CPU.  Each
// decision is defined here once; rt_host.cpp consumes the values.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdio>
#include <cstdlib>

#include "rt_internal.h"

namespace rtmi {

// Path mode keeps kLanes lanes so that consecutive batches run concurrently on separate streams: one batch's
// VALU-bound traversal overlaps the other's HBM-bound path-state traffic.
static const int kLanes = 4;
constexpr int kDefaultLanes = 2;   // path-mode batches in flight on separate streams (RTMI_LANES overrides; 1 lane:
                                   // Cornell 1217, 2 lanes 1500, 3-4 lanes with 4 Mi-sample batches ~1150 Msamples/s)

// The tuning and test knobs of the environment, with their defaults (INTEGRATION.md lists them): read once per
// context, and by rt_debug_bvh_build, so the exported and the uploaded BVHs come from the same parameters.
struct Knobs {
    bool stage_events = true;   // per-stage HIP events (rt_stats ms_*); RTMI_NO_STAGE_EVENTS=1 turns them off
    int lanes = kDefaultLanes;  // batches in flight in path mode (RTMI_LANES)
    // multi-level simple path scenes: NEE rays traced by k_path_shadow (RTMI_SHADOW_QUEUE=1; measured slower than
    // the inline any-hit, kept as a parity-tested option), depth first (RTMI_SHADOW_DFS, exact any-hit, §6)
    int shadow_queue = 0;
    int shadow_dfs = 1;
    int sort_rays = 1;         // RTMI_SORT=0: no coherence sort (A/B)
    float bvh_node_cost = 2.5f;  // SAH node cost relative to a triangle test (RTMI_BVH_CI; r04 with 64 bins: 2.5 vs 3 CFG3 +1.6 %, CFG4 +1.2 %)
    int bvh_max_leaf = kBvhMaxLeaf;  // triangles per BVH leaf at most (RTMI_BVH_LEAF)
    // the any-hit walks' BVH: its own (SAH node cost 2, leaves <= 4), or with RTMI_BVH_ANY="0/4" the closest-hit BVH
    // of set 0 itself (one working set for both queries).  r04 A/B: the shared BVH made CFG4's NEE stage 7.7 % slower
    // (30.0 vs 27.9 ms per step): the shadow rays' better tree outweighs the smaller working set
    float bvh_any_cost = 2.f;
    int bvh_any_leaf = 4;
    int force_amb = -1;        // RTMI_FORCE_AMB=k (test knob, DevScene amb_force / amb_mask): -1 off
    int coop = 1;              // RTMI_COOP=0 (test knob): undecided rays to the fallback kernels (DevScene coop_ok 0)
    int mat_bins = 1;          // RTMI_MAT_BINS=0: mixed multi-level scenes shade every material in one kernel (A/B)
    int emit_filter = 1;       // RTMI_EMIT_FILTER=0: the last depth of a mixed scene traces every ray (A/B)
    int debug_path = 0;        // RTMI_DEBUG_PATH_KERNELS=1 (tests): rt_debug_trace / _occluded run path mode's kernels
    int sort_dir_bits = 3, sort_org_bits = 3;  // sort key widths (RTMI_SORT_BITS="dir/org[/major]"; r03 A/B: 3/3 vs 3/4 CFG3 +1 %, 2/3 -4 %)
    // origin Morton code in the key's high bits (1) or the direction (0); -1: origin-major on the simple path, whose
    // shade kernel traces the NEE shadow rays inline (CFG3 588 -> 600), direction-major in mixed scenes, whose NEE
    // queue has a sort of its own (CFG4 372 vs 367)
    int sort_org_major = -1;
    // Morton sort of the NEE queue (mixed multi-level scenes; RTMI_SORT_NEE="on[/bits]"): CFG4 337 -> 364 at 9 bits
    // per axis (6 / 7 bits: 353 / 356; CFG5 334 -> 355 at 7)
    int sort_nee = 1, sort_nee_bits = 8;  // (r03, device radix sort: 8 bits = 3 passes, CFG4 +1.5 % over 9 bits = 4 passes)
    // single-leaf simple path, depths >= 1: the trace appends its hits to a dense hit queue and the shade runs only
    // those (TraceIO hq_d; Cornell +4.2 %, r07_ab4).  RTMI_HIT_COMPACT=0: every queue position is shaded (A/B)
    int hit_compact = 1;
    // the hit queue's records packed into one float4, (b0, b1, b2, slot | prim << 24 | facing << 30), the trace forming
    // the facing bit, face normals staged in LDS, and depth 0's hit word in hitB.w (rt_internal.h hit_pack, hit_pack0):
    // scenes of <= kHitPackTris triangles, batches of <= kHitPackSlots samples.  RTMI_HIT_PACK=0: unpacked (A/B, fallback)
    int hit_pack = 1;
    size_t batch_samples = 0;  // samples in flight per batch (0: 16 Mi single leaf, 32 Mi multi-level; RTMI_BATCH_SAMPLES)
    // denoiser iterations of step 1 and 2 stage their tile and halo in LDS (same bits; RTMI_DENOISE_LDS=0: every tap a
    // plain load, A/B in DESIGN.md §3c)
    int denoise_lds = 1;
};

inline Knobs read_knobs() {
    Knobs k;
    if (std::getenv("RTMI_NO_STAGE_EVENTS")) k.stage_events = false;
    if (const char* e = std::getenv("RTMI_LANES")) k.lanes = std::max(1, std::min(kLanes, std::atoi(e)));
    if (const char* e = std::getenv("RTMI_SHADOW_QUEUE")) k.shadow_queue = std::atoi(e);
    if (const char* e = std::getenv("RTMI_SHADOW_DFS")) k.shadow_dfs = std::atoi(e);
    if (const char* e = std::getenv("RTMI_SORT")) k.sort_rays = std::atoi(e);
    if (const char* e = std::getenv("RTMI_BVH_CI")) k.bvh_node_cost = (float)std::atof(e);
    if (const char* e = std::getenv("RTMI_BVH_LEAF")) k.bvh_max_leaf = std::max(1, std::min(15, std::atoi(e)));
    if (const char* e = std::getenv("RTMI_BVH_ANY")) {  // "cost/leaf": both fields, or the defaults stay
        float ac;
        int al;
        if (std::sscanf(e, "%f/%d", &ac, &al) == 2) {
            k.bvh_any_cost = ac;
            k.bvh_any_leaf = std::max(1, std::min(15, al));
        }
    }
    if (const char* e = std::getenv("RTMI_FORCE_AMB")) k.force_amb = std::max(-1, std::min(30, std::atoi(e)));
    if (const char* e = std::getenv("RTMI_COOP")) k.coop = std::atoi(e) != 0;
    if (const char* e = std::getenv("RTMI_MAT_BINS")) k.mat_bins = std::atoi(e);
    if (const char* e = std::getenv("RTMI_EMIT_FILTER")) k.emit_filter = std::atoi(e);
    if (const char* e = std::getenv("RTMI_DEBUG_PATH_KERNELS")) k.debug_path = std::atoi(e) != 0;
    if (const char* e = std::getenv("RTMI_SORT_BITS")) {
        int db = 3, ob = 4, om = -1;
        const int got = std::sscanf(e, "%d/%d/%d", &db, &ob, &om);
        // the key is 3 octant bits + 2 x db direction bits + 3 x ob origin bits in one u32, ob <= 9 (spread3_9)
        if (got >= 2 && db >= 0 && db <= 9 && ob >= 0 && ob <= 9 && 3 + 2 * db + 3 * ob <= 32) {
            k.sort_dir_bits = db;
            k.sort_org_bits = ob;
            if (got == 3) k.sort_org_major = om < 0 ? -1 : (om ? 1 : 0);
        }
    }
    if (const char* e = std::getenv("RTMI_SORT_NEE")) std::sscanf(e, "%d/%d", &k.sort_nee, &k.sort_nee_bits);
    k.sort_nee_bits = std::max(1, std::min(9, k.sort_nee_bits));
    if (const char* e = std::getenv("RTMI_HIT_COMPACT")) k.hit_compact = std::atoi(e) != 0;
    if (const char* e = std::getenv("RTMI_HIT_PACK")) k.hit_pack = std::atoi(e) != 0;
    if (const char* e = std::getenv("RTMI_BATCH_SAMPLES")) k.batch_samples = (size_t)std::max(0L, std::atol(e));
    if (const char* e = std::getenv("RTMI_DENOISE_LDS")) k.denoise_lds = std::atoi(e) != 0;
    return k;
}

// The facts a pass's decisions rest on: the uploaded scene (DevScene qcap, n_tris, n_lights, n_emit_tris, coop_ok; the
// upload's scene_full; live textures; a mesh light; a bound environment light, which DevScene n_lights counts), the
// integrator, and the pass's pixels and index range.
enum PassIntegrator { kIntegReference = 0, kIntegPath, kIntegPathMis };
struct PassFacts {
    int qcap = 0, n_tris = 0, n_lights = 0, n_emit_tris = -1, coop_ok = 0;
    bool scene_full = false;
    bool textures = false;
    bool mesh_light = false;
    bool environment = false;
    bool rough = false;        // a non-emissive RT_MAT_ROUGH material (it also makes the scene full)
    bool conductor = false;    // a non-emissive RT_MAT_CONDUCTOR material (it makes the scene full too)
    bool rough_dielectric = false;  // a non-emissive RT_MAT_ROUGH_DIELECTRIC material (§3m; it makes the scene full too)
    bool media = false;        // some bound medium has sigma > 0 (rt_scene_set_media, §3n; its material is a glass: full)
    PassIntegrator integ = kIntegReference;
    int max_depth = 0;
    int n_work = 0, ib = 0, ie = 0;
};

// The material bin of a material (DevMaterial cls, kMatClasses) by its rt_material type and whether it emits: 0 = the bin
// that reads spectra and writes NEE records (an emitter, Lambert 0, rough 3, conductor 4, rough glass 5), 1 = the specular
// bin (mirror 1, glass 2), whose kernels hold no RGH code.  rough_fact: the material makes the scene's `rough` fact (an
// emitter of type 3 does not); conductor_fact: its `conductor` fact (a non-emissive type 4 alone); rough_dielectric_fact:
// its `rough_dielectric` fact (a non-emissive type 5 alone).
inline int material_class(int type, bool emissive) {
    return emissive || type == 0 || type == 3 || type == 4 || type == 5 ? 0 : 1;
}
inline bool rough_dielectric_fact(int type, bool emissive) { return type == 5 && !emissive; }
inline bool rough_fact(int type, bool emissive) { return type == 3 && !emissive; }
inline bool conductor_fact(int type, bool emissive) { return type == 4 && !emissive; }

// Batch sizing and scene flags, shared by the render pass and the feature pass.
struct BatchPlan {
    bool path = false;   // a path integrator (the reference integrator otherwise)
    bool mis = false;    // DevScene mis of the pass's kernels: RT_INTEGRATOR_PATH_MIS
    bool full = false;   // DevScene full: path shading needs the general kernels
    int B = 0;           // sample indices per batch
    size_t nmax = 0;     // samples of the largest batch
    int nsh = 1;         // shards per queue
    size_t ncap = 0;     // queue / hit capacity: the shards of the largest batch (>= nmax)
    int nbatch = 0;      // batches of the pass (0: nothing to render)
    // bounce rays' traces.  Cornell-like single-leaf scenes cost the same per ray: static chunks on a resident grid
    // beat tickets there (A/B 1229 vs 1106-1158 Msamples/s); multi-level octrees vary per ray by 100x: tickets (CFG3
    // 71 -> 96)
    bool dyn = false;
    // multi-level octrees list their ambiguous rays for k_trace_fallback (the trace holds no BFS).  A ray is listed
    // only if the cooperative BFS's FIFO overflows, which the octree's exact queue bound excludes when coop_ok: then no
    // launch, which in two-lane mode would wait for the other lane's resident blocks (r05 kernel traces: 1.28 ms per
    // bounce)
    bool trace_fallback = false;
};

inline BatchPlan plan_batches(const PassFacts& f, const Knobs& kn) {
    BatchPlan p;
    p.path = f.integ != kIntegReference;
    p.mis = f.integ == kIntegPathMis;
    // (textures are fetched, and the environment light sampled, by the general kernels alone)
    p.full = f.scene_full || p.mis || f.textures || f.environment;
    p.nsh = f.qcap == 1 ? 1 : kShards;             // single-leaf scenes use one shard
    p.dyn = f.qcap != 1;
    p.trace_fallback = f.qcap != 1 && !f.coop_ok;
    if (f.ie <= f.ib || f.n_work <= 0) return p;
    // samples per batch: 16 Mi on a single-leaf octree (8 Mi: Cornell 1874 -> 1827; flat above 16 Mi, r06_ab7),
    // 32 Mi on multi-level ones, whose fewer, fuller launches keep more rays in every wave's reach (16 -> 32 Mi: CFG3
    // +2.5 %, CFG4 +3.5 %, flat above, r06_ab23/24)
    const size_t target = kn.batch_samples ? kn.batch_samples : (size_t)(f.qcap == 1 ? 16 : 32) << 20;
    p.B = (int)std::max<size_t>(1, target / (size_t)f.n_work);
    p.B = std::min(p.B, f.ie - f.ib);
    p.nmax = (size_t)p.B * f.n_work;
    p.ncap = (size_t)p.nsh * (size_t)shard_stride((int)p.nmax, p.nsh);
    p.nbatch = (f.ie - f.ib + p.B - 1) / p.B;
    return p;
}

// What varies with the depth of a bounce (PathPlan::at).
struct DepthPlan {
    bool traced = false;       // false: the pass stops before this depth
    bool efilter = false;      // k_emitter_filter ahead of the trace
    bool sort = false;         // coherence sort ahead of the trace
    bool next_keys = false;    // the shade writes the sort keys of the rays it appends (the next depth's sort)
    bool hit_compact = false;  // the trace appends its hits to the hit queue and the shade runs only those
    bool hit_pack = false;     // ... as packed records: one float4 each, hitD is neither allocated nor touched
    bool pack0 = false;        // depth 0 of a packing pass: the hit word in hitB's w lane
    bool trace_fallback = false, nee_fallback = false, shadow = false;  // the launches after the trace / NEE / shade
    // the environment light's miss stage (k_env_miss): after this depth's shade, which zero-initialises L
    // of the misses at lean depth 0, and before the next depth reuses the queue's hit and ray buffers
    bool env_miss = false;
    // the media's absorb stage (k_medium_absorb): between this depth's trace and its shade.  Never at depth
    // 0 (a camera ray's first segment is not attenuated; lean depth 0 holds beta = 1 in registers) and never on an
    // emitter-filtered depth, whose queue holds emitter hits only
    bool absorb = false;
};

// The path pass: computed once per pass.
struct PathPlan {
    // up to `lanes` batches in flight, batch k on lane k mod lanes
    int lanes = 1;
    // multi-level octrees: coherence-sort each bounce's rays (rt_sort.hip); on the single-leaf Cornell box the sort
    // costs more than it saves (1110 -> 720 Msamples/s)
    bool sort_rays = false;
    bool sort_nee = false;     // NEE vertices in Morton order of their shading points
    int org_major = 0;         // the sort key's major field, resolved (Knobs sort_org_major)
    // single-leaf simple path, bounce depths: hits compacted; packed while every slot of a batch fits the record's
    // 24-bit field and every triangle its 6-bit one.  Depth 0 keeps its dense queue: slot = position, and the lean
    // path writes L = 0 for the camera misses there.
    bool hit_compact = false, hit_pack = false;
    // k_generate stores no β = 1 / L = 0 / pdf streams: depth 0 starts from them in registers and the film recomputes
    // the pdf (simple path: +4.5 %).  1: the simple path (the host derives each depth's sampler dimension); 2: mixed
    // scenes, whose slots keep their dimension, prevPdf and TerminateSecondary flag in R_MISC (CFG4: k_generate
    // writes 96 instead of 192 B per sample)
    int lean = 1;
    // multi-level simple scenes: the NEE shadow rays the BVH alone cannot decide (defer 1) or, with
    // RTMI_SHADOW_QUEUE=1, all of them (defer 0) are queued and traced exactly by their own kernel
    bool shq = false;
    int defer = 0;
    // mixed scenes: NEE deferred to k_path_nee (one record per slot, one queue entry per Lambert vertex)
    bool nee = false;
    // mixed multi-level scenes: the trace kernel bins the hits by material class and each class is shaded by a kernel
    // holding only its materials' code (k_path_shade_full<Q, 1 / 2>)
    bool bins = false;
    // NeeIO ml: bit 0 the scene has a mesh light, bit 1 an environment light, bit 2 = rgh, bit 3 = cnd, bit 4 = rgl
    int ml = 0;
    // a rough material: the RGH instantiations of k_path_shade_full (classes 0 and 1) and k_path_nee,
    // whose NEE record is one float4 longer
    bool rgh = false;
    // a conductor material: RGH level 2 of the same kernels.  cnd implies rgh (a conductor vertex is a
    // rough vertex in its control flow); the NEE record also holds the lights' wo.h, four per float4 (nee_extra_f4)
    bool cnd = false;
    bool env = false;          // an environment light is bound: every traced depth ends with the miss stage
    // a rough-glass material: RGH level 3 of the same kernels, whatever else the scene holds.  rgl implies
    // rgh; the NEE record is level 2's (cnd stays the scene's own conductor fact)
    bool rgl = false;
    bool med = false;          // a medium with sigma > 0 is bound: depths >= 1 run the absorb stage
    // slot state layout (rt_internal.h RecView): records for multi-level scenes (sorted, scattered slots), SoA for
    // single-leaf ones (slots stay in queue order)
    bool records = false;
    size_t rec_fs = 0;
    unsigned rec_ss = 1;
    int rec_rng8 = 0;          // SoA simple path: dense 8-byte PCG states
    // what at() rests on
    int max_depth = 0;
    bool full = false, emit_filter = false, trace_fallback = false, nee_fallback = false, shadow = false;

    // the batch needs the (direction, prim) stream of unpacked hit records (Batch hitD)
    bool hit_d() const { return hit_compact && !hit_pack; }

    DepthPlan at(int depth) const {
        DepthPlan d;
        // the last trace can only add emitter hits, which count only after specular bounces or with MIS
        d.traced = depth <= max_depth && !(depth == max_depth && depth > 0 && !full);
        if (!d.traced) return d;
        // the last depth of a mixed scene: only emitter hits still add to L, so the rays that hit no emissive surface
        // are dropped first (k_emitter_filter); no coherence sort
        d.efilter = emit_filter && depth == max_depth && depth > 0;
        d.sort = sort_rays && depth > 0 && !d.efilter;
        d.next_keys = sort_rays && depth < max_depth;
        d.hit_compact = hit_compact && depth > 0;
        d.hit_pack = d.hit_compact && hit_pack;
        d.pack0 = hit_pack && depth == 0;
        d.trace_fallback = trace_fallback;
        d.nee_fallback = nee_fallback;
        d.shadow = shadow;
        d.env_miss = env;
        d.absorb = med && depth >= 1 && !d.efilter;
        return d;
    }
};

// the RGH level of the pass's kernels: 0 none, 1 rough, 2 rough and conductor, 3 those and rough glass (it sizes the NEE
// record: nee_extra_f4)
inline int rgh_level(const PathPlan& p) { return p.rgl ? 3 : p.cnd ? 2 : p.rgh ? 1 : 0; }

inline PathPlan plan_path(const PassFacts& f, const Knobs& kn, const BatchPlan& b) {
    PathPlan p;
    const bool multi = f.qcap != 1;
    p.lanes = std::max(1, std::min(std::min(kn.lanes, kLanes), b.nbatch));
    p.sort_rays = multi && kn.sort_rays;
    p.org_major = kn.sort_org_major >= 0 ? kn.sort_org_major : (b.full ? 0 : 1);
    p.hit_compact = kn.hit_compact && !multi && !b.full;
    p.hit_pack = kn.hit_pack && p.hit_compact && f.n_tris <= kHitPackTris && b.nmax <= (size_t)kHitPackSlots;
    p.lean = b.full ? 2 : 1;
    p.shq = multi && !b.full;
    p.defer = p.shq && !kn.shadow_queue ? 1 : 0;
    p.nee = b.full && f.n_lights > 0;
    p.sort_nee = p.nee && p.sort_rays && kn.sort_nee;
    p.bins = p.nee && multi && kn.mat_bins;
    p.env = f.environment && b.path;
    p.cnd = f.conductor && b.path;
    p.rgl = f.rough_dielectric && b.path;
    p.med = f.media && b.path;
    p.rgh = (f.rough && b.path) || p.cnd || p.rgl;
    p.ml = (f.mesh_light ? 1 : 0) | (p.env ? 2 : 0) | (p.rgh ? 4 : 0) | (p.cnd ? 8 : 0) | (p.rgl ? 16 : 0);
    p.records = multi;
    p.rec_fs = p.records ? 1 : b.nmax;
    p.rec_ss = p.records ? (unsigned)kRecF4 : 1u;
    p.rec_rng8 = !p.records && p.lean == 1 ? 1 : 0;
    p.max_depth = f.max_depth;
    p.full = b.full;
    // (with an environment light the rays that reach no emitter still add the map's radiance: no filter)
    p.emit_filter = kn.emit_filter && b.full && f.n_emit_tris >= 0 && !p.env;
    p.trace_fallback = b.trace_fallback;
    // (no launch either when k_path_nee resolves its undecided shadow rays itself, or k_path_shade the deferred ones,
    // coop_ok: in two-lane mode it waits for the other lane's resident blocks, r05 kernel traces: 0.87 ms per bounce)
    p.nee_fallback = p.nee && multi && !f.coop_ok;
    p.shadow = p.shq && !(p.defer && f.coop_ok);
    return p;
}

}  // namespace rtmi
