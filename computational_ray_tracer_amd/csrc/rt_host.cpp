// librtmi355x — host side of the drop-in C-ABI (include/rtmi355x.h).
//
// Owns: the HIP context/stream, the scene preparation the reference does on the host before its render loop
// (TriModel world transform + back-face flags, Shapes.h:1282-1380; Octtree_Model::CreateOcttree with the
// Möller overlap test, Octtree_Model.h:33-63/180-367, AABB_triangle_Moller.h:187-474; Spectra::Init,
// spectrum.cpp:2612-2634), the flattening of that octree into the HBM layout of rt_internal.h, and the
// orchestration of the wavefront kernels of rt_kernels.hip for one render pass.
//
// There is no CPU fallback: every pass runs on the MI355X; rt_create fails without a gfx950 device.
#include <algorithm>
#include <cstddef>
#include <cstdlib>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <limits>
#include <queue>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/rtmi355x.h"
#include "../data/spectra_data.h"
#include "../data/sensor_data.h"
#include "rt_cull.h"
#include "rt_devbuf.h"
#include "rt_guard.h"
#include "rt_internal.h"
#include "rt_pass_plan.h"
#include "rt_envmap.h"
#include "rt_fresnel.h"
#include "rt_ggx.h"
#include "rt_roughglass.h"
#include "rt_texture.h"

using namespace rtmi;

namespace {

constexpr int kRingMax = 1 << 16;  // largest BFS group FIFO (HBM ring per resident thread, 4 B per entry)
constexpr int kMaxLights = 64;
constexpr float kClusterPadRel = 1e-5f;  // cluster-box inflation per unit of scene extent (see scene upload)
constexpr float kClusterPadCentre = 0x1p-22f;  // ... and per unit of the scene centre's largest |coordinate| (RT_CULL_FMA)

// ------------------------------------------------------------------------------ host float math
// glm operation order, float, -ffp-contract=off (same contract as the device code)
struct F3 { float x, y, z; float operator[](int i) const { return i == 0 ? x : (i == 1 ? y : z); } };
inline F3 f3add(F3 a, F3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline F3 f3sub(F3 a, F3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline F3 f3mul(F3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
inline float f3dot(F3 a, F3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
inline F3 f3cross(F3 a, F3 b) { return {a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; }
inline F3 f3norm(F3 v) { float s = 1.0f / std::sqrt(f3dot(v, v)); return f3mul(v, s); }
inline void m4v(const float* M, float x, float y, float z, float w, float o[4]) {
    for (int r = 0; r < 4; ++r) {
        float a0 = M[0 * 4 + r] * x, a1 = M[1 * 4 + r] * y, a2 = M[2 * 4 + r] * z, a3 = M[3 * 4 + r] * w;
        o[r] = (a0 + a1) + (a2 + a3);
    }
}
// The render-space bounding sphere of an analytic shape for the kernels' conservative cull (rt_device.h
// shape_culled): the object-space box of the shape (sphere: [-r, r]^2 x [zmin, zmax]; disk: [-ro, ro]^2 x {h};
// triangle: its vertices' box) through the inverse of render_to_object — the transform the exact test applies — in
// double, then centre = the box centre, radius = its half diagonal, padded by 1e-3 relative and 1e-3 (1 + |centre|)
// absolute.  A singular transform or a non-finite result disables the cull for the shape (bs[3] = inf).
void shape_bound(DevShape& d) {
    double a[4][8];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) { a[r][c] = d.r2o[c * 4 + r]; a[r][4 + c] = r == c ? 1.0 : 0.0; }
    bool ok = true;
    for (int c = 0; c < 4 && ok; ++c) {  // Gauss-Jordan with partial pivoting
        int pr = c;
        for (int r = c + 1; r < 4; ++r) if (std::fabs(a[r][c]) > std::fabs(a[pr][c])) pr = r;
        if (!(std::fabs(a[pr][c]) > 1e-30)) { ok = false; break; }
        for (int k = 0; k < 8; ++k) std::swap(a[c][k], a[pr][k]);
        const double iv = 1.0 / a[c][c];
        for (int k = 0; k < 8; ++k) a[c][k] *= iv;
        for (int r = 0; r < 4; ++r)
            if (r != c) { const double f = a[r][c]; for (int k = 0; k < 8; ++k) a[r][k] -= f * a[c][k]; }
    }
    double lo[3], hi[3];
    if (d.type == 0) { lo[0] = lo[1] = -d.r; hi[0] = hi[1] = d.r; lo[2] = d.zmin; hi[2] = d.zmax; }
    else if (d.type == 1) { lo[0] = lo[1] = -d.ro; hi[0] = hi[1] = d.ro; lo[2] = hi[2] = d.h; }
    else {
        for (int k = 0; k < 3; ++k) {
            lo[k] = std::min(std::min(d.p1[k], d.p2[k]), d.p3[k]);
            hi[k] = std::max(std::max(d.p1[k], d.p2[k]), d.p3[k]);
        }
    }
    double wlo[3] = {1e300, 1e300, 1e300}, whi[3] = {-1e300, -1e300, -1e300};
    for (int corner = 0; corner < 8 && ok; ++corner) {
        const double p[3] = {(corner & 1) ? hi[0] : lo[0], (corner & 2) ? hi[1] : lo[1], (corner & 4) ? hi[2] : lo[2]};
        for (int r = 0; r < 3; ++r) {
            const double w = a[r][4] * p[0] + a[r][5] * p[1] + a[r][6] * p[2] + a[r][7];
            wlo[r] = std::min(wlo[r], w);
            whi[r] = std::max(whi[r], w);
        }
    }
    double c[3], h2 = 0.0, cm = 0.0;
    for (int r = 0; r < 3; ++r) {
        c[r] = 0.5 * (wlo[r] + whi[r]);
        h2 += 0.25 * (whi[r] - wlo[r]) * (whi[r] - wlo[r]);
        cm = std::max(cm, std::fabs(c[r]));
    }
    const double rp = std::sqrt(h2) * 1.001 + 1e-3 * (1.0 + cm);
    for (int r = 0; r < 3; ++r) d.bs[r] = (float)c[r];
    d.bs[3] = (float)(rp * rp);
    if (!ok || !std::isfinite(d.bs[0]) || !std::isfinite(d.bs[1]) || !std::isfinite(d.bs[2]) || !std::isfinite(d.bs[3]))
        d.bs[3] = std::numeric_limits<float>::infinity();
}
inline F3 m3v(const float* M, F3 v) {
    float o[3];
    for (int r = 0; r < 3; ++r) o[r] = (M[0 * 3 + r] * v.x + M[1 * 3 + r] * v.y) + M[2 * 3 + r] * v.z;
    return {o[0], o[1], o[2]};
}

// ---------------------------------------------------------------------------------- spectra (host)
// spectrum.cpp:60-71 PiecewiseLinearSpectrum::Query with helpers.h:159-172 FindInterval
struct PLS {
    std::vector<float> l, v;
    float query(float lambda) const {
        if (l.empty() || lambda < l.front() || lambda > l.back()) return 0;
        long size = (long)l.size() - 2, first = 1;
        while (size > 0) {
            long half = size >> 1, middle = first + half;
            bool r = l[middle] <= lambda;
            first = r ? middle + 1 : first;
            size = r ? size - (half + 1) : half;
        }
        long o = std::min(std::max(first - 1, 0L), (long)l.size() - 2);
        float t = (lambda - l[o]) / (l[o + 1] - l[o]);
        return (1 - t) * v[o] + t * v[o + 1];
    }
};
struct DenseS {
    std::vector<float> v;  // 360..830
    float query(float lambda) const {
        long off = std::lround(lambda) - 360;
        return (off < 0 || off >= (long)v.size()) ? 0.f : v[off];
    }
};
template <class S>
DenseS to_dense(const S& s) {
    DenseS d;
    d.v.resize(kSpecN);
    for (int l = 360; l <= 830; ++l) d.v[l - 360] = s.query((float)l);
    return d;
}
template <class A, class B>
float inner_product(const A& f, const B& g) {  // spectrum.h:762-768
    float acc = 0;
    for (float lambda = 360; lambda <= 830; ++lambda) acc += f.query(lambda) * g.query(lambda);
    return acc;
}
// The metals' dense (n, k) table NK[4][471] (rt_fresnel.h), built once per process from the measured
// tables; every context uploads its copy (create_one) and rt_metal_nk reads this one.
static const std::vector<float>& metal_nk_table() {
    static const std::vector<float> t = [] {
        std::vector<float> v(2 * (size_t)kMetals * kMetalSpecN);
        const float* eta[kMetals] = {rtdata::metal_ag_eta, rtdata::metal_al_eta, rtdata::metal_au_eta, rtdata::metal_cu_eta};
        const float* kk[kMetals] = {rtdata::metal_ag_k, rtdata::metal_al_k, rtdata::metal_au_k, rtdata::metal_cu_k};
        const int en[kMetals] = {rtdata::metal_ag_eta_n, rtdata::metal_al_eta_n, rtdata::metal_au_eta_n, rtdata::metal_cu_eta_n};
        const int kn[kMetals] = {rtdata::metal_ag_k_n, rtdata::metal_al_k_n, rtdata::metal_au_k_n, rtdata::metal_cu_k_n};
        for (int m = 0; m < kMetals; ++m) metal_nk_build(eta[m], en[m], kk[m], kn[m], v.data() + 2 * (size_t)m * kMetalSpecN);
        return v;
    }();
    return t;
}
struct HostSpectra {
    DenseS X, Y, Z, D65d;
    PLS D65, F1, BK7;
    PLS interleaved(const float* s, int n, bool normalize) const {  // spectrum.cpp:134-165 FromInterleaved
        PLS p;
        if (s[0] > 360) { p.l.push_back(359); p.v.push_back(s[1]); }
        for (int i = 0; i < n / 2; ++i) { p.l.push_back(s[2 * i]); p.v.push_back(s[2 * i + 1]); }
        if (p.l.back() < 830) { p.l.push_back(831); p.v.push_back(p.v.back()); }
        if (normalize) {
            float sc = 106.856895f / inner_product(p, Y);
            for (float& x : p.v) x *= sc;
        }
        return p;
    }
    void init() {
        auto cie = [](const float* t) {
            PLS p;
            p.l.assign(rtdata::cie_lambda, rtdata::cie_lambda + 471);
            p.v.assign(t, t + 471);
            return to_dense(p);
        };
        X = cie(rtdata::cie_x); Y = cie(rtdata::cie_y); Z = cie(rtdata::cie_z);
        D65 = interleaved(rtdata::illum_d65, rtdata::illum_d65_n, true);
        F1 = interleaved(rtdata::illum_f1, rtdata::illum_f1_n, true);
        BK7 = interleaved(rtdata::glass_bk7_eta, rtdata::glass_bk7_eta_n, false);  // spectrum.cpp:2674-2675
        D65d = to_dense(D65);
    }
};

// ------------------------------------------------------------------ Möller triangle / box overlap (host)
// AABB_triangle_Moller.h:187-474 (AxisTest_Z0 never rejects: the quirk at :342 is kept)
bool axis_ok(float pa, float pb, float rad) {
    float mn, mx;
    if (pa < pb) { mn = pa; mx = pb; } else { mn = pb; mx = pa; }
    return !(mn > rad || mx < -rad);
}
bool axis_ok_z12(float p1, float p2, float rad) {
    float mn, mx;
    if (p2 < p1) { mn = p2; mx = p1; } else { mn = p1; mx = p2; }
    return !(mn > rad || mx < -rad);
}
bool tri_box_overlap(F3 c, F3 h, F3 t0, F3 t1, F3 t2) {
    F3 v0 = f3sub(t0, c), v1 = f3sub(t1, c), v2 = f3sub(t2, c);
    F3 e0 = f3sub(v1, v0), e1 = f3sub(v2, v1), e2 = f3sub(v0, v2);
    float fex, fey, fez;
    fex = std::fabs(e0.x); fey = std::fabs(e0.y); fez = std::fabs(e0.z);
    if (!axis_ok(e0.z * v0.y - e0.y * v0.z, e0.z * v2.y - e0.y * v2.z, fez * h.y + fey * h.z)) return false;   // X01
    if (!axis_ok(-e0.z * v0.x + e0.x * v0.z, -e0.z * v2.x + e0.x * v2.z, fez * h.x + fex * h.z)) return false; // Y02
    if (!axis_ok_z12(e0.y * v1.x - e0.x * v1.y, e0.y * v2.x - e0.x * v2.y, fey * h.x + fex * h.y)) return false; // Z12
    fex = std::fabs(e1.x); fey = std::fabs(e1.y); fez = std::fabs(e1.z);
    if (!axis_ok(e1.z * v0.y - e1.y * v0.z, e1.z * v2.y - e1.y * v2.z, fez * h.y + fey * h.z)) return false;   // X01
    if (!axis_ok(-e1.z * v0.x + e1.x * v0.z, -e1.z * v2.x + e1.x * v2.z, fez * h.x + fex * h.z)) return false; // Y02
    // Z0: never rejects (reference returns true on both paths)
    fex = std::fabs(e2.x); fey = std::fabs(e2.y); fez = std::fabs(e2.z);
    if (!axis_ok(e2.z * v0.y - e2.y * v0.z, e2.z * v1.y - e2.y * v1.z, fez * h.y + fey * h.z)) return false;   // X2
    if (!axis_ok(-e2.z * v0.x + e2.x * v0.z, -e2.z * v1.x + e2.x * v1.z, fez * h.x + fex * h.z)) return false; // Y1
    if (!axis_ok_z12(e2.y * v1.x - e2.x * v1.y, e2.y * v2.x - e2.x * v2.y, fey * h.x + fex * h.y)) return false; // Z12
    auto mm = [](float a, float b, float c, float& mn, float& mx) {
        mn = mx = a;
        if (b < mn) mn = b;
        if (b > mx) mx = b;
        if (c < mn) mn = c;
        if (c > mx) mx = c;
    };
    float mn, mx;
    mm(v0.x, v1.x, v2.x, mn, mx);
    if (mn > h.x || mx < -h.x) return false;
    mm(v0.y, v1.y, v2.y, mn, mx);
    if (mn > h.y || mx < -h.y) return false;
    mm(v0.z, v1.z, v2.z, mn, mx);
    if (mn > h.z || mx < -h.z) return false;
    F3 nrm = f3cross(e0, e1);  // planeBoxOverlap
    float vmin[3], vmax[3];
    for (int q = 0; q < 3; ++q) {
        float v = v0[q], nq = nrm[q], mb = h[q];
        if (nq > 0.0f) { vmin[q] = -mb - v; vmax[q] = mb - v; }
        else { vmin[q] = mb - v; vmax[q] = -mb - v; }
    }
    if (f3dot(nrm, {vmin[0], vmin[1], vmin[2]}) > 0.0f) return false;
    if (f3dot(nrm, {vmax[0], vmax[1], vmax[2]}) >= 0.0f) return true;
    return false;
}

// ------------------------------------------------------------------------------- octree builder
// Octtree_Model.h:33-63 CreateOcttree, 180-277 AddTriangle, 279-358 Split, 361-367 tri_boundsIntersection
struct OctBuild {
    struct Node { F3 mn, mx; int first_child = -1; std::vector<int> tris; };
    std::vector<Node> nodes;
    const std::vector<F3>* tri3 = nullptr;  // 3 world vertices per triangle
    int capacity = 40;

    bool overlap(int t, const Node& n) const {
        F3 half = {(n.mx.x - n.mn.x) / 2.0f, (n.mx.y - n.mn.y) / 2.0f, (n.mx.z - n.mn.z) / 2.0f};
        F3 c = f3add(n.mn, half);
        const F3* p = &(*tri3)[3 * (size_t)t];
        return tri_box_overlap(c, half, p[0], p[1], p[2]);
    }
    // the 8 padded child boxes of a node (Octtree_Model.h:279-300): top fl, fr, bl, br, bottom fl, fr, bl, br
    static void child_boxes(F3 mn, F3 mx, F3 cmn[8], F3 cmx[8]) {
        F3 h = {(mx.x - mn.x) / 2.0f, (mx.y - mn.y) / 2.0f, (mx.z - mn.z) / 2.0f};
        F3 C = f3add(mn, h);
        h = f3add(h, {0.01f, 0.01f, 0.01f});
        const F3 lo[8] = {{-h.x, 0, -h.z}, {0, 0, -h.z}, {-h.x, 0, 0}, {0, 0, 0},
                          {-h.x, -h.y, -h.z}, {0, -h.y, -h.z}, {-h.x, -h.y, 0}, {0, -h.y, 0}};
        const F3 hi[8] = {{0, h.y, 0}, {h.x, h.y, 0}, {0, h.y, h.z}, {h.x, h.y, h.z},
                          {0, 0, 0}, {h.x, 0, 0}, {0, 0, h.z}, {h.x, 0, h.z}};
        for (int k = 0; k < 8; ++k) { cmn[k] = f3add(C, lo[k]); cmx[k] = f3add(C, hi[k]); }
    }
    void split(int id) {
        Node ch[8];
        {
            F3 cmn[8], cmx[8];
            child_boxes(nodes[id].mn, nodes[id].mx, cmn, cmx);
            for (int k = 0; k < 8; ++k) { ch[k].mn = cmn[k]; ch[k].mx = cmx[k]; }
        }
        for (int t : nodes[id].tris)
            for (int k = 0; k < 8; ++k)
                if (overlap(t, ch[k])) ch[k].tris.push_back(t);
        size_t cnt = nodes[id].tris.size();
        for (int k = 0; k < 8; ++k)
            if (ch[k].tris.size() == cnt) return;  // abort rule (Octtree_Model.h:331-340)
        int first = (int)nodes.size();
        for (int k = 0; k < 8; ++k) nodes.push_back(std::move(ch[k]));
        nodes[id].first_child = first;
        nodes[id].tris.clear();
        nodes[id].tris.shrink_to_fit();
    }
    void add(int t) {
        std::queue<int> q;
        q.push(0);
        while (!q.empty()) {
            int cur = q.front();
            q.pop();
            if (!overlap(t, nodes[cur])) continue;
            if (nodes[cur].first_child < 0) {
                nodes[cur].tris.push_back(t);
                if ((int)nodes[cur].tris.size() >= capacity) split(cur);
            } else {
                for (int k = 0; k < 8; ++k) q.push(nodes[cur].first_child + k);
            }
        }
    }
};

// On-device build of the same tree (rt_octree.hip: the level-synchronous form of the sequential insertion).  The
// device classifies and scatters each level; the host decides the splits (k = max(capacity, s0 + 1, M + 1) <= len),
// lays out the next level in BFS order and at the end renumbers the nodes in the order the sequential build
// creates them: by the triangle whose insertion triggered the split, then BFS order within that insertion.
int octree_build_device(hipStream_t st, OctBuild& ob, int nt, std::string& err) {
    struct LNode {
        F3 mn, mx;
        int begin, len, s0, level;
        int first_child = -1, trigger = -1;
    };
    auto ok = [&](hipError_t e, const char* what) {
        if (e != hipSuccess) err = std::string("octree build: ") + what + ": " + hipGetErrorString(e);
        return e == hipSuccess;
    };
    const std::vector<F3>& tri3 = *ob.tri3;
    DevBuf<float> d_tri9, d_cbox;
    DevBuf<int> d_ent, d_next, d_seg, d_stats, d_job, d_s0;
    DevBuf<unsigned char> d_mask;  // one mask byte per entry of the largest level
    if (!ok(d_tri9.reserve(3 * tri3.size()), "alloc") ||
        !ok(hipMemcpyAsync(d_tri9.get(), tri3.data(), sizeof(F3) * tri3.size(), hipMemcpyHostToDevice, st), "upload"))
        return RT_E_HIP;
    // the per-node arrays of a level of n nodes: child boxes, segments, statistics, scatter jobs, s0
    auto reserve_nodes = [&](size_t n) {
        return ok(d_cbox.reserve(48 * n), "alloc") && ok(d_seg.reserve(2 * n), "alloc") &&
               ok(d_stats.reserve(9 * n), "alloc") && ok(d_job.reserve(12 * n), "alloc") && ok(d_s0.reserve(8 * n), "alloc");
    };
    // root pass: A_root = the triangles overlapping the root box, in insertion order
    std::vector<int> iota(nt);
    for (int t = 0; t < nt; ++t) iota[t] = t;
    if (!ok(d_ent.reserve(nt), "alloc") || !ok(d_next.reserve(nt), "alloc") || !ok(d_mask.reserve(nt), "alloc") ||
        !reserve_nodes(1))
        return RT_E_OOM;
    {
        float box[48];
        const F3 rmn = ob.nodes[0].mn, rmx = ob.nodes[0].mx;
        for (int k = 0; k < 8; ++k) {
            box[6 * k] = rmn.x; box[6 * k + 1] = rmn.y; box[6 * k + 2] = rmn.z;
            box[6 * k + 3] = rmx.x; box[6 * k + 4] = rmx.y; box[6 * k + 5] = rmx.z;
        }
        int seg[2] = {0, nt}, job[12] = {0, nt, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, stats[9];
        if (!ok(hipMemcpyAsync(d_ent.get(), iota.data(), 4 * (size_t)nt, hipMemcpyHostToDevice, st), "upload") ||
            !ok(hipMemcpyAsync(d_cbox.get(), box, sizeof(box), hipMemcpyHostToDevice, st), "upload") ||
            !ok(hipMemcpyAsync(d_seg.get(), seg, sizeof(seg), hipMemcpyHostToDevice, st), "upload") ||
            !ok(hipMemcpyAsync(d_job.get(), job, sizeof(job), hipMemcpyHostToDevice, st), "upload") ||
            !ok(launch_oct_classify(st, 1, d_cbox.get(), d_seg.get(), d_ent.get(), d_tri9.get(), d_mask.get(),
                                    d_stats.get()), "classify") ||
            !ok(launch_oct_scatter(st, 1, 1, d_job.get(), d_ent.get(), d_mask.get(), d_next.get(), d_s0.get()),
                "scatter") ||
            !ok(hipMemcpyAsync(stats, d_stats.get(), sizeof(stats), hipMemcpyDeviceToHost, st), "download") ||
            !ok(hipStreamSynchronize(st), "sync"))
            return RT_E_HIP;
        std::swap(d_ent, d_next);
        LNode root{rmn, rmx, 0, stats[1], 0, 0};
        ob.nodes.clear();
        std::vector<LNode> all{root};
        std::vector<std::vector<int>> level_ents;
        std::vector<int> frontier{0};
        while (!frontier.empty()) {
            const int n = (int)frontier.size();
            std::vector<float> cbox(48 * (size_t)n);
            std::vector<int> segs(2 * (size_t)n);
            int total = 0;
            for (int i = 0; i < n; ++i) {
                const LNode& N = all[frontier[i]];
                F3 cmn[8], cmx[8];
                OctBuild::child_boxes(N.mn, N.mx, cmn, cmx);
                for (int k = 0; k < 8; ++k) {
                    float* q = &cbox[48 * (size_t)i + 6 * k];
                    q[0] = cmn[k].x; q[1] = cmn[k].y; q[2] = cmn[k].z; q[3] = cmx[k].x; q[4] = cmx[k].y; q[5] = cmx[k].z;
                }
                segs[2 * i] = N.begin; segs[2 * i + 1] = N.len;
                total = std::max(total, N.begin + N.len);
            }
            // buffers that are too small are replaced by ones of twice the size needed
            if ((size_t)n > d_seg.capacity() / 2 && !reserve_nodes(2 * (size_t)n)) return RT_E_OOM;
            if ((size_t)total > d_mask.capacity() && !ok(d_mask.reserve(2 * (size_t)total), "alloc")) return RT_E_OOM;
            std::vector<int> stats(9 * (size_t)n);
            level_ents.emplace_back((size_t)total);
            if (!ok(hipMemcpyAsync(d_cbox.get(), cbox.data(), 4 * cbox.size(), hipMemcpyHostToDevice, st), "upload") ||
                !ok(hipMemcpyAsync(d_seg.get(), segs.data(), 4 * segs.size(), hipMemcpyHostToDevice, st), "upload") ||
                !ok(launch_oct_classify(st, n, d_cbox.get(), d_seg.get(), d_ent.get(), d_tri9.get(), d_mask.get(),
                                        d_stats.get()), "classify") ||
                !ok(hipMemcpyAsync(stats.data(), d_stats.get(), 4 * stats.size(), hipMemcpyDeviceToHost, st),
                    "download") ||
                !ok(hipMemcpyAsync(level_ents.back().data(), d_ent.get(), 4 * (size_t)total, hipMemcpyDeviceToHost, st),
                    "download") ||
                !ok(hipStreamSynchronize(st), "sync"))
                return RT_E_HIP;
            // splits, in frontier (BFS) order; children laid out contiguously in the next level's sequence array
            std::vector<int> jobs, next_frontier;
            int running = 0;
            for (int i = 0; i < n; ++i) {
                LNode& N = all[frontier[i]];
                const int* S = &stats[9 * (size_t)i];
                int k = std::max(std::max(ob.capacity, N.s0 + 1), S[0] + 1);
                if (k > N.len) continue;
                N.trigger = level_ents.back()[(size_t)N.begin + k - 1];
                N.first_child = (int)all.size();
                int job[12] = {N.begin, N.len, k, 0, 0, 0, 0, 0, 0, 0, 0, 0};
                F3 cmn[8], cmx[8];
                OctBuild::child_boxes(N.mn, N.mx, cmn, cmx);
                const int lvl = N.level;
                for (int c = 0; c < 8; ++c) {
                    job[3 + c] = running;
                    all.push_back(LNode{cmn[c], cmx[c], running, S[1 + c], 0, lvl + 1});
                    next_frontier.push_back((int)all.size() - 1);
                    running += S[1 + c];
                }
                jobs.insert(jobs.end(), job, job + 12);
            }
            if (jobs.empty()) break;
            const int nj = (int)jobs.size() / 12;
            if ((size_t)running > d_next.capacity() && !ok(d_next.reserve(2 * (size_t)running), "alloc")) return RT_E_OOM;
            std::vector<int> s0(8 * (size_t)nj);
            if (!ok(hipMemcpyAsync(d_job.get(), jobs.data(), 4 * jobs.size(), hipMemcpyHostToDevice, st), "upload") ||
                !ok(launch_oct_scatter(st, nj, 8, d_job.get(), d_ent.get(), d_mask.get(), d_next.get(), d_s0.get()),
                    "scatter") ||
                !ok(hipMemcpyAsync(s0.data(), d_s0.get(), 4 * s0.size(), hipMemcpyDeviceToHost, st), "download") ||
                !ok(hipStreamSynchronize(st), "sync"))
                return RT_E_HIP;
            for (int j = 0; j < nj; ++j)
                for (int c = 0; c < 8; ++c) all[next_frontier[8 * j + c]].s0 = s0[8 * (size_t)j + c];
            std::swap(d_ent, d_next);
            frontier.swap(next_frontier);
        }
        // renumber: the sequential build appends a split node's 8 children when its trigger triangle is inserted
        std::vector<int> splits;
        for (int i = 0; i < (int)all.size(); ++i)
            if (all[i].first_child >= 0) splits.push_back(i);
        std::stable_sort(splits.begin(), splits.end(), [&](int a, int b) { return all[a].trigger < all[b].trigger; });
        std::vector<int> seq(all.size(), -1);
        seq[0] = 0;
        for (size_t r = 0; r < splits.size(); ++r)
            for (int c = 0; c < 8; ++c) seq[all[splits[r]].first_child + c] = 1 + 8 * (int)r + c;
        ob.nodes.assign(all.size(), OctBuild::Node{});
        for (int i = 0; i < (int)all.size(); ++i) {
            const LNode& N = all[i];
            OctBuild::Node& o = ob.nodes[seq[i]];
            o.mn = N.mn; o.mx = N.mx;
            if (N.first_child >= 0) {
                o.first_child = seq[N.first_child];
            } else {
                const std::vector<int>& E = level_ents[N.level];
                o.tris.assign(E.begin() + N.begin, E.begin() + N.begin + N.len);
            }
        }
    }
    return RT_OK;
}

// ---------------------------------------------------------------------------------------- buffers
// The regions of a lane's NEE index workspace (Batch neeSlot: one allocation, every region one queue capacity long);
// all null without a workspace.
struct NeeSlots {
    int* queue = nullptr;         // the NEE queue's slots (NeeIO slot)
    int* fallback = nullptr;      // the vertices k_path_nee's BVH walk could not decide (NeeIO fb_slot)
    unsigned* key = nullptr;      // the NEE sort's keys at the queue positions (NeeIO key)
    int* bin[kMatClasses] = {};   // the material bins' index lists (BinIO idx)
    static size_t ints(size_t ncap) { return (3 + kMatClasses) * ncap; }
    NeeSlots() = default;
    NeeSlots(int* base, size_t ncap)
        : queue(base), fallback(base + ncap), key(reinterpret_cast<unsigned*>(base + 2 * ncap)) {
        for (int cl = 0; cl < kMatClasses; ++cl) bin[cl] = base + (3 + cl) * ncap;
    }
};

// The device buffers of one batch in flight.  A lane releases them all at once — assigning an empty Batch — when its
// queue capacity must grow or the pass changes between the path and the reference layout (ensure_workspace); the
// sort, shadow and NEE groups are allocated on first use by the scenes that need them.
struct Batch {
    DevBuf<float4> ray;           // rays as interleaved (o, d) pairs: rayO = ray, rayD = ray + 1
    DevBuf<float4> lamA, lamB;    // reference mode
    DevBuf<float4> pdfA, pdfB, hitB;
    DevBuf<float4> rec;           // path mode: one 128-B record per slot (rt_internal.h R_*)
    DevBuf<int> hitPrim;
    DevBuf<float4> hitD;          // path mode: (direction, prim) per compacted hit record (TraceIO hq_d)
    // coherence sort of path queues (multi-level octrees): side queue (interleaved pairs like ray), radix-sort buffers
    DevBuf<float4> sRay;
    DevBuf<int> sS, sVals, sValsAlt;       // sS: the sort permutation (TraceIO perm)
    DevBuf<unsigned> sKeys, sKeysAlt;
    DevBuf<unsigned> sQKey;                // the ray queue's sort keys at queue positions (written by the shade kernels)
    DevBuf<unsigned char> sTemp;           // the sorts' histograms and meta (sort_temp_bytes)
    // shadow queue (multi-level octrees): {o, tMax}, {d, slot}, pending contribution (2 x float4)
    DevBuf<float4> shO, shD, shLA, shLB;
    // deferred NEE of the mixed-scene shade (rt_internal.h NeeIO): records per slot, the index workspace
    DevBuf<float4> neeRec;
    DevBuf<int> neeSlot;
    NeeSlots nee;                          // neeSlot's regions for the current queue capacity
    // specular-chain guides: two ping-pong queues of continuation rays, interleaved pairs like ray
    DevBuf<float4> chainRay;
    // RT_CHAIN_CURVED: kChainMax surface records and one float4 of segment lengths per sample slot, array after array
    DevBuf<float4> chainRec;

    float4* rayO() const { return ray.get(); }
    float4* rayD() const { return ray.get() + 1; }
    // slots the buffers of this layout hold (0: the other layout's, or none)
    size_t capacity(bool path) const { return path ? rec.capacity() / kRecF4 : lamB.capacity(); }
};

}  // namespace

// One lane: its batch buffers and the state that lives as long as the context.  Path mode keeps kLanes lanes so that
// consecutive batches run concurrently on separate streams: one batch's VALU-bound traversal overlaps the other's
// HBM-bound path-state traffic.
struct Work {
    Batch b;
    DevBuf<int> qcount;  // queue q's counters at [q * kQRegion + kQLen / kQTraceTicket / ...] (rt_internal.h)
    // BFS FIFO overflow ring of the multi-level traversal (qcap 0): one per lane, because the lanes' kernels run
    // concurrently and index the ring by their own global thread id
    DevBuf<int> ring;
    // multi-level scenes in path mode: the queue positions of the rays the trace kernel's BVH walk could not decide
    // (TraceIO fb_pos; k_trace_fallback traces them with the reference BFS)
    DevBuf<int> tfb;
    // specular-chain guides: the counters of the continuation queues, region l - 1 for level l's queue (its shard
    // lengths, its trace's chunk tickets and fallback list length), and the unused region the last level is given
    DevBuf<int> chain_ctr;
    hipStream_t stream = nullptr;  // lanes >= 1: own stream (lane 0 runs on the caller's stream)
    hipEvent_t film_done = nullptr;
};

struct rt_ctx {
    // coherence sort of path queues (multi-level octrees): scene quantisation of the sort key
    float4 sort_lo{}, sort_scale{};
    int device = 0;
    int octree_build = RT_OCTREE_BUILD_DEVICE;
    hipStream_t stream = nullptr;
    std::string err;
    bool have_scene = false, have_cam = false, have_smp = false, have_film = false, have_integ = false;
    rt_camera_desc cam{};
    rt_sampler_desc smp{};
    rt_film_desc film{};
    rt_integrator_desc integ{};
    // scene (host mirrors kept for export)
    int n_tris = 0;
    std::vector<float> h_bounds;
    std::vector<int32_t> h_child, h_leaf_first, h_leaf_count, h_refs;
    rt_octree_info info{};
    bool cull = false;
    bool scene_full = false;   // the scene needs the general path-shade kernel
    bool scene_rough = false;  // a non-emissive RT_MAT_ROUGH material: the RGH instantiations
    long long rgh_launches[2] = {0, 0};  // the last path pass's launches of them: shade, NEE (rt_debug_rough_stats)
    bool scene_conductor = false;  // a non-emissive RT_MAT_CONDUCTOR material: RGH level 2
    long long cnd_launches[2] = {0, 0};  // the last path pass's level-2 launches: shade, NEE (rt_debug_conductor_stats)
    bool scene_rough_dielectric = false;  // a non-emissive RT_MAT_ROUGH_DIELECTRIC material: RGH level 3
    long long rgl_launches[2] = {0, 0};  // the last path pass's level-3 launches: shade, NEE (rt_debug_roughglass_stats)
    DevScene dsc{};
    std::vector<DevBuf<unsigned char>> scene_allocs;  // the arrays dsc points to
    const float* d_kappa = nullptr;  // per analytic shape: the curvature the curved chain guides use (in scene_allocs)
    // mesh lights of the uploaded scene: per light its slice (first, n) of the shared id and cdf arrays
    // (n = 0: not a mesh light) and its total area; the arrays themselves are in scene_allocs.  any = the path kernels
    // run their ML instantiations.
    struct MeshLights {
        bool any = false;
        std::vector<int> first, n;
        std::vector<float> area;
        const int* tri = nullptr;
        const float* cdf = nullptr;
    } ml;
    // the environment light bound to the uploaded scene (rt_scene_set_environment): its baked texels and
    // cdf tables, and the scene's light list with the environment's DevLight appended (dsc.lights points to it while
    // live; base_lights / h_lights are the upload's list, which clearing restores).  live = the path kernels run their
    // TL = 2 instantiations and every traced depth ends with k_env_miss.
    struct Environment {
        bool live = false;
        int W = 0, H = 0;
        float total = 0.f;
        DevBuf<float4> coef;
        DevBuf<float> cond, marg;
        DevBuf<DevLight> lights;
        DevLight dev{};
    } env;
    std::vector<DevLight> h_lights;         // the uploaded scene's DevLights (mesh lights completed)
    const DevLight* base_lights = nullptr;  // ... on the device (in scene_allocs)
    // albedo textures of the uploaded scene (rt_scene_set_textures): live = the path kernels run their TEX
    // instantiations on dev (the DevTex in device memory that points to the other arrays).  table: the RGB -> sigmoid
    // coefficient table (kRgbRes z-nodes, then kRgbTableFloats coefficients), uploaded once per context on first use.
    // mat_flags: per material of the scene, bit 0 = it emits, bit 1 = an analytic shape uses it, bit 2 = a conductor, bit 3 = a rough glass (none takes a texture).
    struct Textures {
        bool live = false;
        DevBuf<float4> texels;
        DevBuf<int4> recs;
        DevBuf<int> matTex;
        DevBuf<float2> triUV;
        DevBuf<DevTex> dev;
        DevBuf<float> table;
        std::vector<unsigned char> mat_flags;
        size_t n_texels = 0;
    } tx;
    // absorbing media of the uploaded scene (rt_scene_set_media): bound = one entry per material, table =
    // their (c0, c1, c2, sigma) on the device, live = some sigma > 0, so depths >= 1 of a path pass run k_medium_absorb.
    // mat_type / mat_emits: per material of the scene, what rt_scene_set_media validates against.  ctr: the stage's
    // spread segment counter, zeroed per path pass; launches: the last path pass's launches of the stage.
    struct Media {
        bool live = false;
        std::vector<rt_medium> bound;
        DevBuf<float4> table;
        DevBuf<unsigned long long> ctr;
        std::vector<int> mat_type;
        std::vector<unsigned char> mat_emits;
        int launches = 0;
        bool counted = false;  // the last path pass ran the stage: ctr holds its segments (else they are 0)
    } med;
    // albedo demodulation: the sensor albedo of the scene's materials, then of its texels, 16 B per
    // entry; built on first use and again after rt_scene_upload, rt_scene_set_textures or rt_film_set
    struct Albedo {
        DevBuf<float4> table;
        bool valid = false;
    } alb;
    // spectra + resolve matrices
    HostSpectra hs;
    DevBuf<DevSpectra> d_spec;
    float resolveA[9], resolveB[9];
    DevBuf<float> d_resolve;
    // pixel work list
    int tile = 32, n_shards = 1, shard_id = 0;
    bool work_dirty = true;
    int n_work = 0;
    DevBuf<int> d_work;
    // one workspace per lane (path mode runs up to kLanes batches concurrently on separate streams)
    Work ws[kLanes];
    bool warned_eye = false;    // check_ready: the camera-eye-beyond-oguard warning was printed
    Knobs knobs;
    int bvh_count[3][2] = {};  // per BVH (set 0, set 1, any-hit): nodes, tiles (rt_bvh_export)
    hipEvent_t done = nullptr; // recorded at the end of every pass: a later call on another stream waits for it
    DevBuf<unsigned long long> d_ctr;
    DevBuf<float4> d_film;     // staging film for rt_render_pass (host film)
    DevBuf<float> d_cdf;       // Gaussian / Lanczos filter tables: x then y, cdf_n + 1 floats each
    int cdf_n = 0;
    int film_y_int = 0;  // the film's raster y (float division + floor) equals the integer division for every pixel
    DevBuf<uint32_t> d_sobol_mats;  // Sobol generator columns; d_sobol_fwd: fwd then inv tables for sobol_m
    DevBuf<uint64_t> d_sobol_fwd;
    int sobol_m = 0;
    int grid = 0;              // persistent grid size (blocks)
    // stats
    rt_stats stats{};
    double ms_env_miss = 0;    // the environment's miss stage alone (also in stats.ms_shade); zeroed with the stats
    struct Ev { hipEvent_t a, b; int stage; };
    std::vector<Ev> pending;
    std::vector<hipEvent_t> pool;
    int work_epoch = 0;        // bumped whenever build_work rebuilds d_work
    // multi-device context (rt_options.n_devices > 1): this context renders on devices[0] and
    // peers[j] on devices[j + 1]; tile t of the caller's shard goes to device (t / n_shards) mod n_devices
    std::vector<rt_ctx*> peers;
    struct PeerLink {          // on devices[0]: peer j's owned pixel ids and its compact exchange buffer
        DevBuf<int> work0;
        DevBuf<float4> xfer0;
        int n = 0, epoch = -1;
    };
    std::vector<PeerLink> links;
    hipEvent_t gathered = nullptr;   // devices[0]: peers' pixels packed (multi-device) / peer: pass done
    DevBuf<float4> xfer;             // on a peer: its compact exchange buffer
    // adaptive sampling session (rt_adaptive_*): device film and moments, the active pixel list (a
    // subsequence of d_work, ping-ponged by the compaction), the per-block estimate and the compaction's scratch
    struct Adaptive {
        bool live = false;
        rt_adaptive_desc desc{};
        rt_adaptive_info info{};
        DevBuf<float4> film;
        DevBuf<float2> mom;
        DevBuf<int> active[2];
        int cur = 0;                 // active[cur] is the current list (info.active_pixels entries)
        DevBuf<float> block_error;
        DevBuf<int> converged, wave_count, wave_offset, totals;
        DevBuf<float4> feat;         // rt_adaptive_denoise: the feature film of indices [0, feat_k), 0: not rendered,
        int feat_k = 0;              // through the chain pass of depth feat_chain
        int feat_chain = 0;
        DevBuf<float4> alb;          // rt_adaptive_denoise_albedo: the albedo film of the same indices,
        int alb_k = 0;               // rendered together with feat; 0: not rendered
        int alb_chain = 0;
        // a guided temporal frame's session (rt_temporal_frame_guided): with `on` the steps estimate the
        // block errors with k_temporal_error, on the film blended with rec, the frame's reprojected history (the
        // temporal session's buffer; null: there is none)
        struct Guide {
            bool on = false;
            const float4* rec = nullptr;
            float max_history = 0.f;
        } guide;
    } ad;
    // denoiser workspace (rt_denoise, rt_adaptive_denoise): staging of the host arrays, the guides and
    // the (c, var) ping-pong; grows on demand
    struct Denoise {
        DevBuf<float4> film, feat, g, cv[2], out;
        DevBuf<float4> alb, a;       // the albedo variants: albedo film staging, the per-pixel (a, sa)
        DevBuf<float2> mom, gz;
        DevBuf<float> var;
    } dn;
    // temporal accumulation (rt_temporal_*): the session's device-resident history, 56 B per pixel in
    // each of two sets (set `cur` is the last frame's: its unfiltered accumulation, features and positions, with M its
    // camera's world-to-film matrix); the staging of rt_temporal_accumulate's host arrays; the class counters
    struct Temporal {
        bool live = false;
        rt_temporal_desc desc{};
        int frames = 0;              // frames behind set `cur` (0: no history)
        int cur = 0;
        float M[16] = {};
        DevBuf<float4> film[2], feat[2], pos[2];
        DevBuf<float2> mom[2];
        DevBuf<float4> s_film, s_feat, s_pos, s_hfilm, s_hfeat, s_hpos, s_out;
        DevBuf<float2> s_mom, s_hmom, s_outm;
        DevBuf<unsigned long long> ctr;
        DevBuf<float4> rec;          // guided frames: the reprojected history, (nh, m1h, m2h, 0) per pixel;
                                     // also rt_temporal_block_error's
    } tp;
};

namespace {

void set_error(rt_ctx* c, const std::string& msg) {
    if (c) c->err = msg;
}
int fail(rt_ctx* c, int code, const std::string& msg) {
    if (c) c->err = msg;
    return code;
}
#define HIPCHK(c, call)                                                                                   \
    do {                                                                                                  \
        hipError_t _e = (call);                                                                           \
        if (_e != hipSuccess)                                                                             \
            return fail((c), _e == hipErrorOutOfMemory ? RT_E_OOM : RT_E_HIP,                             \
                        std::string(#call) + ": " + hipGetErrorString(_e));                               \
    } while (0)

// (the coefficient table stays: it belongs to the context, not to the scene)
void free_textures(rt_ctx* c) {
    c->tx.live = false;
    c->tx.texels.reset(); c->tx.recs.reset(); c->tx.matTex.reset(); c->tx.triUV.reset(); c->tx.dev.reset();
    c->tx.n_texels = 0;
    c->alb.table.reset();  // (the albedo table covers the texels: released with them, rebuilt on first use)
    c->alb.valid = false;
}

// (the scene's own light list again)
void free_environment(rt_ctx* c) {
    if (c->env.live) {
        c->dsc.lights = c->base_lights;
        c->dsc.n_lights = (int)c->h_lights.size();
    }
    c->env = rt_ctx::Environment{};
}

// (the counter stays: it belongs to the context)
void free_media(rt_ctx* c) {
    c->med.live = false;
    c->med.bound.clear();
    c->med.table.reset();
}

void free_scene(rt_ctx* c) {
    free_textures(c);
    free_environment(c);
    free_media(c);
    c->med.mat_type.clear();
    c->med.mat_emits.clear();
    c->h_lights.clear();
    c->base_lights = nullptr;
    c->tx.mat_flags.clear();
    c->scene_allocs.clear();
    c->dsc = DevScene{};
    c->d_kappa = nullptr;
    c->ml = rt_ctx::MeshLights{};
    c->have_scene = false;
}

// (the NEE queue, the fallback list, the NEE sort keys: rt_internal.h NeeIO; the material bins' index lists: BinIO)
int ensure_nee_workspace(rt_ctx* c, Batch& b, size_t rec_f4, size_t ncap) {
    HIPCHK(c, b.neeRec.reserve(rec_f4));
    HIPCHK(c, b.neeSlot.reserve(NeeSlots::ints(ncap)));
    b.nee = NeeSlots(b.neeSlot.get(), ncap);
    return RT_OK;
}

int ensure_shadow_workspace(rt_ctx* c, Batch& b, size_t n) {
    if (b.shLB.capacity() < n) {  // allocating: a NEE workspace left by a mixed scene is given back first
        b.neeRec.reset();
        b.neeSlot.reset();
        b.nee = NeeSlots{};
    }
    HIPCHK(c, b.shO.reserve(n)); HIPCHK(c, b.shD.reserve(n));
    HIPCHK(c, b.shLA.reserve(n)); HIPCHK(c, b.shLB.reserve(n));
    return RT_OK;
}

int ensure_sort_workspace(rt_ctx* c, Batch& b, size_t n) {
    HIPCHK(c, b.sRay.reserve(2 * n)); HIPCHK(c, b.sS.reserve(n));
    HIPCHK(c, b.sVals.reserve(n)); HIPCHK(c, b.sValsAlt.reserve(n));
    HIPCHK(c, b.sKeys.reserve(n)); HIPCHK(c, b.sKeysAlt.reserve(n)); HIPCHK(c, b.sQKey.reserve(n));
    HIPCHK(c, b.sTemp.reserve(sort_temp_bytes()));
    return RT_OK;
}

// this lane's BFS overflow ring (multi-level octrees whose FIFO bound exceeds the register variants)
int ensure_ring(rt_ctx* c, Work& w) {
    if (c->dsc.qcap != 0) return RT_OK;
    HIPCHK(c, w.ring.reserve((size_t)c->dsc.ring_threads * (size_t)(c->dsc.ring_mask + 1)));
    return RT_OK;
}
// the scene as a pass's kernels see it: the integrator's flags are the pass's, not the context's (c->dsc keeps 0 / 0:
// the debug entries run the simple kernels)
DevScene pass_scene(const rt_ctx* c, const BatchPlan& bp) {
    DevScene d = c->dsc;
    d.mis = bp.mis;
    d.full = bp.full;
    return d;
}
// ... and as a lane's kernels see it: its own overflow ring
DevScene lane_scene(const DevScene& sc, const Work& w) {
    DevScene d = sc;
    d.ring = w.ring.get();
    return d;
}

// hit_d: the path pass compacts its hits without packing them (PathPlan hit_d), so the batch needs hitD
int ensure_workspace(rt_ctx* c, Work& w, size_t n, bool path, bool hit_d = false) {
    int rc;
    HIPCHK(c, w.qcount.reserve(2 * kQRegion));
    if (&w != &c->ws[0] && !w.stream) HIPCHK(c, hipStreamCreateWithFlags(&w.stream, hipStreamNonBlocking));
    if (!w.film_done) HIPCHK(c, hipEventCreateWithFlags(&w.film_done, hipEventDisableTiming));
    if ((rc = ensure_ring(c, w))) return rc;
    Batch& b = w.b;
    // the compacted hit records' (direction, prim) stream, sized like hitB (RTMI_HIT_COMPACT: the single-leaf
    // simple path; the scene may have changed since the batch buffers were allocated)
    if (b.capacity(path) >= n) {
        if (hit_d) HIPCHK(c, b.hitD.reserve(n));
        else if (path) b.hitD.reset();  // (packed records, or another scene: not kept beside the batch)
        return RT_OK;
    }
    b = Batch{};  // every batch buffer of the lane, the sort, shadow and NEE groups included
    // path mode: queue arrays hold 2 ping-pong queues of n entries each
    size_t nq = path ? 2 * n : n;
    // rays as interleaved (o, d) pairs, 32 B per ray (rayD = rayO + 1, kernels index [k << rsh] with rsh = 1): a
    // scattered read of one ray (the coherence sort's gather) touches one line instead of two
    HIPCHK(c, b.ray.reserve(2 * nq));
    HIPCHK(c, b.pdfA.reserve(n)); HIPCHK(c, b.pdfB.reserve(n));
    HIPCHK(c, b.hitB.reserve(n)); HIPCHK(c, b.hitPrim.reserve(n));
    if (path) {
        HIPCHK(c, b.rec.reserve((size_t)kRecF4 * n));
        if (hit_d) HIPCHK(c, b.hitD.reserve(n));
    } else {
        HIPCHK(c, b.lamA.reserve(n)); HIPCHK(c, b.lamB.reserve(n));
    }
    return RT_OK;
}

// Sampler dimension bookkeeping of the simple path integrator (rt_device.h Smp): every path of a depth has drawn
// the same dimensions — the camera sample, then two Get2D per bounce — so the shade kernel takes its starting
// dimension as an argument instead of a per-slot field.  (A stratified sample with index >= spp draws zeros without
// advancing; its dimension is never read again.)
static int dim_get2d(const DevSampler& S, int dim) {
    if (S.kind == 1) return dim + 2;
    if (S.kind == 2) return (dim + 1 >= kSobolDims ? 2 : dim) + 2;
    return dim;
}
static int dim_after_camera(const DevSampler& S, const DevCamera& cam) {
    int dim = S.kind == 2 ? 2 : 0;                                                // StartPixelSample
    if (S.kind == 1) dim += 1;                                                    // Get1D (wavelengths)
    else if (S.kind == 2) dim = (dim >= kSobolDims ? 2 : dim) + 1;
    if (S.kind == 1) dim += 2;                                                    // GetPixel2D
    if ((cam.type == RT_CAMERA_PERSPECTIVE && cam.lens_radius > 0) || cam.type > RT_CAMERA_PINHOLE)
        dim = dim_get2d(S, dim);                                                  // lens sample
    return dim;
}

hipEvent_t ev_get(rt_ctx* c) {
    if (!c->pool.empty()) {
        hipEvent_t e = c->pool.back();
        c->pool.pop_back();
        return e;
    }
    hipEvent_t e;
    hipEventCreate(&e);
    return e;
}
void ev_mark(rt_ctx* c, hipStream_t st, int stage, hipEvent_t a) {
    if (!a) return;  // stage timing off
    hipEvent_t b = ev_get(c);
    hipEventRecord(b, st);
    c->pending.push_back({a, b, stage});
}
hipEvent_t ev_start(rt_ctx* c, hipStream_t st) {
    if (!c->knobs.stage_events) return nullptr;
    hipEvent_t a = ev_get(c);
    hipEventRecord(a, st);
    return a;
}
enum { ST_GEN = 0, ST_TRACE, ST_SHADE, ST_SHADOW, ST_FILM, ST_SORT, ST_FILTER, ST_ENVMISS };

void harvest(rt_ctx* c) {
    for (auto& e : c->pending) {
        float ms = 0;
        hipEventSynchronize(e.b);
        hipEventElapsedTime(&ms, e.a, e.b);
        switch (e.stage) {
            case ST_GEN: c->stats.ms_generate += ms; break;
            case ST_TRACE: c->stats.ms_trace += ms; c->stats.launches_trace += 1; break;
            case ST_SHADE: c->stats.ms_shade += ms; c->stats.launches_shade += 1; break;
            case ST_SHADOW: c->stats.ms_shadow += ms; break;
            case ST_SORT: c->stats.ms_sort += ms; break;
            case ST_FILTER: c->stats.ms_trace += ms; break;  // (the last depth's emitter filter: no trace launch)
            // the environment's miss stage: part of the shading time, and on its own for rt_debug_env_stats
            case ST_ENVMISS: c->stats.ms_shade += ms; c->ms_env_miss += ms; break;
            default: c->stats.ms_film += ms; break;
        }
        c->pool.push_back(e.a);
        c->pool.push_back(e.b);
    }
    c->pending.clear();
}

// Owned pixels in tile order: tile_size² tiles in row-major tile order, tile t owned iff t % n == id;
// inside a tile 8×8 micro-tiles (one wave64 = one micro-tile → coherent rays), row-major inside.
int build_work(rt_ctx* c) {
    if (!c->work_dirty && c->d_work.get()) return RT_OK;
    int W = c->film.res_x, H = c->film.res_y, T = c->tile;
    int tx = (W + T - 1) / T, ty = (H + T - 1) / T;
    std::vector<int> px;
    px.reserve((size_t)W * H / std::max(1, c->n_shards) + T * T);
    for (int t = 0; t < tx * ty; ++t) {
        if (t % c->n_shards != c->shard_id) continue;
        int x0 = (t % tx) * T, y0 = (t / tx) * T;
        for (int my = 0; my < T; my += 8)
            for (int mx = 0; mx < T; mx += 8)
                for (int yy = 0; yy < 8; ++yy)
                    for (int xx = 0; xx < 8; ++xx) {
                        int x = x0 + mx + xx, y = y0 + my + yy;
                        if (mx + xx < T && my + yy < T && x < W && y < H) px.push_back(y * W + x);
                    }
    }
    c->d_work.reset();  // (the release waits for the queued passes that still read the old list)
    HIPCHK(c, c->d_work.reserve(px.size()));
    HIPCHK(c, hipMemcpy(c->d_work.get(), px.data(), px.size() * sizeof(int), hipMemcpyHostToDevice));
    c->n_work = (int)px.size();
    c->work_dirty = false;
    ++c->work_epoch;
    return RT_OK;
}

// Sampling.h:781-807 Continuous_Inversion_Sampler table (Riemann sum, renormalised, last entry 1) and the
// filters' 1-D factors (filters.h:101-107 Gaussian with helpers.h:221-225, 228-231 Lanczos with 236-251);
// powf(v, 2) is written v * v.
template <class F>
void inversion_table(F pdf, float a, float b, int N, std::vector<float>& cdf) {
    cdf.assign(N + 1, 0.0f);
    float delta_x = (b - a) / (float)N;
    float sum = 0;
    for (int n = 1; n < N + 1; n++) {
        float x = a + delta_x * n;
        float current_x = x < a ? a : (b < x ? b : x);
        sum += delta_x * pdf(current_x);
        cdf[n] = sum;
    }
    float scaling_term = 1.0f / cdf[N];
    for (int n = 1; n < N; n++) cdf[n] *= scaling_term;
    cdf[N] = 1.0f;
}
inline float gaussian_f(float x, float mu, float sigma) {
    const float Pi = 3.14159265358979323846f;
    float v = x - mu;
    return 1.0f / std::sqrt(2 * Pi * sigma * sigma) * std::exp(-(v * v) / (2 * sigma * sigma));
}
inline float sinx_over_x(float x) {
    if (1 - x * x == 1) return 1;
    return std::sin(x) / x;
}
inline float windowed_sinc(float x, float radius, float tau) {
    const float Pi = 3.14159265358979323846f;
    if (std::fabs(x) > radius) return 0;
    return sinx_over_x(Pi * x) * sinx_over_x(Pi * (x / tau));
}
int build_filter_tables(const rt_film_desc& d, std::vector<float>& tx, std::vector<float>& ty) {
    float rx = d.filter_radius[0], ry = d.filter_radius[1];
    if (d.filter == RT_FILTER_GAUSSIAN) {
        float sigma = d.filter_param > 0 ? d.filter_param : 0.5f;
        float ex = gaussian_f(rx, 0, sigma), ey = gaussian_f(ry, 0, sigma);
        inversion_table([&](float x) { return std::max<float>(0, gaussian_f(x, 0, sigma) - ex); }, -rx, rx, 10000, tx);
        inversion_table([&](float y) { return std::max<float>(0, gaussian_f(y, 0, sigma) - ey); }, -ry, ry, 10000, ty);
        return 10000;
    }
    float tau = d.filter_param > 0 ? d.filter_param : 3.f;
    inversion_table([&](float x) { return windowed_sinc(x, rx, tau); }, -rx, rx, 2000, tx);
    inversion_table([&](float y) { return windowed_sinc(y, ry, tau); }, -ry, ry, 2000, ty);
    return 2000;
}

DevCamera dev_camera(const rt_camera_desc& d) {
    DevCamera c;
    std::memcpy(c.r2c, d.raster_to_camera, 64);
    std::memcpy(c.c2w, d.camera_to_world, 64);
    c.lens_radius = d.lens_radius;
    c.focal_distance = d.focal_distance;
    c.type = d.type;
    std::memcpy(c.r2s, d.raster_to_screen, 64);
    c.pinhole_depth = d.pinhole_depth;
    c.thin_focal = d.thin_focal;
    c.thin_aperture = d.thin_aperture_diameter;
    c.sensor_depth = d.sensor_depth;
    return c;
}
// Sobol generator matrices (32 dimensions, Joe-Kuo new-joe-kuo-6.21201 direction numbers; dimension 0 = van der
// Corput) and SobolIntervalToIndex's tables for a resolution exponent m (the reference's VdCSobolMatrices /
// VdCSobolMatricesInv, HelperFunctions.h:212-470, derived here by inverting the 2m x 2m GF(2) pixel map).
void sobol_tables(int m, std::vector<uint32_t>& mats, std::vector<uint64_t>& fwd, std::vector<uint64_t>& inv) {
    static const int dirs[31][9] = {
        {1, 0, 1}, {2, 1, 1, 3}, {3, 1, 1, 3, 1}, {3, 2, 1, 1, 1}, {4, 1, 1, 1, 3, 3}, {4, 4, 1, 3, 5, 13},
        {5, 2, 1, 1, 5, 5, 17}, {5, 4, 1, 1, 5, 5, 5}, {5, 7, 1, 1, 7, 11, 19}, {5, 11, 1, 1, 5, 1, 1},
        {5, 13, 1, 1, 1, 3, 11}, {5, 14, 1, 3, 5, 5, 31}, {6, 1, 1, 3, 3, 9, 7, 49}, {6, 13, 1, 1, 1, 15, 21, 21},
        {6, 16, 1, 3, 1, 13, 27, 49}, {6, 19, 1, 1, 1, 15, 7, 5}, {6, 22, 1, 3, 1, 15, 13, 25},
        {6, 25, 1, 1, 5, 5, 19, 61}, {7, 1, 1, 3, 7, 11, 23, 15, 103}, {7, 4, 1, 3, 7, 13, 13, 15, 69},
        {7, 7, 1, 1, 3, 13, 7, 35, 63}, {7, 8, 1, 3, 5, 9, 1, 25, 53}, {7, 14, 1, 3, 1, 13, 9, 35, 107},
        {7, 19, 1, 3, 1, 5, 27, 61, 31}, {7, 21, 1, 1, 5, 11, 19, 41, 61}, {7, 28, 1, 3, 5, 3, 3, 13, 69},
        {7, 31, 1, 1, 7, 13, 1, 19, 1}, {7, 32, 1, 3, 7, 5, 13, 19, 59}, {7, 37, 1, 1, 3, 9, 25, 29, 41},
        {7, 41, 1, 3, 5, 13, 23, 1, 55}, {7, 42, 1, 3, 7, 3, 13, 59, 17}};
    const int S = kSobolMatrixSize;
    mats.assign((size_t)kSobolDims * S, 0u);
    for (int j = 0; j < 32; ++j) mats[j] = 1u << (31 - j);
    for (int d = 1; d < kSobolDims; ++d) {
        int s = dirs[d - 1][0], a = dirs[d - 1][1];
        uint64_t dn[kSobolMatrixSize];
        for (int i = 0; i < s; ++i) dn[i] = (uint64_t)dirs[d - 1][2 + i];
        for (int i = s; i < S; ++i) {  // m_i = 2^s m_{i-s} ^ m_{i-s} ^ sum_k a_k 2^k m_{i-k}
            uint64_t v = dn[i - s] ^ (dn[i - s] << s);
            for (int k = 1; k < s; ++k)
                if ((a >> (s - 1 - k)) & 1) v ^= dn[i - k] << k;
            dn[i] = v;
        }
        for (int j = 0; j < S; ++j) mats[(size_t)d * S + j] = (uint32_t)((dn[j] << (63 - j)) >> 32);
    }
    fwd.assign(S, 0);
    inv.assign(S, 0);
    if (m == 0) return;
    const int n = 2 * m;
    auto col = [&](int j) { return ((uint64_t)(mats[j] >> (32 - m)) << m) | (uint64_t)(mats[S + j] >> (32 - m)); };
    for (int c = 0; c + n < S; ++c) fwd[c] = col(n + c);
    uint64_t rows[32], id[32];
    for (int r = 0; r < n; ++r) {
        rows[r] = 0;
        for (int j = 0; j < n; ++j) rows[r] |= ((col(j) >> r) & 1ull) << j;
        id[r] = 1ull << r;
    }
    for (int c = 0; c < n; ++c) {
        int p = c;
        while (!((rows[p] >> c) & 1)) ++p;
        std::swap(rows[p], rows[c]);
        std::swap(id[p], id[c]);
        for (int r = 0; r < n; ++r)
            if (r != c && ((rows[r] >> c) & 1)) { rows[r] ^= rows[c]; id[r] ^= id[c]; }
    }
    for (int c = 0; c < n; ++c)  // column c of M^-1: index bits set by pixel bit c
        for (int r = 0; r < n; ++r) inv[c] |= ((id[r] >> c) & 1ull) << r;
}

DevSampler dev_sampler(const rt_ctx* c) {
    const rt_sampler_desc& d = c->smp;
    DevSampler s{};
    s.kind = d.kind; s.xs = d.x_samples; s.ys = d.y_samples; s.jitter = d.jitter; s.seed = d.seed;
    s.spp = d.kind == RT_SAMPLER_STRATIFIED ? d.x_samples * d.y_samples : d.x_samples;
    s.randomize = d.randomize;
    s.sobol_m = c->sobol_m;
    s.scale = 1 << c->sobol_m;
    s.sobol_mats = c->d_sobol_mats.get();
    s.sobol_fwd = c->d_sobol_fwd.get();
    s.sobol_inv = s.sobol_fwd ? s.sobol_fwd + kSobolMatrixSize : nullptr;
    auto pow2 = [](int v) { return v > 0 && (v & (v - 1)) == 0; };
    if (s.kind == RT_SAMPLER_STRATIFIED && pow2(s.xs) && pow2(s.ys)) {
        s.p2 = 1;
        while ((1 << s.lg_xs) < s.xs) ++s.lg_xs;
        s.inv_xs = 1.0f / (float)s.xs;   // exact: powers of two
        s.inv_ys = 1.0f / (float)s.ys;
        s.inv_spp = 1.0f / (float)s.spp;
    }
    return s;
}

// sample ids of a batch starting at sample index b0 (s = i n_pixels + j)
SampleIds sample_ids(const int* work, int n_work, int b0) {
    SampleIds ids{work, n_work, b0, nullptr, nullptr};
    ids.np_div = make_intdiv((uint32_t)n_work);
    return ids;
}

// Sobol tables on the device for the current film (scale = RoundUpPow2(max(res)), samplers.h:243)
int ensure_sobol(rt_ctx* c) {
    if (c->smp.kind != RT_SAMPLER_SOBOL) return RT_OK;
    int v = std::max(c->film.res_x, c->film.res_y) - 1;
    v |= v >> 1; v |= v >> 2; v |= v >> 4; v |= v >> 8; v |= v >> 16;
    int m = (int)std::log2((float)(v + 1));
    if (m > 16) return fail(c, RT_E_LIMIT, "Sobol sampler supports film resolutions up to 65536");
    if (c->d_sobol_mats.get() && c->sobol_m == m) return RT_OK;
    std::vector<uint32_t> mats;
    std::vector<uint64_t> fwd, inv;
    sobol_tables(m, mats, fwd, inv);
    HIPCHK(c, c->d_sobol_mats.reserve(mats.size()));
    HIPCHK(c, c->d_sobol_fwd.reserve(2 * kSobolMatrixSize));
    uint64_t* const d_fwd = c->d_sobol_fwd.get();
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(c->d_sobol_mats.get(), mats.data(), mats.size() * 4, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(d_fwd, fwd.data(), kSobolMatrixSize * 8, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(d_fwd + kSobolMatrixSize, inv.data(), kSobolMatrixSize * 8, hipMemcpyHostToDevice));
    c->sobol_m = m;
    return RT_OK;
}
DevFilm dev_film(const rt_ctx* c) {
    const rt_film_desc& d = c->film;
    DevFilm f;
    f.res_x = d.res_x; f.res_y = d.res_y; f.filter = d.filter;
    f.rx = d.filter_radius[0]; f.ry = d.filter_radius[1]; f.imaging_ratio = d.imaging_ratio;
    f.cdf_x = c->d_cdf.get();
    f.cdf_y = f.cdf_x ? f.cdf_x + (c->cdf_n + 1) : nullptr;
    f.cdf_n = c->cdf_n;
    f.rx_div = make_intdiv((uint32_t)d.res_x);
    f.y_int = c->film_y_int;
    return f;
}

// The reference integrator's kernel arguments over a lane's batch buffers, n samples in a queue of nsh shards
// (render pass and rt_debug_samples).  The caller adds the shade's pixel list and film.
struct RefIO {
    GenOut go;
    TraceIO tio;
    ShadeRefIO sio;
};
RefIO ref_io(const rt_ctx* c, const Batch& b, int n, int nsh) {
    RefIO r{};
    r.go = GenOut{b.rayO(), b.rayD(), b.lamA.get(), b.lamB.get(), b.pdfA.get(), b.pdfB.get(), RecView{nullptr, 0, 0}, 0, 1};
    r.tio = TraceIO{b.rayO(), b.rayD(), QueueView{nullptr, shard_stride(n, nsh), n, nsh}, c->cull ? 1 : 0, b.hitB.get(),
                    b.hitPrim.get(), nullptr, 1};
    ShadeRefIO& io = r.sio;
    io.rsh = 1;  // the workspace's interleaved rays
    float a = c->integ.albedo_rgb[0];
    io.albedo_c2 = (a - .5f) / std::sqrt(a * (1 - a));  // color.cpp:35-37
    float g = 1.0f / (2.0f * 1.0f);                      // RGBIlluminant(1,1,1): scale = 2*max = 2, rgb/scale = .5
    io.illum_c2 = (g - .5f) / std::sqrt(g * (1 - g));
    io.illum_scale = 2.0f;
    io.rayD = b.rayD(); io.lamA = b.lamA.get(); io.lamB = b.lamB.get(); io.pdfA = b.pdfA.get(); io.pdfB = b.pdfB.get();
    io.hitB = b.hitB.get(); io.hitPrim = b.hitPrim.get();
    return r;
}

int check_ready(rt_ctx* c) {
    if (!c) return RT_E_ARG;
    if (!c->have_scene || !c->have_cam || !c->have_smp || !c->have_film || !c->have_integ)
        return fail(c, RT_E_STATE, "scene, camera, sampler, film and integrator must be set before rendering");
    // The multi-level BVH decides rays whose origin lies within oguard = 8 M of the scene's vertices' extent M
    // (scene_bvh); a camera eye farther out sends every camera ray to the exact octree BFS.  Correct, but a large
    // performance cliff that only the fallback counter shows: say so once per context.
    if (c->dsc.oguard > 0.f && !c->warned_eye) {
        const float* t = c->cam.camera_to_world + 12;  // column-major: the translation column
        if (std::max(std::fabs(t[0]), std::max(std::fabs(t[1]), std::fabs(t[2]))) > c->dsc.oguard) {
            std::fprintf(stderr, "rtmi355x: the camera eye lies beyond the BVH's origin guard (8x the scene extent): "
                                 "every camera ray takes the exact octree BFS (slow, still exact)\n");
            c->warned_eye = true;
        }
    }
    return RT_OK;
}

// Calls on a context may use different streams (rt_render_pass on the context's stream, rt_render_pass_device on the
// caller's, the debug entry points): each waits for the previous call's work, which shares the lane-0 buffers.
int order_after_previous(rt_ctx* c, hipStream_t st) {
    if (!c->done) HIPCHK(c, hipEventCreateWithFlags(&c->done, hipEventDisableTiming));
    else HIPCHK(c, hipStreamWaitEvent(st, c->done, 0));
    return RT_OK;
}
int mark_done(rt_ctx* c, hipStream_t st) {
    HIPCHK(c, hipEventRecord(c->done, st));
    return RT_OK;
}

// The bracket of a call that queues work on st: wait for the previous call, run body (a callable returning a status),
// record `done` whatever body returned; the status is body's, or the record's when body succeeded.
template <class Body>
int ordered(rt_ctx* c, hipStream_t st, Body body) {
    int rc = order_after_previous(c, st);
    if (rc) return rc;
    rc = body();
    const int rc2 = mark_done(c, st);
    return rc ? rc : rc2;
}

// A caller's host array of n elements into a staging buffer (grow-only: a larger earlier call's block is reused), and a
// buffer's first n elements out to a host array; both asynchronous on st.
template <class T>
int stage_in(rt_ctx* c, DevBuf<T>& buf, const void* host, size_t n, hipStream_t st) {
    HIPCHK(c, buf.reserve(n));
    HIPCHK(c, hipMemcpyAsync(buf.get(), host, n * sizeof(T), hipMemcpyHostToDevice, st));
    return RT_OK;
}
template <class T>
int stage_out(rt_ctx* c, void* host, const DevBuf<T>& buf, size_t n, hipStream_t st) {
    HIPCHK(c, hipMemcpyAsync(host, buf.get(), n * sizeof(T), hipMemcpyDeviceToHost, st));
    return RT_OK;
}

// the pixels a pass renders and their order: the full work list, or an adaptive session's active list with the
// session's moment film (mom null: no moments)
struct PassTarget {
    const int* work;
    int n;
    float2* mom;
};

int render_device_body(rt_ctx* c, int ib, int ie, float4* film, hipStream_t st, const PassTarget& pass);
// one render pass over [ib, ie) of the full work list into the device film
int render_device(rt_ctx* c, int ib, int ie, float4* film, hipStream_t st) {
    int rc = check_ready(c);
    if (rc) return rc;
    return ordered(c, st, [&]() -> int {
        if (int rc = build_work(c)) return rc;  // (may reallocate d_work: the target is formed after it)
        return render_device_body(c, ib, ie, film, st, PassTarget{c->d_work.get(), c->n_work, nullptr});
    });
}

// The refusals of a pass over indices [ib, ie) that need the context (render pass and feature pass): the range, the
// Sobol tables of the current film, the unjittered stratified sampler's index limit.
int pass_checks(rt_ctx* c, int ib, int ie) {
    if (ib < 0 || ie < ib) return fail(c, RT_E_ARG, "invalid index range");
    if (int rc = ensure_sobol(c)) return rc;
    if (c->smp.kind == RT_SAMPLER_STRATIFIED && !c->smp.jitter && ie > dev_sampler(c).spp)
        return fail(c, RT_E_ARG, "StratifiedSampler without jitter supports indices < SamplesPerPixel (samplers.h:83-87)");
    return RT_OK;
}
// what a pass over [ib, ie) of n_work pixels is planned from (rt_pass_plan.h)
PassFacts pass_facts(const rt_ctx* c, int n_work, int ib, int ie) {
    PassFacts f;
    f.qcap = c->dsc.qcap; f.n_tris = c->dsc.n_tris; f.n_lights = c->dsc.n_lights;
    f.n_emit_tris = c->dsc.n_emit_tris; f.coop_ok = c->dsc.coop_ok;
    f.scene_full = c->scene_full; f.textures = c->tx.live; f.mesh_light = c->ml.any;
    f.environment = c->env.live;
    f.rough = c->scene_rough;
    f.conductor = c->scene_conductor;
    f.rough_dielectric = c->scene_rough_dielectric;
    f.media = c->med.live;
    f.integ = c->integ.kind == RT_INTEGRATOR_PATH_MIS ? kIntegPathMis
              : c->integ.kind == RT_INTEGRATOR_PATH   ? kIntegPath : kIntegReference;
    f.max_depth = c->integ.max_depth;
    f.n_work = n_work; f.ib = ib; f.ie = ie;
    return f;
}

// One trace launch of path mode, and the exact BFS for the rays it listed when the plan says one may be (BatchPlan
// trace_fallback), as one ST_TRACE stage: the path pass's bounces and the chain pass's levels.
int trace_with_fallback(rt_ctx* c, hipStream_t s, const DevScene& sc, const TraceIO& tio, bool fallback) {
    hipEvent_t e0 = ev_start(c, s);
    HIPCHK(c, launch_trace_closest(s, c->grid, sc.qcap, sc, tio, c->d_ctr.get()));
    if (fallback) HIPCHK(c, launch_trace_fallback(s, c->grid, sc.qcap, sc, tio, c->d_ctr.get()));
    ev_mark(c, s, ST_TRACE, e0);
    return RT_OK;
}

// ---- the reference integrator's pass: one batch at a time on the caller's stream
int render_reference(rt_ctx* c, const BatchPlan& bp, int ib, int ie, float4* film, hipStream_t st,
                     const PassTarget& pass) {
    const DevCamera cam = dev_camera(c->cam);
    const DevSampler smp = dev_sampler(c);
    const DevFilm fd = dev_film(c);
    const DevScene sc = pass_scene(c, bp);
    Work& w = c->ws[0];
    if (int rc = ensure_workspace(c, w, bp.ncap, false)) return rc;
    for (int b0 = ib; b0 < ie; b0 += bp.B) {
        int nIdx = std::min(bp.B, ie - b0);
        int nS = nIdx * pass.n;
        SampleIds ids = sample_ids(pass.work, pass.n, b0);
        RefIO r = ref_io(c, w.b, nS, bp.nsh);
        hipEvent_t e0 = ev_start(c, st);
        HIPCHK(c, launch_generate(st, c->grid, nS, ids, cam, smp, fd, r.go));
        ev_mark(c, st, ST_GEN, e0);
        e0 = ev_start(c, st);
        HIPCHK(c, launch_trace_closest(st, 0, sc.qcap, lane_scene(sc, w), r.tio, c->d_ctr.get()));
        ev_mark(c, st, ST_TRACE, e0);
        r.sio.work_pixels = pass.work; r.sio.n_pixels = pass.n; r.sio.n_index = nIdx;
        r.sio.film = film;
        r.sio.mom = pass.mom;
        e0 = ev_start(c, st);
        HIPCHK(c, launch_ref_shade_film(st, 0, sc, c->d_spec.get(), fd, r.sio, c->d_ctr.get()));
        ev_mark(c, st, ST_FILM, e0);
    }
    return RT_OK;
}

// ---- path mode: up to PathPlan lanes batches in flight, batch k on lane k mod lanes (lane 0 = the caller's stream).
// Within a lane everything is stream-ordered; across lanes only the film kernels are chained (batch k's film after
// batch k-1's), so every pixel still adds its sample indices in increasing order.
//
// Concurrent lanes share the CUs.  Each launch still asks for every resident block (grid_div 1): the dispatcher hands
// blocks to whichever lane's kernel has them pending, so a VALU-bound trace and an HBM-bound shade of the other lane
// end up co-resident (Cornell A/B: 1 lane 1217, 2 lanes with half grids 1422, with full grids 1500)

// what the stages of one path pass share
struct PathPass {
    rt_ctx* c;
    BatchPlan bp;
    PathPlan pp;
    DevScene sc;  // pass_scene
    DevCamera cam;
    DevSampler smp;
    DevFilm fd;
    PassTarget target;
    float4* film;
};
// one lane's batch in flight
struct Lane {
    Work* w = nullptr;
    hipStream_t s = nullptr;
    DevScene sc{};   // lane_scene
    RecView rv{};
    SampleIds ids{};
    int nIdx = 0;    // sample indices of the batch
    int nS = 0;      // its samples
    int S = 0;       // shard stride of every queue of this batch: shard j at [j S, j S + len_j)
    int cur = 0;     // the current ray queue of the two (ping-pong; ncap entries each)
    float4* rays(const PathPass& p, int q) const { return w->b.rayO() + 2 * (size_t)q * p.bp.ncap; }
    int* counters(int q) const { return w->qcount.get() + kQRegion * q; }
};
// one lane's bounce at one depth: what the stages hand on
struct Bounce {
    int depth;
    DepthPlan d;
    int* qc_cur;            // the counter regions of the current and the next queue
    int* qc_nxt;
    const float4* cO;       // the rays the trace and the shade read (the queue's, the filtered or the sorted ones)
    QueueView qv;           // ... and their queue
    TraceIO tio{};
    PathIO pio{};           // the shade's, read by the NEE and shadow stages too
    ShadowQueueIO sqio{};
    NeeIO nio{};
};

int path_workspaces(const PathPass& p) {
    rt_ctx* c = p.c;
    const BatchPlan& bp = p.bp;
    const PathPlan& pp = p.pp;
    for (int l = 0; l < pp.lanes; ++l) {
        Work& w = c->ws[l];
        int rc;
        if ((rc = ensure_workspace(c, w, bp.ncap, true, pp.hit_d()))) return rc;
        if (pp.sort_rays && (rc = ensure_sort_workspace(c, w.b, bp.ncap))) return rc;
        // the trace-fallback list (multi-level octrees): one entry per queue position at most
        if (bp.dyn) HIPCHK(c, w.tfb.reserve(bp.ncap));
    }
    for (int l = 0; l < pp.lanes && pp.shq; ++l)
        if (int rc = ensure_shadow_workspace(c, c->ws[l].b, bp.ncap)) return rc;
    for (int l = 0; l < pp.lanes && pp.nee; ++l)
        if (int rc = ensure_nee_workspace(c, c->ws[l].b, bp.nmax * (size_t)(nee_stride(p.sc.n_lights) + nee_extra_f4(rgh_level(pp), p.sc.n_lights)), bp.ncap)) return rc;
    return RT_OK;
}

// lane l takes the batch of indices [b0, min(b0 + B, ie)) and generates its camera rays
int stage_generate(const PathPass& p, Lane& L, int l, int b0, int ie, hipStream_t st) {
    rt_ctx* c = p.c;
    L.w = &c->ws[l];
    L.s = l == 0 ? st : L.w->stream;
    L.sc = lane_scene(p.sc, *L.w);
    L.rv = RecView{L.w->b.rec.get(), p.pp.rec_fs, p.pp.rec_ss, p.pp.rec_rng8};
    L.ids = sample_ids(p.target.work, p.target.n, b0);
    L.nIdx = std::min(p.bp.B, ie - b0);
    L.nS = L.nIdx * p.target.n;
    L.S = shard_stride(L.nS, p.bp.nsh);
    L.cur = 0;
    const Batch& b = L.w->b;
    GenOut go{b.rayO(), b.rayD(), nullptr, nullptr, b.pdfA.get(), b.pdfB.get(), L.rv, p.pp.lean, 1};
    // camera rays fill queue 0 densely (positions 0..nS-1: QueueView without lengths); both counter regions
    // start at zero: k_generate zeroes them (a memset launch here waited for the other lane's resident blocks
    // in two-lane mode, r05 kernel traces)
    go.zero = L.w->qcount.get();
    hipEvent_t e0 = ev_start(c, L.s);
    HIPCHK(c, launch_generate(L.s, c->grid, L.nS, L.ids, p.cam, p.smp, p.fd, go));
    ev_mark(c, L.s, ST_GEN, e0);
    return RT_OK;
}

// emitter filter, coherence sort, the trace and its fallback
int stage_trace(const PathPass& p, const Lane& L, Bounce& bo) {
    rt_ctx* c = p.c;
    const Batch& b = L.w->b;
    const DepthPlan& d = bo.d;
    const Knobs& kn = c->knobs;
    bo.qc_cur = L.counters(L.cur);
    bo.qc_nxt = L.counters(L.cur ^ 1);
    bo.cO = L.rays(p, L.cur);
    bo.qv = bo.depth == 0 ? QueueView{nullptr, L.S, L.nS, p.bp.nsh} : QueueView{bo.qc_cur + kQLen, L.S, 0, p.bp.nsh};
    hipEvent_t e0;
    // the next queue's length and the chunk tickets its trace and shade launches will use start at zero: depth 0
    // (k_generate zeroed both regions) / the trace kernel zeroes it (below), except before the emitter filter, which
    // appends to it ahead of the trace: its survivors go into the free next queue, whose rays the trace and shade
    // kernels then take (the shade appends nothing at this depth)
    if (d.efilter) {
        HIPCHK(c, hipMemsetAsync(bo.qc_nxt, 0, kQRegion * sizeof(int), L.s));
        const EmitIO eio{bo.qv, bo.cO, L.rays(p, L.cur ^ 1), bo.qc_nxt + kQLen};
        e0 = ev_start(c, L.s);
        HIPCHK(c, launch_emitter_filter(L.s, c->grid, L.sc, eio));
        ev_mark(c, L.s, ST_FILTER, e0);
        bo.cO = eio.nO;
        bo.qv = QueueView{bo.qc_nxt + kQLen, L.S, 0, p.bp.nsh};
    }
    TraceIO& tio = bo.tio;
    tio = TraceIO{bo.cO, bo.cO + 1, bo.qv, 0, b.hitB.get(), b.hitPrim.get(),
                  p.bp.dyn ? bo.qc_cur + kQTraceTicket : nullptr, 1};
    if (bo.depth > 0 && !d.efilter) tio.zero = bo.qc_nxt;
    // packed hit records, depth 0: the hit word (prim, flip, front) in hitB's w lane, so the shade reads hitB alone
    // (no hitPrim, no ray).  Nothing else reads this depth's hits on the simple path.
    if (d.pack0) tio.hq_pack = 1;
    // the hit queue's length word is this queue's shadow-queue length, which single-leaf scenes never use (zero before
    // the launch like the rest of the region)
    if (d.hit_compact) {
        if (d.hit_pack) tio.hq_pack = 1;
        else tio.hq_d = b.hitD.get();
        tio.hq_len = bo.qc_cur + kQShadowLen;
    }
    if (p.bp.dyn) {  // ambiguous rays listed for k_trace_fallback
        tio.fb_pos = L.w->tfb.get();
        tio.fb_len = bo.qc_cur + kQTraceFallback;
    }
    // multi-level octrees: bounce rays sorted by (octant, direction cell, origin Morton code) before the trace.  The
    // device reads the queue length itself, so only live rays are sorted and the host reads nothing back (sorting the
    // capacity with padded keys: -0.6 %)
    if (d.sort) {
        SortRaysIO so{b.sQKey.get(), b.sS.get(), b.sKeys.get(), b.sKeysAlt.get(), b.sVals.get(), b.sValsAlt.get(),
                      b.sTemp.get(), kn.sort_dir_bits, kn.sort_org_bits, bo.qc_cur + kQLen, L.S};
        e0 = ev_start(c, L.s);
        HIPCHK(c, launch_sort_rays(L.s, so));
        ev_mark(c, L.s, ST_SORT, e0);
        tio.perm = b.sS.get();  // the trace kernel gathers the sorted rays into the side queue
        tio.so = b.sRay.get();
        bo.cO = tio.so;
    }
    return trace_with_fallback(c, L.s, L.sc, tio, d.trace_fallback);
}

// the media's absorb stage of this depth: over the queue the trace just wrote, before the shade (and
// before k_bin_materials) reads beta, so the vertex's own light terms carry the attenuation.  Timed with the shade stage,
// as the miss stage is.
int stage_absorb(const PathPass& p, const Lane& L, const Bounce& bo) {
    rt_ctx* c = p.c;
    if (!bo.d.absorb) return RT_OK;
    const Batch& b = L.w->b;
    const MediumIO mio{bo.qv, bo.cO, b.hitB.get(), b.hitPrim.get(), L.rv, bo.depth, L.sc.triWorld, L.sc.triMaterial,
                       L.sc.shapes, L.sc.n_tris, c->med.table.get(), (int)c->med.bound.size(), c->med.ctr.get()};
    hipEvent_t e0 = ev_start(c, L.s);
    HIPCHK(c, launch_medium_absorb(L.s, c->grid, mio));
    ++c->med.launches;
    ev_mark(c, L.s, ST_SHADE, e0);
    return RT_OK;
}

// the shade's arguments over the traced rays: PathIO, the shadow queue, the NEE queue
void shade_io(const PathPass& p, const Lane& L, Bounce& bo) {
    const rt_ctx* c = p.c;
    const Batch& b = L.w->b;
    const PathPlan& pp = p.pp;
    const Knobs& kn = c->knobs;
    PathIO& pio = bo.pio;
    pio.lean = pp.lean;
    pio.rayO = bo.cO; pio.rayD = bo.cO + 1; pio.q = bo.qv;
    pio.hitB = b.hitB.get(); pio.hitPrim = b.hitPrim.get();
    if (bo.d.hit_compact) {  // items = the hit records (PathIO hq_d)
        pio.q = QueueView{bo.tio.hq_len, L.S, 0, p.bp.nsh};
        pio.hq_d = bo.tio.hq_d;
    }
    pio.nO = L.rays(p, L.cur ^ 1); pio.nD = pio.nO + 1;
    pio.nCount = bo.qc_nxt + kQLen;
    pio.rec = L.rv; pio.pdfA = b.pdfA.get(); pio.pdfB = b.pdfB.get();
    pio.depth = bo.depth; pio.max_depth = pp.max_depth;
    pio.dim = -1;
    if (pp.lean == 1) {
        pio.dim = dim_after_camera(p.smp, p.cam);
        for (int d = 0; d < bo.depth; ++d) pio.dim = dim_get2d(p.smp, dim_get2d(p.smp, pio.dim));
    }
    pio.ticket = p.bp.dyn ? bo.qc_cur + kQShadeTicket : nullptr;
    if (bo.d.next_keys) {  // keys of the rays this shade appends (next sort)
        pio.nkey.key = b.sQKey.get();
        pio.nkey.lo = c->sort_lo;
        pio.nkey.scale = c->sort_scale;
        pio.nkey.dir_bits = kn.sort_dir_bits;
        pio.nkey.org_bits = kn.sort_org_bits;
        pio.nkey.org_major = pp.org_major;
    }
    if (pp.shq) {  // this queue's region holds the shadow-queue length and ticket (zeroed with it)
        ShadowQueueIO& sq = bo.sqio;
        sq.shO = b.shO.get(); sq.shD = b.shD.get(); sq.shLA = b.shLA.get(); sq.shLB = b.shLB.get();
        sq.shCount = bo.qc_cur + kQShadowLen;
        sq.shTicket = bo.qc_cur + kQShadowTicket;
        sq.defer = pp.defer;
    }
    if (pp.nee)
        bo.nio = NeeIO{b.neeRec.get(), b.nee.queue, bo.qc_cur + kQShadowLen, bo.qc_cur + kQShadowTicket, b.nee.fallback,
                       bo.qc_cur + kQNeeFallback, pp.sort_nee ? b.nee.key : nullptr, c->sort_lo, c->sort_scale,
                       kn.sort_nee_bits};
    if (c->tx.live) bo.nio.tex = c->tx.dev.get();
    bo.nio.ml = pp.ml;
}

// the shade: one kernel, or the hits binned by material and one kernel per bin over its index list
int stage_shade(const PathPass& p, const Lane& L, Bounce& bo) {
    rt_ctx* c = p.c;
    const Batch& b = L.w->b;
    shade_io(p, L, bo);
    const DevSpectra* const d_spec = c->d_spec.get();
    hipEvent_t e0 = ev_start(c, L.s);
    if (p.pp.bins) {
        BinIO bio{bo.qv, b.hitPrim.get(), {}, bo.qc_cur + kQBinLen};
        for (int cl = 0; cl < kMatClasses; ++cl) bio.idx[cl] = b.nee.bin[cl];
        if (bo.depth == 0) { bio.rayO = bo.cO; bio.rec = L.rv; }  // lean depth 0: the misses' L = 0 (BinIO)
        HIPCHK(c, launch_bin_materials(L.s, c->grid, L.sc, bio));
        for (int cl = 0; cl < kMatClasses; ++cl) {
            PathIO bp = bo.pio;
            bp.q = QueueView{bo.qc_cur + kQBinLen + cl * kShards * kQStride, L.S, 0, p.bp.nsh};
            bp.ticket = bo.qc_cur + kQBinTicket + cl * kShards * kQStride;
            bp.bin_idx = bio.idx[cl];
            HIPCHK(c, launch_path_shade(L.s, c->grid, L.sc.qcap, L.sc, d_spec, p.smp, p.fd, L.ids, bp, c->d_ctr.get(),
                                        bo.sqio, bo.nio, 1 + cl));
            if (p.pp.rgh && cl == 0) ++c->rgh_launches[0];  // (the specular bin has no RGH instantiation)
            if (p.pp.cnd && cl == 0) ++c->cnd_launches[0];
            if (p.pp.rgl && cl == 0) ++c->rgl_launches[0];
        }
    } else {
        HIPCHK(c, launch_path_shade(L.s, c->grid, L.sc.qcap, L.sc, d_spec, p.smp, p.fd, L.ids, bo.pio, c->d_ctr.get(),
                                    bo.sqio, bo.nio, 0, p.pp.hit_pack));
        if (p.pp.rgh && p.pp.nee) ++c->rgh_launches[0];
        if (p.pp.cnd && p.pp.nee) ++c->cnd_launches[0];
        if (p.pp.rgl && p.pp.nee) ++c->rgl_launches[0];
    }
    ev_mark(c, L.s, ST_SHADE, e0);
    return RT_OK;
}

// the environment light's misses of this depth: over the queue the shade just read.  A missed slot gets
// no other addition at this depth (the shade and the NEE kernels touch hits only), so the order of its sums is fixed.
// Timed with the shade stage (rt_stats has no field of its own for it).
int stage_env_miss(const PathPass& p, const Lane& L, const Bounce& bo) {
    rt_ctx* c = p.c;
    if (!bo.d.env_miss) return RT_OK;
    const EnvMissIO eio{bo.qv, bo.cO, L.w->b.hitPrim.get(), L.rv, bo.depth, p.pp.lean, p.bp.mis ? 1 : 0, c->env.dev};
    hipEvent_t e0 = ev_start(c, L.s);
    HIPCHK(c, launch_env_miss(L.s, c->grid, c->d_spec.get(), eio));
    ev_mark(c, L.s, ST_ENVMISS, e0);
    return RT_OK;
}

// mixed scenes: the NEE queue's sort, this bounce's shadow rays (before the next bounce reads L), their fallback
int stage_nee(const PathPass& p, const Lane& L, const Bounce& bo) {
    rt_ctx* c = p.c;
    const Batch& b = L.w->b;
    if (!p.pp.nee) return RT_OK;
    hipEvent_t e0;
    if (p.pp.sort_nee) {  // (no host round trip)
        SortNeeIO so{b.nee.queue, bo.qc_cur + kQShadowLen, L.S, b.nee.key, b.sKeys.get(), b.sKeysAlt.get(),
                     b.sVals.get(), b.sValsAlt.get(), b.sTemp.get(), c->knobs.sort_nee_bits};
        e0 = ev_start(c, L.s);
        HIPCHK(c, launch_sort_nee(L.s, so));
        ev_mark(c, L.s, ST_SORT, e0);
    }
    e0 = ev_start(c, L.s);
    HIPCHK(c, launch_path_nee(L.s, c->grid, L.sc.qcap, L.sc, c->d_spec.get(), bo.pio, bo.nio, c->d_ctr.get()));
    if (bo.d.nee_fallback)
        HIPCHK(c, launch_path_nee_fallback(L.s, c->grid, L.sc.qcap, L.sc, c->d_spec.get(), bo.pio, bo.nio, c->d_ctr.get()));
    if (p.pp.rgh) c->rgh_launches[1] += bo.d.nee_fallback ? 2 : 1;
    if (p.pp.cnd) c->cnd_launches[1] += bo.d.nee_fallback ? 2 : 1;
    if (p.pp.rgl) c->rgl_launches[1] += bo.d.nee_fallback ? 2 : 1;
    ev_mark(c, L.s, ST_SHADOW, e0);
    return RT_OK;
}

// multi-level simple scenes: the queued shadow rays
int stage_shadow(const PathPass& p, const Lane& L, const Bounce& bo) {
    rt_ctx* c = p.c;
    if (!bo.d.shadow) return RT_OK;
    hipEvent_t e0 = ev_start(c, L.s);
    HIPCHK(c, launch_path_shadow(L.s, c->grid, L.sc.qcap, c->knobs.shadow_dfs != 0, L.sc, bo.pio, bo.sqio, c->d_ctr.get()));
    ev_mark(c, L.s, ST_SHADOW, e0);
    return RT_OK;
}

// the batch's samples into the film, after the previous batch's (after: the lane of the most recent film launch)
int stage_film(const PathPass& p, const Lane& L, const Work* after) {
    rt_ctx* c = p.c;
    const Batch& b = L.w->b;
    if (after && after != L.w) HIPCHK(c, hipStreamWaitEvent(L.s, after->film_done, 0));
    PathFilmIO fio{p.target.work, p.target.n, L.nIdx, L.rv, b.pdfA.get(), b.pdfB.get(), p.film};
    fio.lean = p.pp.lean;
    fio.mom = p.target.mom;
    hipEvent_t e0 = ev_start(c, L.s);
    HIPCHK(c, launch_path_film(L.s, 0, c->d_spec.get(), p.fd, fio, c->d_ctr.get()));
    ev_mark(c, L.s, ST_FILM, e0);
    HIPCHK(c, hipEventRecord(L.w->film_done, L.s));
    return RT_OK;
}

int render_path(rt_ctx* c, const PassFacts& f, const BatchPlan& bp, int ib, int ie, float4* film, hipStream_t st,
                const PassTarget& pass) {
    const PathPass p{c, bp, plan_path(f, c->knobs, bp), pass_scene(c, bp), dev_camera(c->cam), dev_sampler(c),
                     dev_film(c), pass, film};
    const int lanes = p.pp.lanes;
    int rc;
    c->rgh_launches[0] = c->rgh_launches[1] = 0;
    c->cnd_launches[0] = c->cnd_launches[1] = 0;
    c->rgl_launches[0] = c->rgl_launches[1] = 0;
    c->med.launches = 0;
    c->med.counted = p.pp.med;
    if (p.pp.med) {  // the segment counter of this pass (ahead of every lane: they start after st)
        HIPCHK(c, c->med.ctr.reserve(kMediumCtrWords));
        HIPCHK(c, hipMemsetAsync(c->med.ctr.get(), 0, kMediumCtrWords * sizeof(unsigned long long), st));
    }
    if ((rc = path_workspaces(p))) return rc;
    if (lanes > 1) {  // lanes 1.. start after the caller's earlier work on st
        HIPCHK(c, hipEventRecord(c->ws[0].film_done, st));
        for (int l = 1; l < lanes; ++l) HIPCHK(c, hipStreamWaitEvent(c->ws[l].stream, c->ws[0].film_done, 0));
    }
    const Work* last_film = nullptr;  // lane of the most recent film launch
    for (int g0 = ib; g0 < ie; g0 += bp.B * lanes) {
        Lane lane[kLanes];
        int n = 0;  // lanes with a batch in this round
        for (; n < lanes && g0 + n * bp.B < ie; ++n)
            if ((rc = stage_generate(p, lane[n], n, g0 + n * bp.B, ie, st))) return rc;
        for (int depth = 0; p.pp.at(depth).traced; ++depth)
            for (int l = 0; l < n; ++l) {
                Lane& L = lane[l];
                Bounce bo{depth, p.pp.at(depth)};
                if ((rc = stage_trace(p, L, bo)) || (rc = stage_absorb(p, L, bo)) || (rc = stage_shade(p, L, bo)) ||
                    (rc = stage_env_miss(p, L, bo)) ||
                    (rc = stage_nee(p, L, bo)) ||
                    (rc = stage_shadow(p, L, bo)))
                    return rc;
                L.cur ^= 1;
            }
        for (int l = 0; l < n; ++l) {
            if ((rc = stage_film(p, lane[l], last_film))) return rc;
            last_film = lane[l].w;
        }
    }
    // the caller's stream resumes after every lane's last film
    for (int l = 1; l < lanes; ++l) HIPCHK(c, hipStreamWaitEvent(st, c->ws[l].film_done, 0));
    return RT_OK;
}

int render_device_body(rt_ctx* c, int ib, int ie, float4* film, hipStream_t st, const PassTarget& pass) {
    if (int rc = pass_checks(c, ib, ie)) return rc;
    const PassFacts f = pass_facts(c, pass.n, ib, ie);
    const BatchPlan bp = plan_batches(f, c->knobs);
    if (!bp.nbatch) return RT_OK;
    return bp.path ? render_path(c, f, bp, ib, ie, film, st, pass) : render_reference(c, bp, ib, ie, film, st, pass);
}

// ---------------------------------------------------------------------------------- PixelSensor (a18, a20)
// glm float order throughout: mat3 is column-major (m[col * 3 + row]); inverse = glm's cofactor form; products
// sum (a0 b0 + a1 b1) + a2 b2.
void inv3(const float* a, float* o) {
    auto m = [&](int col, int row) { return a[col * 3 + row]; };
    float ood = 1.0f / (+m(0, 0) * (m(1, 1) * m(2, 2) - m(2, 1) * m(1, 2)) -
                        m(1, 0) * (m(0, 1) * m(2, 2) - m(2, 1) * m(0, 2)) +
                        m(2, 0) * (m(0, 1) * m(1, 2) - m(1, 1) * m(0, 2)));
    o[0] = +(m(1, 1) * m(2, 2) - m(2, 1) * m(1, 2)) * ood;
    o[3] = -(m(1, 0) * m(2, 2) - m(2, 0) * m(1, 2)) * ood;
    o[6] = +(m(1, 0) * m(2, 1) - m(2, 0) * m(1, 1)) * ood;
    o[1] = -(m(0, 1) * m(2, 2) - m(2, 1) * m(0, 2)) * ood;
    o[4] = +(m(0, 0) * m(2, 2) - m(2, 0) * m(0, 2)) * ood;
    o[7] = -(m(0, 0) * m(2, 1) - m(2, 0) * m(0, 1)) * ood;
    o[2] = +(m(0, 1) * m(1, 2) - m(1, 1) * m(0, 2)) * ood;
    o[5] = -(m(0, 0) * m(1, 2) - m(1, 0) * m(0, 2)) * ood;
    o[8] = +(m(0, 0) * m(1, 1) - m(1, 0) * m(0, 1)) * ood;
}
void mul3(const float* A, const float* B, float* o) {
    for (int col = 0; col < 3; ++col)
        for (int r = 0; r < 3; ++r)
            o[col * 3 + r] = (A[0 * 3 + r] * B[col * 3 + 0] + A[1 * 3 + r] * B[col * 3 + 1]) + A[2 * 3 + r] * B[col * 3 + 2];
}

// Spectra::Init's named illuminants (spectrum.cpp:2620-2637): FromInterleaved(.., normalize = true)
PLS named_illuminant(const HostSpectra& hs, int which) {
    static const float* const tab[] = {rtdata::illum_d65, rtdata::illum_a, rtdata::illum_d50, rtdata::illum_f1,
                                       rtdata::illum_f2, rtdata::illum_f3, rtdata::illum_f4, rtdata::illum_f5,
                                       rtdata::illum_f6, rtdata::illum_f7, rtdata::illum_f8, rtdata::illum_f9,
                                       rtdata::illum_f10, rtdata::illum_f11, rtdata::illum_f12, rtdata::illum_aces_d60};
    static const int n[] = {rtdata::illum_d65_n, rtdata::illum_a_n, rtdata::illum_d50_n, rtdata::illum_f1_n,
                            rtdata::illum_f2_n, rtdata::illum_f3_n, rtdata::illum_f4_n, rtdata::illum_f5_n,
                            rtdata::illum_f6_n, rtdata::illum_f7_n, rtdata::illum_f8_n, rtdata::illum_f9_n,
                            rtdata::illum_f10_n, rtdata::illum_f11_n, rtdata::illum_f12_n, rtdata::illum_aces_d60_n};
    return hs.interleaved(tab[which], n[which], true);
}

// pixelsensor.h:104-117 ProjectReflectance: (b_i(λ) refl(λ)) illum(λ) summed over λ = 360..830 (float loop),
// divided by Σ b2(λ) illum(λ)
template <class R, class I, class B1, class B2, class B3>
F3 project_reflectance(const R& refl, const I& illum, const B1& b1, const B2& b2, const B3& b3) {
    float g = 0, r0 = 0, r1 = 0, r2 = 0;
    for (float l = 360; l <= 830; ++l) {
        g += b2.query(l) * illum.query(l);
        r0 += b1.query(l) * refl.query(l) * illum.query(l);
        r1 += b2.query(l) * refl.query(l) * illum.query(l);
        r2 += b3.query(l) * refl.query(l) * illum.query(l);
    }
    return F3{r0 / g, r1 / g, r2 / g};
}

// XYZFromSensorRGB (pixelsensor.h:37-79) and the sRGB RGBFromXYZ (colorspace.cpp:13-28) of a film description,
// plus the sensor's dense r/g/b curves.
void sensor_matrices(const HostSpectra& hs, int sensor, int illum_id, float* xyz_from_sensor, float* rgb_from_xyz,
                     DenseS bars[3]) {
    auto xyz_of = [&](const PLS& s) {  // SpectrumToXYZ
        float X = inner_product(hs.X, s), Y = inner_product(hs.Y, s), Z = inner_product(hs.Z, s);
        return F3{X / 106.856895f, Y / 106.856895f, Z / 106.856895f};
    };
    auto xy_of = [](F3 c) { return std::pair<float, float>{c.x / (c.x + c.y + c.z), c.y / (c.x + c.y + c.z)}; };
    auto xyY = [](float x, float y) { return y == 0 ? F3{0, 0, 0} : F3{x * 1.0f / y, 1.0f, (1 - x - y) * 1.0f / y}; };
    // sRGB (colorspace.cpp:91-106): primaries, white = the D65 illuminant's xy
    F3 W = xyz_of(hs.D65);
    auto w = xy_of(W);
    F3 R = xyY((float).64, (float).33), G = xyY((float).3, (float).6), Bp = xyY((float).15, (float).06);
    float rgb[9] = {R.x, R.y, R.z, G.x, G.y, G.z, Bp.x, Bp.y, Bp.z}, irgb[9];
    inv3(rgb, irgb);
    F3 Cw = m3v(irgb, W);
    float dg[9] = {Cw.x, 0, 0, 0, Cw.y, 0, 0, 0, Cw.z}, xyzFromRgb[9];
    mul3(rgb, dg, xyzFromRgb);
    inv3(xyzFromRgb, rgb_from_xyz);
    PLS illum = named_illuminant(hs, illum_id);
    if (sensor == RT_SENSOR_XYZ) {
        bars[0] = hs.X; bars[1] = hs.Y; bars[2] = hs.Z;
        // pixelsensor.h:70-79: WhiteBalance(SpectrumToXYZ(sensorIllum).xy, sRGB.w) (color.h:616-629, Bradford)
        float lmsFromXyz[9] = {(float)0.8951, (float)-0.7502, (float)0.0389, (float)0.2664, (float)1.7135,
                               (float)-0.0685, (float)-0.1614, (float)0.0367, (float)1.0296};
        float xyzFromLms[9] = {(float)0.986993, (float)0.432305, (float)-0.00852866, (float)-0.147054, (float)0.51836,
                               (float)0.0400428, (float)0.159963, (float)0.0492912, (float)0.968487};
        auto sw = xy_of(xyz_of(illum));
        F3 src = xyY(sw.first, sw.second), dst = xyY(w.first, w.second);
        F3 sl = m3v(lmsFromXyz, src), dl = m3v(lmsFromXyz, dst);
        float corr[9] = {dl.x / sl.x, 0, 0, 0, dl.y / sl.y, 0, 0, 0, dl.z / sl.z}, t1[9];
        mul3(xyzFromLms, corr, t1);
        mul3(t1, lmsFromXyz, xyz_from_sensor);
        return;
    }
    // camera curves: PiecewiseLinearSpectrum::FromInterleaved(.., false) sampled densely (pixelsensor.h:41)
    int cam = sensor - 1;
    for (int ch = 0; ch < 3; ++ch)
        bars[ch] = to_dense(hs.interleaved(rtdata::camera_curves[cam][ch], rtdata::camera_curves_n[cam][ch], false));
    float rgbCamera[24][3], xyzOutput[24][3];
    for (int i = 0; i < 24; ++i) {
        PLS sw = hs.interleaved(rtdata::swatches[i], rtdata::swatches_n[i], false);
        F3 c3 = project_reflectance(sw, illum, bars[0], bars[1], bars[2]);
        rgbCamera[i][0] = c3.x; rgbCamera[i][1] = c3.y; rgbCamera[i][2] = c3.z;
    }
    float sensorWhiteG = inner_product(illum, bars[1]);
    float sensorWhiteY = inner_product(illum, hs.Y);
    for (int i = 0; i < 24; ++i) {
        PLS sw = hs.interleaved(rtdata::swatches[i], rtdata::swatches_n[i], false);
        F3 x3 = project_reflectance(sw, hs.D65d, hs.X, hs.Y, hs.Z);  // outputColorSpace->illuminant (dense D65)
        float k = sensorWhiteY / sensorWhiteG;
        xyzOutput[i][0] = x3.x * k; xyzOutput[i][1] = x3.y * k; xyzOutput[i][2] = x3.z * k;
    }
    // helpers.h:258-272 LinearLeastSquares<3>: AtA[i][j] / AtB[i][j] are glm [column i][row j]
    float AtA[9] = {0}, AtB[9] = {0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            for (int r = 0; r < 24; ++r) {
                AtA[i * 3 + j] += rgbCamera[r][i] * rgbCamera[r][j];
                AtB[i * 3 + j] += rgbCamera[r][i] * xyzOutput[r][j];
            }
    float AtAi[9], P[9];
    inv3(AtA, AtAi);
    mul3(AtAi, AtB, P);
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) xyz_from_sensor[c * 3 + r] = P[r * 3 + c];  // glm::transpose
}

int setup_sensor(rt_ctx* c, const rt_film_desc& d) {
    c->alb.valid = false;  // (the albedo table is baked under the sensor's curves)
    DenseS bars[3];
    sensor_matrices(c->hs, d.sensor, d.sensor_illum, c->resolveA, c->resolveB, bars);
    float both[18];
    std::memcpy(both, c->resolveA, 36);
    std::memcpy(both + 9, c->resolveB, 36);
    char* base = (char*)c->d_spec.get();
    if (hipMemcpy(c->d_resolve.get(), both, sizeof(both), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(base + offsetof(DevSpectra, SR), bars[0].v.data(), 4 * kSpecN, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(base + offsetof(DevSpectra, SG), bars[1].v.data(), 4 * kSpecN, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(base + offsetof(DevSpectra, SB), bars[2].v.data(), 4 * kSpecN, hipMemcpyHostToDevice) != hipSuccess)
        return fail(c, RT_E_HIP, "sensor upload");
    std::vector<float4> spk(kSpecN);
    for (int i = 0; i < kSpecN; ++i)
        spk[i] = make_float4(bars[0].v[i], bars[1].v[i], bars[2].v[i], c->hs.D65d.v[i]);
    if (hipMemcpy(base + offsetof(DevSpectra, SPK), spk.data(), sizeof(float4) * kSpecN, hipMemcpyHostToDevice) !=
        hipSuccess)
        return fail(c, RT_E_HIP, "sensor upload");
    return RT_OK;
}


// ---- multi-device pass (rt_options.n_devices > 1).  Device 0 packs each peer's owned pixels of the
// caller's film into that peer's exchange buffer; the peer copies them over xGMI, scatters them into its own film,
// renders its tiles (the same kernels, the same per-pixel index order), packs them and copies them back; device 0
// scatters them into the caller's film.  Pure copies: the film is bit-identical to a one-device render.
int peer_prepare(rt_ctx* c, size_t j) {
    rt_ctx* p = c->peers[j];
    rt_ctx::PeerLink& L = c->links[j];
    hipSetDevice(p->device);
    int rc = build_work(p);
    if (rc) return fail(c, rc, "device " + std::to_string(p->device) + ": " + p->err);
    size_t n = (size_t)p->film.res_x * p->film.res_y;
    HIPCHK(c, p->d_film.reserve(n));
    HIPCHK(c, p->xfer.reserve((size_t)p->n_work));
    hipSetDevice(c->device);
    if (L.epoch != p->work_epoch) {
        HIPCHK(c, L.work0.reserve((size_t)p->n_work));
        HIPCHK(c, L.xfer0.reserve((size_t)p->n_work));
        HIPCHK(c, hipMemcpyPeer(L.work0.get(), c->device, p->d_work.get(), p->device, sizeof(int) * p->n_work));
        L.n = p->n_work;
        L.epoch = p->work_epoch;
    }
    return RT_OK;
}

// the peer's half of a pass, on its own stream (runs in its own host thread: multi-level octrees sort with a
// host round trip per bounce, which must not serialise the devices)
int peer_pass(rt_ctx* c, size_t j, int ib, int ie) {
    rt_ctx* p = c->peers[j];
    const rt_ctx::PeerLink& L = c->links[j];
    hipSetDevice(p->device);
    hipStream_t ps = p->stream;
    const size_t bytes = sizeof(float4) * L.n;
    HIPCHK(p, hipStreamWaitEvent(ps, c->gathered, 0));
    if (L.n) {
        HIPCHK(p, hipMemcpyPeerAsync(p->xfer.get(), p->device, L.xfer0.get(), c->device, bytes, ps));
        HIPCHK(p, launch_film_scatter(ps, L.n, p->d_work.get(), p->xfer.get(), p->d_film.get()));
    }
    int rc = render_device(p, ib, ie, p->d_film.get(), ps);
    if (rc) return rc;
    if (L.n) {
        HIPCHK(p, launch_film_gather(ps, L.n, p->d_work.get(), p->d_film.get(), p->xfer.get()));
        HIPCHK(p, hipMemcpyPeerAsync(L.xfer0.get(), c->device, p->xfer.get(), p->device, bytes, ps));
    }
    HIPCHK(p, hipEventRecord(p->gathered, ps));
    return RT_OK;
}

int render_multi(rt_ctx* c, int ib, int ie, float4* film, hipStream_t st) {
    if (c->peers.empty()) return render_device(c, ib, ie, film, st);
    int rc = check_ready(c);
    if (rc) return rc;
    if (ib < 0 || ie < ib) return fail(c, RT_E_ARG, "invalid index range");
    for (size_t j = 0; j < c->peers.size(); ++j)
        if ((rc = peer_prepare(c, j))) return rc;
    hipSetDevice(c->device);
    for (const rt_ctx::PeerLink& L : c->links)
        if (L.n) HIPCHK(c, launch_film_gather(st, L.n, L.work0.get(), film, L.xfer0.get()));
    HIPCHK(c, hipEventRecord(c->gathered, st));
    std::vector<int> prc(c->peers.size(), RT_OK);
    std::vector<std::thread> th;
    th.reserve(c->peers.size());
    for (size_t j = 0; j < c->peers.size(); ++j) th.emplace_back([&, j] { prc[j] = peer_pass(c, j, ib, ie); });
    rc = render_device(c, ib, ie, film, st);
    for (std::thread& t : th) t.join();
    hipSetDevice(c->device);
    if (rc) return rc;
    for (size_t j = 0; j < c->peers.size(); ++j)
        if (prc[j]) return fail(c, prc[j], "device " + std::to_string(c->peers[j]->device) + ": " + c->peers[j]->err);
    for (size_t j = 0; j < c->peers.size(); ++j) {
        const rt_ctx::PeerLink& L = c->links[j];
        HIPCHK(c, hipStreamWaitEvent(st, c->peers[j]->gathered, 0));
        if (L.n) HIPCHK(c, launch_film_scatter(st, L.n, L.work0.get(), L.xfer0.get(), film));
    }
    return RT_OK;
}

}  // namespace

// =========================================================================================== C-ABI
extern "C" {

int rt_abi_version(void) { return RT_ABI_VERSION; }

static void destroy_one(rt_ctx* c);

static int create_one(const rt_options* opt, rt_ctx** out) {
    if (!out) return RT_E_ARG;
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return RT_E_NODEVICE;
    int dev = opt ? opt->device : 0;
    if (dev < 0 || dev >= ndev) return RT_E_ARG;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return RT_E_HIP;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return RT_E_NODEVICE;
    rt_ctx* c = new rt_ctx();
    c->device = dev;
    c->octree_build = opt ? opt->octree_build : RT_OCTREE_BUILD_DEVICE;
    if (hipSetDevice(dev) != hipSuccess || hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
        delete c;
        return RT_E_HIP;
    }
    c->grid = prop.multiProcessorCount * 8;  // persistent grid: 8 blocks of 256 per CU
    c->knobs = read_knobs();
    c->hs.init();
    if (c->d_spec.reserve(1) != hipSuccess || c->ws[0].qcount.reserve(2 * kQRegion) != hipSuccess ||
        c->d_ctr.reserve(kCtrWords) != hipSuccess || c->d_resolve.reserve(18) != hipSuccess) {
        destroy_one(c);
        return RT_E_OOM;
    }
    DevSpectra ds{};
    std::memcpy(ds.X, c->hs.X.v.data(), 4 * kSpecN);
    std::memcpy(ds.Y, c->hs.Y.v.data(), 4 * kSpecN);
    std::memcpy(ds.Z, c->hs.Z.v.data(), 4 * kSpecN);
    std::memcpy(ds.D65, c->hs.D65d.v.data(), 4 * kSpecN);
    ds.f1_n = (int)c->hs.F1.l.size();
    std::memcpy(ds.f1_lambda, c->hs.F1.l.data(), 4 * ds.f1_n);
    std::memcpy(ds.f1_value, c->hs.F1.v.data(), 4 * ds.f1_n);
    ds.bk7_n = (int)c->hs.BK7.l.size();
    std::memcpy(ds.bk7_lambda, c->hs.BK7.l.data(), 4 * ds.bk7_n);
    std::memcpy(ds.bk7_value, c->hs.BK7.v.data(), 4 * ds.bk7_n);
    static_assert(sizeof(ds.NK) == sizeof(float) * 2 * kMetals * kMetalSpecN && kMetalSpecN == kSpecN, "NK layout");
    std::memcpy(ds.NK, metal_nk_table().data(), sizeof(ds.NK));
    hipMemcpy(c->d_spec.get(), &ds, sizeof(ds), hipMemcpyHostToDevice);
    hipMemset(c->d_ctr.get(), 0, sizeof(unsigned long long) * kCtrWords);
    {
        rt_film_desc fd{};  // XYZ sensor under D65 until rt_film_set says otherwise
        if (setup_sensor(c, fd) != RT_OK) {
            destroy_one(c);
            return RT_E_HIP;
        }
    }
    *out = c;
    return RT_OK;
}

static void destroy_one(rt_ctx* c) {
    if (!c) return;
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);
    for (Work& w : c->ws)
        if (w.stream) hipStreamSynchronize(w.stream);
    harvest(c);
    for (hipEvent_t e : c->pool) hipEventDestroy(e);
    for (Work& w : c->ws) {
        if (w.film_done) hipEventDestroy(w.film_done);
        if (w.stream) hipStreamDestroy(w.stream);
    }
    if (c->done) hipEventDestroy(c->done);
    if (c->gathered) hipEventDestroy(c->gathered);
    if (c->stream) hipStreamDestroy(c->stream);
    delete c;  // every DevBuf member, while c->device is current
}

const char* rt_last_error(const rt_ctx* c) { return c ? c->err.c_str() : "null context"; }

// World-space triangles of a (validated) scene: ObjectToRender * vec4(p,1) per vertex (= the per-test transform,
// Shapes.h:1117-1122), back-face flags (Shapes.h:1339-1380) and degenerate flags (Shapes.h:1131).
struct SceneWorld {
    std::vector<F3> wv, tri3;
    std::vector<uint8_t> back, degen;
};
static void scene_world(const rt_scene_desc* s, SceneWorld& w) {
    const int nt = s->n_triangles, nv = s->n_vertices;
    w.wv.resize(nv);
    for (int i = 0; i < nv; ++i) {
        float o[4];
        m4v(s->object_to_render, s->positions[3 * i], s->positions[3 * i + 1], s->positions[3 * i + 2], 1.f, o);
        w.wv[i] = {o[0], o[1], o[2]};
    }
    w.tri3.resize(3 * (size_t)nt);
    for (int t = 0; t < nt; ++t)
        for (int k = 0; k < 3; ++k) w.tri3[3 * (size_t)t + k] = w.wv[s->indices[3 * t + k]];
    w.back.assign(nt, 0);
    w.degen.assign(nt, 0);
    const bool cull = s->cull_backfaces != 0;
    F3 look = f3norm({s->cull_look[0], s->cull_look[1], s->cull_look[2]});
    for (int t = 0; t < nt; ++t) {
        const F3* p = &w.tri3[3 * (size_t)t];
        F3 cr = f3cross(f3sub(p[2], p[0]), f3sub(p[1], p[0]));
        w.degen[t] = f3dot(cr, cr) == 0;
        if (cull) {
            F3 n[3];
            for (int k = 0; k < 3; ++k) {
                uint32_t v = s->indices[3 * t + k];
                n[k] = {s->normals[3 * v], s->normals[3 * v + 1], s->normals[3 * v + 2]};
            }
            F3 sum = f3add(f3add(n[0], n[1]), n[2]);
            F3 N = f3norm({sum.x / 3.0f, sum.y / 3.0f, sum.z / 3.0f});
            N = f3norm(m3v(s->normal_to_render, N));
            w.back[t] = f3dot(look, N) > 0;
        }
    }
}
// The fast traversal's BVH over tile set `set` (non-degenerate triangles; set 1 without the back-facing ones) and
// the canonical rule's constants, from M = max |world vertex coordinate|:
//   wabs = M 2^-20 (the window W(t) = t 2^-16 + wabs; the oracle's Octree::SetWindow computes the same value);
//   pad = M 2^-18: every child box is padded by it before quantisation.  The slab test's rounding (box_entry in
//     rt_kernels.hip: base = fma(origin, inv, -o inv), t = fma(q, inv 2^e, base)) moves a plane by at most a few
//     ulp of max(|o|, M) along its axis, i.e. < 2^-21 max(|o|, M), well inside the pad while |o| <= 8 M;
//   oguard = 8 M: rays whose origin lies farther out in some coordinate are declared ambiguous (exact BFS).
static void scene_bvh(const SceneWorld& w, int set, float node_cost, int max_leaf, BvhData& out, float& wabs,
                      float& oguard) {
    float mc = 0.f;
    for (const F3& p : w.wv) mc = std::max(mc, std::max(std::fabs(p.x), std::max(std::fabs(p.y), std::fabs(p.z))));
    wabs = mc * 0x1p-20f;
    oguard = mc * 8.f;
    const float pad = mc * 0x1p-18f;
    const int nt = (int)w.degen.size();
    std::vector<float> t9;
    std::vector<int> ids;
    for (int t = 0; t < nt; ++t) {
        if (w.degen[t] || (set == 1 && w.back[t])) continue;
        for (int k = 0; k < 3; ++k) {
            const F3& p = w.tri3[3 * (size_t)t + k];
            t9.push_back(p.x); t9.push_back(p.y); t9.push_back(p.z);
        }
        ids.push_back(t);
    }
    build_bvh8(t9.data(), ids.data(), (int)ids.size(), pad, node_cost, out, max_leaf);
}

// The first rule a scene description breaks, or an empty string.  geometry_only: the rules a BVH build alone depends
// on (rt_debug_bvh_build).
static std::string validate_scene(const rt_scene_desc* s, bool geometry_only = false) {
    if (s->n_triangles <= 0 || s->n_vertices <= 0 || !s->positions || !s->indices)
        return "scene needs positions and indices";
    if (s->cull_backfaces && !s->normals) return "back-face culling needs vertex normals";
    for (int t = 0; t < 3 * s->n_triangles; ++t)
        if (s->indices[t] >= (uint32_t)s->n_vertices) return "triangle index out of range";
    if (geometry_only) return "";
    auto mat_ok = [&](int m) { return m >= 0 && m < std::max(1, s->n_materials); };
    if (s->tri_material)
        for (int t = 0; t < s->n_triangles; ++t)
            if (!mat_ok(s->tri_material[t])) return "material id out of range";
    for (int i = 0; i < s->n_materials; ++i) {
        const rt_material& m = s->materials[i];
        if (m.type < RT_MAT_DIFFUSE || m.type > RT_MAT_ROUGH_DIELECTRIC) return "unknown material type";
        if (m.type == RT_MAT_DIELECTRIC && m.eta < 0) return "dielectric eta must be >= 0";
        // (the roughness travels in eta; an emitter of type 3 is an emitter like any other: its eta is not read)
        if (m.type == RT_MAT_ROUGH && !(m.emission_scale > 0) && !ggx_alpha_ok(m.eta))
            return "rough material: alpha (rt_material.eta) must be in [0.01, 1] (below 0.01: RT_MAT_MIRROR)";
        // a conductor: alpha by the rough rule, the metal in sigmoid[0], the other two coefficients unused
        if (m.type == RT_MAT_CONDUCTOR && !(m.emission_scale > 0)) {
            if (!ggx_alpha_ok(m.eta)) return "conductor material: alpha (rt_material.eta) must be in [0.01, 1]";
            if (!metal_id_ok(m.sigmoid[0])) return "conductor material: sigmoid[0] must be a metal, RT_METAL_AG .. RT_METAL_CU";
            if (!(m.sigmoid[1] == 0.f && m.sigmoid[2] == 0.f)) return "conductor material: sigmoid[1] and sigmoid[2] must be 0";
        }
        // a rough glass: a constant index above 1 in eta, alpha by the rough rule in sigmoid[0]
        if (m.type == RT_MAT_ROUGH_DIELECTRIC && !(m.emission_scale > 0)) {
            if (m.eta == 0.f)
                return "rough dielectric material: eta 0 (dispersive BK7) is not supported on a rough interface; give a constant eta > 1";
            if (!roughglass_eta_ok(m.eta)) return "rough dielectric material: eta must be finite and > 1";
            if (!ggx_alpha_ok(m.sigmoid[0])) return "rough dielectric material: alpha (rt_material.sigmoid[0]) must be in [0.01, 1]";
            if (!(m.sigmoid[1] == 0.f && m.sigmoid[2] == 0.f))
                return "rough dielectric material: sigmoid[1] and sigmoid[2] must be 0";
        }
    }
    if (s->n_shapes < 0 || (s->n_shapes > 0 && !s->shapes)) return "shapes";
    for (int i = 0; i < s->n_shapes; ++i) {
        const rt_shape& h = s->shapes[i];
        if (!mat_ok(h.material)) return "shape material out of range";
        if (h.type == RT_SHAPE_SPHERE) {
            if (!(h.radius > 0) || h.zmin > -h.radius || h.zmax < h.radius || h.phimax < 360.f)
                return "only full spheres are supported (zmin <= -r, zmax >= r, phimax >= 360)";
        } else if (h.type == RT_SHAPE_DISK) {
            if (h.phimax < 360.f || !(h.outer_radius > 0) || h.inner_radius < 0)
                return "only full disks are supported (phimax >= 360)";
        } else if (h.type != RT_SHAPE_TRIANGLE) {
            return "unknown shape type";
        }
    }
    if (s->n_lights < 0 || s->n_lights > kMaxLights || (s->n_lights > 0 && !s->lights))
        return "lights: at most " + std::to_string(kMaxLights);
    for (int i = 0; i < s->n_lights; ++i) {
        const rt_light& L = s->lights[i];
        if (L.type == RT_LIGHT_QUAD) {
            if (!mat_ok(L.material) || !(s->materials && s->materials[L.material].emission_scale > 0))
                return "quad light needs an emissive material";
        } else if (L.type == RT_LIGHT_DISK) {
            if (L.shape < 0 || L.shape >= s->n_shapes || s->shapes[L.shape].type != RT_SHAPE_DISK ||
                s->shapes[L.shape].inner_radius != 0 || !(s->materials[s->shapes[L.shape].material].emission_scale > 0))
                return "disk light needs an emissive full DISK shape with inner radius 0";
        } else if (L.type == RT_LIGHT_DISTANT) {
            if (L.dir[0] == 0 && L.dir[1] == 0 && L.dir[2] == 0) return "distant light direction";
        } else if (L.type == RT_LIGHT_MESH) {
            // (that a non-degenerate triangle uses the material is checked once the world triangles exist:
            // scene_upload_one)
            if (!mat_ok(L.material) || !(s->materials && s->materials[L.material].emission_scale > 0))
                return "mesh light needs an emissive material";
            for (int h = 0; h < s->n_shapes; ++h)
                if (s->shapes[h].material == L.material)
                    return "mesh light material is used by an analytic shape (mesh lights are triangles only)";
            // DevMaterial.light names one light: no other light of any type may stand behind this material
            for (int j = 0; j < s->n_lights; ++j) {
                const rt_light& O = s->lights[j];
                if (j != i && (O.type == RT_LIGHT_QUAD || O.type == RT_LIGHT_MESH) && O.material == L.material)
                    return "mesh light material is named by another light";
            }
        } else if (L.type != RT_LIGHT_POINT) {
            return "unknown light type";
        }
    }
    return "";
}

// The octree's root box — TriModel::Bounds (Shapes.h:1390-1397): object-space min/max (max starts at FLT_MIN, :1292)
// then Bounds3::Transform (Shapes.h:60-98, same FLT_MIN quirk) — and the coherence sorts' quantisation over it.
static void scene_root_box(rt_ctx* c, const rt_scene_desc* s, F3& rmn, F3& rmx) {
    const float FMAX = std::numeric_limits<float>::max(), FMIN = std::numeric_limits<float>::min();
    F3 omn = {FMAX, FMAX, FMAX}, omx = {FMIN, FMIN, FMIN};
    for (int i = 0; i < s->n_vertices; ++i) {
        const float* p = s->positions + 3 * i;
        omn = {std::min(omn.x, p[0]), std::min(omn.y, p[1]), std::min(omn.z, p[2])};
        omx = {std::max(omx.x, p[0]), std::max(omx.y, p[1]), std::max(omx.z, p[2])};
    }
    const F3 corners[8] = {{omn.x, omn.y, omn.z}, {omn.x, omx.y, omn.z}, {omn.x, omx.y, omx.z}, {omn.x, omn.y, omx.z},
                           {omx.x, omx.y, omx.z}, {omx.x, omn.y, omx.z}, {omx.x, omn.y, omn.z}, {omx.x, omx.y, omn.z}};
    rmn = {FMAX, FMAX, FMAX};
    rmx = {FMIN, FMIN, FMIN};
    for (const F3& q : corners) {
        float o[4];
        m4v(s->object_to_render, q.x, q.y, q.z, 1.f, o);
        rmn = {std::min(rmn.x, o[0]), std::min(rmn.y, o[1]), std::min(rmn.z, o[2])};
        rmx = {std::max(rmx.x, o[0]), std::max(rmx.y, o[1]), std::max(rmx.z, o[2])};
    }
    // ray coherence sort: origins quantised to 9 bits per axis over the root box
    F3 e = f3sub(rmx, rmn);
    auto sc = [](float x) { return x > 0 ? 512.0f / x : 0.0f; };
    c->sort_lo = make_float4(rmn.x, rmn.y, rmn.z, 0.f);
    c->sort_scale = make_float4(sc(e.x), sc(e.y), sc(e.z), 0.f);
}

// The octree in the HBM layout of rt_internal.h: node SoA + the leaf tiles of the two tile sets (set 0: the
// non-degenerate triangles, set 1: without the back-facing ones).
struct FlatOctree {
    std::vector<float4> nA, nB;
    std::vector<int2> lr[2];
    std::vector<float4> tiles[2];
};
// (also fills the context's host mirrors of the tree, h_*)
static void flatten_octree(rt_ctx* c, const OctBuild& ob, const SceneWorld& sw, FlatOctree& f) {
    const int nn = (int)ob.nodes.size();
    f.nA.resize(nn); f.nB.resize(nn);
    f.lr[0].resize(nn); f.lr[1].resize(nn);
    c->h_bounds.assign(6 * (size_t)nn, 0.f);
    c->h_child.assign(nn, -1);
    c->h_leaf_first.assign(nn, 0);
    c->h_leaf_count.assign(nn, 0);
    c->h_refs.clear();
    auto push_tile = [&](std::vector<float4>& v, int t) {
        const F3* p = &sw.tri3[3 * (size_t)t];
        int bits = t;
        float fid;
        std::memcpy(&fid, &bits, 4);
        v.push_back(make_float4(p[0].x, p[0].y, p[0].z, p[1].x));
        v.push_back(make_float4(p[1].y, p[1].z, p[2].x, p[2].y));
        v.push_back(make_float4(p[2].z, fid, 0.f, 0.f));
    };
    for (int i = 0; i < nn; ++i) {
        const auto& N = ob.nodes[i];
        int child = N.first_child;
        float fc;
        std::memcpy(&fc, &child, 4);
        f.nA[i] = make_float4(N.mn.x, N.mn.y, N.mn.z, fc);
        f.nB[i] = make_float4(N.mx.x, N.mx.y, N.mx.z, 0.f);
        float* b = &c->h_bounds[6 * (size_t)i];
        b[0] = N.mn.x; b[1] = N.mn.y; b[2] = N.mn.z; b[3] = N.mx.x; b[4] = N.mx.y; b[5] = N.mx.z;
        c->h_child[i] = child;
        c->h_leaf_first[i] = (int)c->h_refs.size();
        c->h_leaf_count[i] = (int)N.tris.size();
        f.lr[0][i] = make_int2((int)f.tiles[0].size() / 3, 0);
        f.lr[1][i] = make_int2((int)f.tiles[1].size() / 3, 0);
        for (int t : N.tris) {
            c->h_refs.push_back(t);
            if (sw.degen[t]) continue;
            push_tile(f.tiles[0], t);
            f.lr[0][i].y++;
            if (!sw.back[t]) { push_tile(f.tiles[1], t); f.lr[1][i].y++; }
        }
    }
}

// What the traversal kernels need to know about the octree's shape.
struct OctLimits {
    int depth = 0;       // of the deepest node
    int bound = 0;       // exact worst case of the kernels' BFS group FIFO
    int qcap = 1;        // 1: single leaf; 16: register FIFO; 0: the LDS + HBM-spill FIFO
    bool ids16 = true;   // every group id (first child = 1 + 8 g) fits 16 bits
};
static int octree_limits(rt_ctx* c, const OctBuild& ob, OctLimits& L) {
    const int nn = (int)ob.nodes.size();
    std::vector<int> depth(nn, 0);
    for (int i = 0; i < nn; ++i) {
        const int fc = ob.nodes[i].first_child;
        if (fc >= 0) {
            for (int k = 0; k < 8; ++k) depth[fc + k] = depth[i] + 1;
            // children are created 8 at a time after the root (node 1 + 8 g)
            if ((fc - 1) % 8 != 0 || (fc - 1) / 8 > 65535) L.ids16 = false;
        }
        L.depth = std::max(L.depth, depth[i]);
    }
    // Exact worst case of the kernel's group FIFO: replay the BFS with every box test passing (any real ray
    // pushes a subset of these groups, in the same order, so its queue is never longer at the same point).
    {
        std::vector<int> fifo;
        fifo.reserve(nn);
        size_t head = 0;
        int cur = 0, left = 1;
        while (true) {
            int fc = ob.nodes[cur].first_child;
            if (fc >= 0) {
                fifo.push_back(fc);
                L.bound = std::max(L.bound, (int)(fifo.size() - head));
            }
            if (--left > 0) { ++cur; continue; }
            if (head == fifo.size()) break;
            cur = fifo[head++];
            left = 8;
        }
    }
    if (ob.nodes[0].first_child >= 0) {
        const int caps[] = {16};  // register FIFO; larger bounds use the LDS + HBM-spill FIFO (qcap 0)
        L.qcap = 0;
        for (int cp : caps)
            if (cp >= L.bound) { L.qcap = cp; break; }
        if (!L.qcap && L.bound > kRingMax)
            return fail(c, RT_E_LIMIT, "octree BFS frontier bound " + std::to_string(L.bound) + " exceeds " +
                                           std::to_string(kRingMax) + " groups");
        // the LDS FIFO stores 16-bit group ids
        if (!L.qcap && !L.ids16) return fail(c, RT_E_LIMIT, "octree too large for 16-bit BFS group ids");
    }
    return RT_OK;
}

// multi-level octrees: the fast traversal's BVH per tile set (non-degenerate triangles; set 1 without the
// back-facing ones) and the canonical-rule window (rt_bvh.cpp)
// [kBvhAny]: the any-hit BVH of the shadow rays (set 0), built with its own SAH cost and leaf size
static int scene_bvhs(rt_ctx* c, const SceneWorld& sw, int qcap, BvhData bvh[3], float& wabs, float& oguard) {
    const Knobs& kn = c->knobs;
    if (qcap != 1) {
        // a BVH leaf word holds its first tile in 27 bits (rt_kernels.hip decode_leaf): one tile per triangle
        if (sw.tri3.size() / 3 >= ((size_t)1 << 27))
            return fail(c, RT_E_LIMIT, "more than 2^27 triangles: the BVH leaf words hold 27-bit tile offsets");
        for (int st = 0; st < (c->cull ? 2 : 1); ++st)
            scene_bvh(sw, st, kn.bvh_node_cost, kn.bvh_max_leaf, bvh[st], wabs, oguard);
        if (kn.bvh_any_cost > 0) scene_bvh(sw, 0, kn.bvh_any_cost, kn.bvh_any_leaf, bvh[kBvhAny], wabs, oguard);
    } else {
        // single leaf: the same window for the closest-hit pass 2's nearest-first order (rt_kernels.hip traverse)
        float mc = 0.f;
        for (const F3& p : sw.wv) mc = std::max(mc, std::max(std::fabs(p.x), std::max(std::fabs(p.y), std::fabs(p.z))));
        wabs = mc * 0x1p-20f;
    }
    return RT_OK;
}

// Per-triangle shading data, materials, analytic shapes and lights as the kernels read them.
struct ShadingArrays {
    std::vector<float4> tw, tn;     // world vertices and vertex normals, 3 per triangle
    std::vector<int> tm;            // material per triangle
    std::vector<DevMaterial> mats;
    std::vector<DevShape> shapes;
    std::vector<float> kappa;       // per shape: shape_curvature
    std::vector<DevLight> lights;
    // the emissive surfaces, for the last depth's emitter filter (EmitIO): non-degenerate triangles and shapes whose
    // material emits
    std::vector<int> etris, eshapes;
    // mesh lights: per light its slice (first, n) of ml_tri, the non-degenerate triangles of the
    // light's material in ascending id (n = 0: not a mesh light)
    std::vector<int> ml_first, ml_n, ml_tri;
    bool full = false;              // the scene needs the general path-shade kernel
    bool rough = false;             // a non-emissive RT_MAT_ROUGH material (the RGH instantiations)
    bool conductor = false;         // a non-emissive RT_MAT_CONDUCTOR material (RGH level 2)
    bool rough_dielectric = false;  // a non-emissive RT_MAT_ROUGH_DIELECTRIC material (RGH level 3)
};
// The curvature magnitude the curved chain guides give a shape: 1 / (radius sigma) for a sphere whose
// object_to_render linear part L is a rotation times a uniform scale sigma, 0 for every other shape.  In float64:
// G = L^T L, sigma^2 = tr G / 3, uniform iff max |G - sigma^2 I| <= 1e-5 sigma^2; the result is rounded to float.
static float shape_curvature(const rt_shape& h) {
    if (h.type != RT_SHAPE_SPHERE) return 0.f;
    double G[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double g = 0;  // columns i and j of the column-major matrix
            for (int r = 0; r < 3; ++r) g += (double)h.object_to_render[4 * i + r] * (double)h.object_to_render[4 * j + r];
            G[i][j] = g;
        }
    const double s2 = (G[0][0] + G[1][1] + G[2][2]) / 3.0;
    double dev = 0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) dev = std::max(dev, std::fabs(G[i][j] - (i == j ? s2 : 0.0)));
    if (!(s2 > 0) || !(dev <= 1e-5 * s2)) return 0.f;
    const double rs = (double)h.radius * std::sqrt(s2);
    return rs > 0 ? (float)(1.0 / rs) : 0.f;
}
static void shading_arrays(const rt_scene_desc* s, const SceneWorld& sw, ShadingArrays& a) {
    const int nt = s->n_triangles;
    a.tw.resize(3 * (size_t)nt); a.tn.resize(3 * (size_t)nt);
    for (int t = 0; t < nt; ++t)
        for (int k = 0; k < 3; ++k) {
            const F3& p = sw.tri3[3 * (size_t)t + k];
            a.tw[3 * (size_t)t + k] = make_float4(p.x, p.y, p.z, 0.f);
            uint32_t v = s->indices[3 * t + k];
            a.tn[3 * (size_t)t + k] = s->normals ? make_float4(s->normals[3 * v], s->normals[3 * v + 1], s->normals[3 * v + 2], 0.f)
                                                 : make_float4(0.f, 0.f, 1.f, 0.f);
        }
    a.tm.assign(nt, 0);
    if (s->tri_material) a.tm.assign(s->tri_material, s->tri_material + nt);
    std::vector<DevMaterial>& mats = a.mats;
    for (int i = 0; i < s->n_materials; ++i) {
        const rt_material& m = s->materials[i];
        // material bin (kMatClasses): a rough reflector reads spectra and writes NEE records, like Lambert
        const int cls = material_class(m.type, m.emission_scale > 0);  // (rt_pass_plan.h)
        a.rough = a.rough || rough_fact(m.type, m.emission_scale > 0);
        a.conductor = a.conductor || conductor_fact(m.type, m.emission_scale > 0);
        a.rough_dielectric = a.rough_dielectric || rough_dielectric_fact(m.type, m.emission_scale > 0);
        mats.push_back(DevMaterial{m.sigmoid[0], m.sigmoid[1], m.sigmoid[2], m.emission_scale, m.type, m.eta, -1, cls});
    }
    if (mats.empty()) mats.push_back(DevMaterial{0.f, 0.f, 0.f, 0.f, RT_MAT_DIFFUSE, 0.f, -1, 0});
    std::vector<DevShape>& shapes = a.shapes;
    shapes.resize(s->n_shapes);
    for (int i = 0; i < s->n_shapes; ++i) {
        const rt_shape& h = s->shapes[i];
        DevShape& d = shapes[i];
        d = DevShape{};
        d.type = h.type; d.material = h.material; d.light = -1;
        d.r = h.radius;
        d.zmin = std::min(std::max(h.zmin, -h.radius), h.radius);  // glm::clamp(_zmin, -r, r) (Shapes.h:222-223)
        d.zmax = std::min(std::max(h.zmax, -h.radius), h.radius);
        d.h = h.height; d.ri = h.inner_radius; d.ro = h.outer_radius;
        std::memcpy(d.o2r, h.object_to_render, 64); std::memcpy(d.r2o, h.render_to_object, 64);
        std::memcpy(d.n2r, h.normal_to_render, 36);
        std::memcpy(d.p1, h.p, 12); std::memcpy(d.p2, h.p + 3, 12); std::memcpy(d.p3, h.p + 6, 12);
        shape_bound(d);
        a.kappa.push_back(shape_curvature(h));
    }
    a.lights.resize(s->n_lights);
    bool full = s->n_shapes > 0 || s->n_lights != 1;
    for (const DevMaterial& m : mats) full = full || m.type != RT_MAT_DIFFUSE;
    for (int i = 0; i < s->n_lights; ++i) {
        const rt_light& q = s->lights[i];
        DevLight& L = a.lights[i];
        L = DevLight{};
        L.type = q.type; L.shape = q.shape; L.material = q.material; L.scale = q.scale;
        for (int k = 0; k < 3; ++k) { L.p[k] = q.p[k]; L.e1[k] = q.e1[k]; L.e2[k] = q.e2[k]; L.n[k] = q.n[k]; }
        if (q.type == RT_LIGHT_QUAD) {
            F3 cr = f3cross({q.e1[0], q.e1[1], q.e1[2]}, {q.e2[0], q.e2[1], q.e2[2]});
            L.area = std::sqrt(f3dot(cr, cr));
            if (mats[q.material].light < 0) mats[q.material].light = i;
        } else if (q.type == RT_LIGHT_DISK) {
            const DevShape& ds = shapes[q.shape];
            const float phimax = 360.0f * 0.01745329251994329576923690768489f;  // glm::radians(360.f)
            L.area = phimax * .5f * (ds.ro * ds.ro - ds.ri * ds.ri);           // Disk::Area (Shapes.h:641-644)
            F3 n = f3norm(m3v(ds.n2r, F3{0.f, 0.f, 1.f}));
            L.n[0] = n.x; L.n[1] = n.y; L.n[2] = n.z;
            L.material = ds.material; L.ro = ds.ro; L.h = ds.h;
            std::memcpy(L.o2r, ds.o2r, 64);
            shapes[q.shape].light = i;
        } else if (q.type == RT_LIGHT_DISTANT) {
            F3 d = f3norm(F3{q.dir[0], q.dir[1], q.dir[2]});
            L.dir[0] = d.x; L.dir[1] = d.y; L.dir[2] = d.z;
        } else if (q.type == RT_LIGHT_MESH) {
            // (p, e1, e2 and area are set from the device table: upload_scene, mesh_light_tables)
            for (int k = 0; k < 3; ++k) L.p[k] = L.e1[k] = L.e2[k] = L.n[k] = 0.f;
            mats[q.material].light = i;  // (validate_scene: no other light names this material)
        }
        if (q.type != RT_LIGHT_QUAD) full = true;
    }
    a.ml_first.assign(s->n_lights, 0);
    a.ml_n.assign(s->n_lights, 0);
    for (int i = 0; i < s->n_lights; ++i) {
        if (s->lights[i].type != RT_LIGHT_MESH) continue;
        a.ml_first[i] = (int)a.ml_tri.size();
        for (int t = 0; t < nt; ++t)
            if (!sw.degen[t] && a.tm[t] == s->lights[i].material) a.ml_tri.push_back(t);
        a.ml_n[i] = (int)a.ml_tri.size() - a.ml_first[i];
    }
    a.full = full;
    for (int t = 0; t < nt; ++t)
        if (!sw.degen[t] && mats[a.tm[t]].emit > 0) a.etris.push_back(t);
    for (int i = 0; i < s->n_shapes; ++i)
        if (mats[shapes[i].material].emit > 0) a.eshapes.push_back(i);
}

// single-leaf octree: conservative boxes of runs of kClusterTris leaf tiles (pass-1 culling in the kernel); a
// box miss means none of its triangles can pass the watertight test's tMax-independent checks, so the
// inflation only has to cover those checks' rounding.  In the sheared frame every vertex coordinate carries
// at most ~4 ulp(M) of error, M = the largest |vertex - origin|; with origins inside 8 extents of the scene
// centre (cl_guard; farther rays never skip) M <= 9.8 ext, i.e. <= 2.4e-6 ext, and the pad is 1e-5 ext +
// 1e-3 — small enough that a wave of rays leaving one wall (origin offset 1e-4 (1 + max|p|)) skips it.  The box
// test's own rounding comes on top (rt_cull.h, where the bound is derived): with the inverse direction's rounding its
// FMA form moves a plane by up to 1.5e-6 ext + 3 * 2^-24 |c|, c = the scene's centre; the first part fits the pad
// above (3.9e-6 ext in all), the second is what kClusterPadCentre |c| adds to it.
struct LeafClusters {
    std::vector<float4> box[2];     // per tile set: (min, max) per cluster; empty for multi-level octrees
    unsigned long long fan_pairs[2] = {0, 0};
    float4 guard{};
};
static void leaf_clusters(const OctBuild::Node& R, const FlatOctree& f, LeafClusters& cl) {
    float ext = std::max(std::max(R.mx.x - R.mn.x, R.mx.y - R.mn.y), R.mx.z - R.mn.z);
    float pad = kClusterPadRel * ext + 1e-3f;
    cl.guard = make_float4(.5f * (R.mn.x + R.mx.x), .5f * (R.mn.y + R.mx.y), .5f * (R.mn.z + R.mx.z), 64.f * ext * ext);
#if RT_CULL_FMA
    // the cull's FMA form rounds o / d, not plane - o: 3 * 2^-24 |c| of its error grows with the scene's distance |c|
    // from the coordinate origin, not with its extent (rt_cull.h); that part is added to the pad (Cornell: +1 %)
    pad += kClusterPadCentre * std::max(std::max(std::fabs(cl.guard.x), std::fabs(cl.guard.y)), std::fabs(cl.guard.z));
#endif
    for (int st = 0; st < 2; ++st) {
        const std::vector<float4>& tl = f.tiles[st];
        int nt_leaf = (int)tl.size() / 3;
        for (int k0 = 0; k0 < nt_leaf; k0 += kClusterTris) {
            float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
            for (int k = k0; k < std::min(nt_leaf, k0 + kClusterTris); ++k) {
                const float4* q = tl.data() + 3 * k;
                float v[9] = {q[0].x, q[0].y, q[0].z, q[0].w, q[1].x, q[1].y, q[1].z, q[1].w, q[2].x};
                for (int j = 0; j < 3; ++j)
                    for (int a = 0; a < 3; ++a) { mn[a] = std::min(mn[a], v[3 * j + a]); mx[a] = std::max(mx[a], v[3 * j + a]); }
            }
            cl.box[st].push_back(make_float4(mn[0] - pad, mn[1] - pad, mn[2] - pad, 0.f));
            cl.box[st].push_back(make_float4(mx[0] + pad, mx[1] + pad, mx[2] + pad, 0.f));
        }
        // fan pairs: tile k+1 = (a, c, d) after tile k = (a, b, c), bit for bit (_quad / OBJ fan triangulation)
        unsigned long long fp = 0;
        for (int k = 0; k + 1 < std::min(nt_leaf, 64); k += 2) {
            const float4* q = tl.data() + 3 * k;
            float v[9] = {q[0].x, q[0].y, q[0].z, q[0].w, q[1].x, q[1].y, q[1].z, q[1].w, q[2].x};
            float w[9] = {q[3].x, q[3].y, q[3].z, q[3].w, q[4].x, q[4].y, q[4].z, q[4].w, q[5].x};
            if (!std::memcmp(w, v, 12) && !std::memcmp(w + 3, v + 6, 12)) fp |= 1ull << k;
        }
        cl.fan_pairs[st] = fp;
    }
}

// one host array on the device, owned by the context's scene (at least 16 bytes, so empty arrays have a pointer too)
extern "C++" template <class T>
static int upload_array(rt_ctx* c, const std::vector<T>& v, const T*& dst) {
    const size_t bytes = v.size() * sizeof(T);
    DevBuf<unsigned char> b;
    HIPCHK(c, b.reserve(std::max<size_t>(bytes, 16)));
    dst = reinterpret_cast<const T*>(b.get());
    c->scene_allocs.push_back(std::move(b));
    if (bytes) HIPCHK(c, hipMemcpy(c->scene_allocs.back().get(), v.data(), bytes, hipMemcpyHostToDevice));
    return RT_OK;
}

// The device tables of the scene's mesh lights, built by k_meshlight_table from the resident world
// triangles, and each mesh light's DevLight words: its slice of the shared id and cdf arrays and its total area.
static int mesh_light_tables(rt_ctx* c, const ShadingArrays& a, const float4* triWorld, std::vector<DevLight>& lights) {
    rt_ctx::MeshLights& M = c->ml;
    M.first = a.ml_first;
    M.n = a.ml_n;
    M.area.assign(lights.size(), 0.f);
    std::vector<int> jobs, job_light;
    for (size_t i = 0; i < lights.size(); ++i)
        if (a.ml_n[i] > 0) { jobs.push_back(a.ml_first[i]); jobs.push_back(a.ml_n[i]); job_light.push_back((int)i); }
    if (job_light.empty()) return RT_OK;
    const int nj = (int)job_light.size();
    std::vector<float> zeros(a.ml_tri.size(), 0.f), zarea(nj, 0.f);
    const int* d_jobs = nullptr;
    const float *d_sums = nullptr, *d_area = nullptr;
    int rc;
    if ((rc = upload_array(c, a.ml_tri, M.tri)) || (rc = upload_array(c, zeros, M.cdf)) ||
        (rc = upload_array(c, zeros, d_sums)) || (rc = upload_array(c, jobs, d_jobs)) ||
        (rc = upload_array(c, zarea, d_area)))
        return rc;
    std::vector<float> area(nj);
    HIPCHK(c, launch_meshlight_table(c->stream, triWorld, nj, d_jobs, M.tri, const_cast<float*>(d_sums),
                                     const_cast<float*>(M.cdf), const_cast<float*>(d_area)));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(area.data(), d_area, sizeof(float) * (size_t)nj, hipMemcpyDeviceToHost));
    for (int j = 0; j < nj; ++j) {
        const int i = job_light[j];
        if (!(area[j] > 0.f) || !std::isfinite(area[j]))
            return fail(c, RT_E_ARG, "mesh light " + std::to_string(i) + ": the total area of its triangles is not a positive finite float");
        M.area[i] = area[j];
        lights[i].area = area[j];
        meshlight_pack(lights[i], MeshLightTab{M.tri + a.ml_first[i], M.cdf + a.ml_first[i], a.ml_n[i]});
    }
    M.any = true;
    return RT_OK;
}

// Everything on the device and the DevScene that points to it.
static int upload_scene(rt_ctx* c, const rt_scene_desc* s, const FlatOctree& f, const OctLimits& lim,
                        const ShadingArrays& a, const LeafClusters& cl, BvhData bvh[3], float wabs, float oguard) {
    DevScene& d = c->dsc;
    const int qcap = lim.qcap;
    int rc;
    if ((rc = upload_array(c, f.nA, d.nodeA)) || (rc = upload_array(c, f.nB, d.nodeB)) ||
        (rc = upload_array(c, f.lr[0], d.leafRange[0])) || (rc = upload_array(c, f.lr[1], d.leafRange[1])) ||
        (rc = upload_array(c, f.tiles[0], d.tiles[0])) || (rc = upload_array(c, f.tiles[1], d.tiles[1])) ||
        (rc = upload_array(c, a.tw, d.triWorld)) || (rc = upload_array(c, a.tn, d.triNormal)) ||
        (rc = upload_array(c, a.tm, d.triMaterial)) || (rc = upload_array(c, a.mats, d.materials)) ||
        (rc = upload_array(c, a.shapes, d.shapes)) || (rc = upload_array(c, a.kappa, c->d_kappa)))
        return rc;
    std::vector<DevLight> lights = a.lights;  // (mesh lights: completed from the device tables)
    if ((rc = mesh_light_tables(c, a, d.triWorld, lights)) || (rc = upload_array(c, lights, d.lights))) return rc;
    c->h_lights = lights;
    c->base_lights = d.lights;
    if (qcap == 1) {
        d.cl_guard = cl.guard;
        for (int st = 0; st < 2; ++st) {
            d.n_clusters[st] = (int)cl.box[st].size() / 2;
            d.fan_pairs[st] = cl.fan_pairs[st];
        }
    }
    if ((rc = upload_array(c, cl.box[0], d.clusters[0])) || (rc = upload_array(c, cl.box[1], d.clusters[1]))) return rc;
    const int bvh_nodes0 = (int)(bvh[0].nodes.size() / kBvhNodeF4);
    for (int st = 0; st < 3; ++st) {
        // a BVH not built here (no culled set; the any-hit walks on the closest-hit BVH of set 0) uses set 0's arrays
        const int src = bvh[st].nodes.empty() ? 0 : st;
        c->bvh_count[st][0] = (int)(bvh[src].nodes.size() / kBvhNodeF4);
        c->bvh_count[st][1] = (int)bvh[src].tid.size();
    }
    for (int st = 0; st < 3; ++st) {
        d.bvh[st] = nullptr; d.btiles[st] = nullptr; d.btid[st] = nullptr;
        if (bvh[st].nodes.empty()) continue;
        // the kernels stage nodes [0, kBvhTopNodes) in LDS unconditionally: pad with empty nodes
        if (bvh[st].nodes.size() < kBvhNodeF4 * (size_t)kBvhTopNodes)
            bvh[st].nodes.resize(kBvhNodeF4 * (size_t)kBvhTopNodes, make_float4(0.f, 0.f, 0.f, 0.f));
        bvh[st].tiles.resize(bvh[st].tiles.size() + 4, 0.f);  // (an empty BVH still gets a buffer)
        bvh[st].tid.push_back(-1);
        if ((rc = upload_array(c, bvh[st].nodes, d.bvh[st])) || (rc = upload_array(c, bvh[st].tiles, d.btiles[st])) ||
            (rc = upload_array(c, bvh[st].tid, d.btid[st])))
            return rc;
    }
    for (int st = 1; st < 3; ++st)
        if (!d.bvh[st]) { d.bvh[st] = d.bvh[0]; d.btiles[st] = d.btiles[0]; d.btid[st] = d.btid[0]; }
    d.wabs = wabs;
    d.oguard = oguard;
    d.amb_force = c->knobs.force_amb >= 0;
    d.amb_mask = c->knobs.force_amb > 0 ? (1u << c->knobs.force_amb) - 1u : 0u;
    c->info.bvh_nodes = bvh_nodes0;
    c->info.bvh_depth = bvh[0].depth;
    if (qcap != 1) d.n_clusters[0] = d.n_clusters[1] = 0;
    d.n_nodes = (int)f.nA.size();
    d.n_tris = s->n_triangles;
    d.n_shapes = s->n_shapes;
    d.n_materials = (int)a.mats.size();
    c->scene_full = a.full;
    c->scene_rough = a.rough;
    c->scene_conductor = a.conductor;
    c->scene_rough_dielectric = a.rough_dielectric;
    d.qcap = qcap;
    // the cooperative BFS's FIFO holds 16-bit group ids (first child = 1 + 8 g) and kCoopFifo of them
    d.coop_ok = c->knobs.coop && qcap != 1 && lim.bound <= kCoopFifo && lim.ids16 ? 1 : 0;
    d.depth = d.n_nodes < (1 << 24) ? lim.depth : 1 << 30;  // DFS stack entries hold 24-bit group ids
    if (qcap == 0) {  // each lane allocates its ring of ring_threads x rs ints (ensure_ring)
        int rs = 1;
        while (rs < lim.bound) rs <<= 1;
        d.ring_threads = c->grid * kBlockThreads;
        d.ring_mask = rs - 1;
    }
    d.n_lights = s->n_lights;
    if (s->n_lights >= 1) d.light0 = lights[0];
    // more than kMaxEmitTris emissive triangles turn the emitter filter off
    if ((rc = upload_array(c, a.etris, d.emit_tris)) || (rc = upload_array(c, a.eshapes, d.emit_shapes))) return rc;
    d.n_emit_tris = (int)a.etris.size() <= kMaxEmitTris ? (int)a.etris.size() : -1;
    d.n_emit_shapes = (int)a.eshapes.size();
    c->have_scene = true;
    return RT_OK;
}

static int scene_upload_one(rt_ctx* c, const rt_scene_desc* s) {
    if (!c || !s) return RT_E_ARG;
    const std::string bad = validate_scene(s);
    if (!bad.empty()) return fail(c, RT_E_ARG, bad);
    SceneWorld sw;
    scene_world(s, sw);
    for (int i = 0; i < s->n_lights; ++i) {  // (before the old scene is released: a rejected upload changes nothing)
        if (s->lights[i].type != RT_LIGHT_MESH) continue;
        bool used = false;
        for (int t = 0; t < s->n_triangles && !used; ++t)
            used = !sw.degen[t] && (s->tri_material ? s->tri_material[t] : 0) == s->lights[i].material;
        if (!used) return fail(c, RT_E_ARG, "mesh light " + std::to_string(i) + ": no non-degenerate triangle uses its material");
    }
    hipSetDevice(c->device);
    hipStreamSynchronize(c->stream);
    free_scene(c);
    c->cull = s->cull_backfaces != 0;
    // octree build (all triangles, culled and degenerate included — the reference inserts every triangle)
    OctBuild ob;
    ob.tri3 = &sw.tri3;
    ob.capacity = s->octree_capacity > 0 ? s->octree_capacity : 40;
    OctBuild::Node root;
    scene_root_box(c, s, root.mn, root.mx);
    ob.nodes.push_back(root);
    if (c->octree_build == RT_OCTREE_BUILD_HOST) {
        for (int t = 0; t < s->n_triangles; ++t) ob.add(t);
    } else {
        std::string err;
        int brc = octree_build_device(c->stream, ob, s->n_triangles, err);
        if (brc) return fail(c, brc, err);
    }
    int rc;
    FlatOctree flat;
    flatten_octree(c, ob, sw, flat);
    OctLimits lim;
    if ((rc = octree_limits(c, ob, lim))) return rc;
    BvhData bvh[3];
    float wabs = 0.f, oguard = 0.f;
    if ((rc = scene_bvhs(c, sw, lim.qcap, bvh, wabs, oguard))) return rc;
    c->info.n_nodes = (int)ob.nodes.size();
    c->info.n_leaf_refs = (int)c->h_refs.size();
    c->info.max_queue_groups = lim.bound;
    c->info.depth = lim.depth;
    c->n_tris = s->n_triangles;
    ShadingArrays shade;
    shading_arrays(s, sw, shade);
    LeafClusters clus;
    if (lim.qcap == 1) leaf_clusters(ob.nodes[0], flat, clus);
    if ((rc = upload_scene(c, s, flat, lim, shade, clus, bvh, wabs, oguard))) return rc;
    c->tx.mat_flags.assign(shade.mats.size(), 0);
    for (size_t i = 0; i < shade.mats.size(); ++i)
        c->tx.mat_flags[i] = shade.mats[i].emit > 0 ? 1 : shade.mats[i].type == RT_MAT_CONDUCTOR ? 4
                             : shade.mats[i].type == RT_MAT_ROUGH_DIELECTRIC ? 8 : 0;
    for (const DevShape& h : shade.shapes) c->tx.mat_flags[h.material] |= 2;
    c->med.mat_type.resize(shade.mats.size());
    c->med.mat_emits.resize(shade.mats.size());
    for (size_t i = 0; i < shade.mats.size(); ++i) {
        c->med.mat_type[i] = shade.mats[i].type;
        c->med.mat_emits[i] = shade.mats[i].emit > 0 ? 1 : 0;
    }
    return RT_OK;
}

static int camera_set_one(rt_ctx* c, const rt_camera_desc* d) {
    if (!c || !d) return RT_E_ARG;
    if (d->type < RT_CAMERA_PERSPECTIVE || d->type > RT_CAMERA_THINLENS) return fail(c, RT_E_ARG, "unknown camera type");
    c->cam = *d;
    c->have_cam = true;
    return RT_OK;
}

static int sampler_set_one(rt_ctx* c, const rt_sampler_desc* d) {
    if (!c || !d) return RT_E_ARG;
    if (d->kind < RT_SAMPLER_INDEPENDENT || d->kind > RT_SAMPLER_SOBOL) return fail(c, RT_E_ARG, "unknown sampler");
    if (d->kind == RT_SAMPLER_SOBOL && (d->randomize < RT_SOBOL_NONE || d->randomize > RT_SOBOL_OWEN))
        return fail(c, RT_E_ARG, "unknown Sobol randomization");
    if (d->x_samples <= 0 || (d->kind == RT_SAMPLER_STRATIFIED && d->y_samples <= 0))
        return fail(c, RT_E_ARG, "samples per pixel must be positive");
    c->smp = *d;
    c->have_smp = true;
    return RT_OK;
}

static int film_set_one(rt_ctx* c, const rt_film_desc* d) {
    if (!c || !d) return RT_E_ARG;
    if (d->res_x <= 0 || d->res_y <= 0 || d->filter < RT_FILTER_BOX || d->filter > RT_FILTER_LANCZOS)
        return fail(c, RT_E_ARG, "invalid film");
    if ((size_t)d->res_x * d->res_y > ((size_t)1 << 27)) return fail(c, RT_E_LIMIT, "film too large");
    if (c->ad.live) return fail(c, RT_E_STATE, "rt_film_set during an adaptive session (rt_adaptive_end first)");
    if (c->tp.live) return fail(c, RT_E_STATE, "rt_film_set during a temporal session (rt_temporal_end first)");
    if (d->sensor < 0 || d->sensor >= RT_SENSOR_COUNT || d->sensor_illum < 0 || d->sensor_illum >= RT_ILLUM_COUNT)
        return fail(c, RT_E_ARG, "unknown sensor or sensor illuminant");
    hipSetDevice(c->device);
    if (c->stream) hipStreamSynchronize(c->stream);  // queued passes may still read the old tables
    int y_int = 0;  // committed with the film descriptor below, only once the sensor is set up
    {  // RayTracerTestApp.h:289-291 divides in float; the kernels may divide integers where that is identical
        const int w = d->res_x, n = d->res_x * d->res_y;
        int ok = 1;
        for (int p = 0; p < n && ok; ++p) ok = (int)std::floor((float)p / (float)w) == p / w;
        y_int = ok;
    }
    int rc = setup_sensor(c, *d);
    if (rc) return rc;
    c->d_cdf.reset();
    c->cdf_n = 0;
    if (d->filter == RT_FILTER_GAUSSIAN || d->filter == RT_FILTER_LANCZOS) {
        std::vector<float> tx, ty;
        int n = build_filter_tables(*d, tx, ty);
        if (c->d_cdf.reserve(2 * (size_t)(n + 1)) != hipSuccess) return fail(c, RT_E_OOM, "filter tables");
        hipMemcpy(c->d_cdf.get(), tx.data(), sizeof(float) * (n + 1), hipMemcpyHostToDevice);
        hipMemcpy(c->d_cdf.get() + (n + 1), ty.data(), sizeof(float) * (n + 1), hipMemcpyHostToDevice);
        c->cdf_n = n;
    }
    c->film = *d;
    c->film_y_int = y_int;
    c->have_film = true;
    c->work_dirty = true;
    return RT_OK;
}

static_assert(rtdata::n_cameras + 1 == RT_SENSOR_COUNT, "camera table and RT_SENSOR_COUNT disagree");

const char* rt_sensor_name(int sensor) {
    if (sensor == RT_SENSOR_XYZ) return "xyz";
    if (sensor < 1 || sensor >= RT_SENSOR_COUNT) return nullptr;
    return rtdata::camera_names[sensor - 1];
}

static int impl_rt_film_matrices(rt_ctx* c, float* xyz_from_sensor9, float* rgb_from_xyz9) {
    if (!c || !xyz_from_sensor9 || !rgb_from_xyz9) return RT_E_ARG;
    std::memcpy(xyz_from_sensor9, c->resolveA, 36);
    std::memcpy(rgb_from_xyz9, c->resolveB, 36);
    return RT_OK;
}

static int integrator_set_one(rt_ctx* c, const rt_integrator_desc* d) {
    if (!c || !d) return RT_E_ARG;
    if (d->kind != RT_INTEGRATOR_REFERENCE && d->kind != RT_INTEGRATOR_PATH && d->kind != RT_INTEGRATOR_PATH_MIS)
        return fail(c, RT_E_ARG, "unknown integrator");
    if (d->max_depth < 0 || d->max_depth > 64) return fail(c, RT_E_ARG, "max_depth out of range");
    if (d->kind == RT_INTEGRATOR_REFERENCE &&
        !(d->albedo_rgb[0] == d->albedo_rgb[1] && d->albedo_rgb[1] == d->albedo_rgb[2] && d->albedo_rgb[0] > 0 &&
          d->albedo_rgb[0] < 1))
        return fail(c, RT_E_ARG, "reference Li albedo must be a grey in (0,1): the RGB->spectrum table is absent "
                                 "(color.cpp:114), only the uniform branch color.cpp:35-37 exists");
    c->integ = *d;
    c->have_integ = true;
    return RT_OK;
}

static int set_shard_one(rt_ctx* c, int tile_size, int n_shards, int shard_id) {
    if (!c || tile_size <= 0 || tile_size % 8 || n_shards <= 0 || shard_id < 0 || shard_id >= n_shards)
        return c ? fail(c, RT_E_ARG, "invalid shard (tile_size must be a positive multiple of 8)") : RT_E_ARG;
    if (c->ad.live) return fail(c, RT_E_STATE, "rt_set_shard during an adaptive session (rt_adaptive_end first)");
    if (c->tp.live) return fail(c, RT_E_STATE, "rt_set_shard during a temporal session (rt_temporal_end first)");
    c->tile = tile_size;
    c->n_shards = n_shards;
    c->shard_id = shard_id;
    c->work_dirty = true;
    return RT_OK;
}

static int impl_rt_render_pass_device(rt_ctx* c, int ib, int ie, void* d_film, void* stream) {
    if (!c || !d_film) return RT_E_ARG;
    hipSetDevice(c->device);
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    return render_multi(c, ib, ie, (float4*)d_film, st);
}

static int impl_rt_render_pass(rt_ctx* c, int ib, int ie, rt_pixel* film) {
    if (!c || !film) return RT_E_ARG;
    int rc = check_ready(c);
    if (rc) return rc;
    hipSetDevice(c->device);
    size_t n = (size_t)c->film.res_x * c->film.res_y;
    if ((rc = stage_in(c, c->d_film, film, n, c->stream))) return rc;
    if ((rc = render_multi(c, ib, ie, c->d_film.get(), c->stream))) return rc;
    if ((rc = stage_out(c, film, c->d_film, n, c->stream))) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return RT_OK;
}

// ---- adaptive sampling: a session's film, moments and active list stay on the device; a step renders
// the next indices on the active list (render_device_body with the list in place of d_work), then estimates every
// 8x8 block's error and compacts the list.  The host reads two ints per step: the new list length and the number
// of blocks not converged.
namespace {
int adaptive_check_desc(rt_ctx* c, const rt_adaptive_desc* d, bool counts) {
    if (counts) {
        if (d->min_samples < 2) return fail(c, RT_E_ARG, "adaptive: min_samples must be at least 2 (a variance needs two samples)");
        if (d->step_samples < 1) return fail(c, RT_E_ARG, "adaptive: step_samples must be at least 1");
        if (d->max_samples < d->min_samples) return fail(c, RT_E_ARG, "adaptive: max_samples is below min_samples");
        // (indices past spp: PermutationElement's cycle walk need not end for strata counts that are no power of two)
        if (d->max_samples > dev_sampler(c).spp)
            return fail(c, RT_E_ARG, "adaptive: max_samples exceeds the sampler's samples per pixel");
    }
    if (!std::isfinite(d->rel_error) || d->rel_error < 0) return fail(c, RT_E_ARG, "adaptive: rel_error must be finite and >= 0");
    if (!std::isfinite(d->abs_floor) || d->abs_floor < 0) return fail(c, RT_E_ARG, "adaptive: abs_floor must be finite and >= 0");
    return RT_OK;
}

int adaptive_blocks(const rt_ctx* c) { return ((c->film.res_x + 7) / 8) * ((c->film.res_y + 7) / 8); }

// the estimate's outputs, the compaction's scratch and both active lists for the current film and work list
int adaptive_reserve(rt_ctx* c) {
    rt_ctx::Adaptive& a = c->ad;
    const size_t nb = (size_t)adaptive_blocks(c), nw = (size_t)adaptive_waves(c->n_work);
    HIPCHK(c, a.block_error.reserve(nb)); HIPCHK(c, a.converged.reserve(nb));
    HIPCHK(c, a.wave_count.reserve(nw)); HIPCHK(c, a.wave_offset.reserve(nw));
    HIPCHK(c, a.totals.reserve(2));
    HIPCHK(c, a.active[0].reserve((size_t)c->n_work)); HIPCHK(c, a.active[1].reserve((size_t)c->n_work));
    return RT_OK;
}

// block errors and flags from (film, mom), by the plain estimate or the guided one, then in[0, n)
// compacted into out; blocks until the counts are read
int adaptive_select(rt_ctx* c, const float4* film, const float2* mom, const rt_adaptive_desc& d, const int* in, int n,
                    int* out, int* n_out, int* n_blocks, hipStream_t st,
                    const rt_ctx::Adaptive::Guide& guide = rt_ctx::Adaptive::Guide{}) {
    rt_ctx::Adaptive& a = c->ad;
    const AdaptiveIO io{c->film.res_x, c->film.res_y, film, mom, d.rel_error, d.abs_floor, a.block_error.get(),
                        a.converged.get(), a.totals.get()};
    int t[2] = {0, 0};
    if (guide.on) HIPCHK(c, launch_temporal_error(st, io, guide.rec, guide.max_history));
    else HIPCHK(c, launch_adaptive_error(st, io));
    HIPCHK(c, launch_adaptive_compact(st, io, in, n, out, a.wave_count.get(), a.wave_offset.get()));
    HIPCHK(c, hipMemcpyAsync(t, a.totals.get(), sizeof(t), hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    *n_out = t[0];
    *n_blocks = t[1];
    return RT_OK;
}

void adaptive_release(rt_ctx* c) {
    c->ad = rt_ctx::Adaptive{};  // (hipFree waits for the work that still uses the buffers)
}
}  // namespace

// frame_owned: the session is the one a temporal frame runs (rt_temporal_frame), which alone may open one while a
// temporal session is live; the public rt_adaptive_begin passes false
static int impl_rt_adaptive_begin(rt_ctx* c, const rt_adaptive_desc* d, bool frame_owned) {
    if (!c) return RT_E_ARG;
    if (!d) return fail(c, RT_E_ARG, "adaptive: null descriptor");
    int rc = check_ready(c);
    if (rc) return rc;
    if (!c->peers.empty()) return fail(c, RT_E_STATE, "adaptive sampling supports one-device contexts only");
    rt_ctx::Adaptive& a = c->ad;
    if (a.live) return fail(c, RT_E_STATE, "an adaptive session is already open (rt_adaptive_end first)");
    if (c->tp.live && !frame_owned)
        return fail(c, RT_E_STATE, "a temporal session is open: its frames own the adaptive session (rt_temporal_end first)");
    if ((rc = adaptive_check_desc(c, d, true))) return rc;
    hipSetDevice(c->device);
    if ((rc = build_work(c))) return rc;
    if ((rc = adaptive_reserve(c))) return rc;
    const size_t n = (size_t)c->film.res_x * c->film.res_y;
    HIPCHK(c, a.film.reserve(n));
    HIPCHK(c, a.mom.reserve(n));
    hipStream_t st = c->stream;
    rc = ordered(c, st, [&]() -> int {
        HIPCHK(c, hipMemsetAsync(a.film.get(), 0, n * sizeof(float4), st));
        HIPCHK(c, hipMemsetAsync(a.mom.get(), 0, n * sizeof(float2), st));
        HIPCHK(c, hipMemsetAsync(a.block_error.get(), 0, (size_t)adaptive_blocks(c) * sizeof(float), st));
        if (c->n_work)
            HIPCHK(c, hipMemcpyAsync(a.active[0].get(), c->d_work.get(), (size_t)c->n_work * sizeof(int),
                                     hipMemcpyDeviceToDevice, st));
        return RT_OK;
    });
    if (rc) return rc;
    a.cur = 0;
    a.desc = *d;
    a.info = rt_adaptive_info{};
    a.info.active_pixels = c->n_work;
    a.live = true;
    return RT_OK;
}

static int impl_rt_adaptive_step(rt_ctx* c, rt_adaptive_info* info) {
    if (!c) return RT_E_ARG;
    rt_ctx::Adaptive& a = c->ad;
    if (!a.live) return fail(c, RT_E_STATE, "no adaptive session is open (rt_adaptive_begin first)");
    if (a.info.active_pixels > 0 && a.info.index_done < a.desc.max_samples) {
        int rc = check_ready(c);
        if (rc) return rc;
        if (a.desc.max_samples > dev_sampler(c).spp)
            return fail(c, RT_E_STATE, "adaptive: the sampler now has fewer samples per pixel than max_samples");
        hipSetDevice(c->device);
        const int ib = a.info.index_done;
        const int k = a.info.iterations == 0 ? a.desc.min_samples : a.desc.step_samples;
        const int ie = ib + std::min(k, a.desc.max_samples - ib);
        const int n = a.info.active_pixels;
        hipStream_t st = c->stream;
        int n_out = 0, n_blocks = 0;
        rc = ordered(c, st, [&]() -> int {
            const PassTarget active{a.active[a.cur].get(), n, a.mom.get()};
            if (int rc = render_device_body(c, ib, ie, a.film.get(), st, active)) return rc;
            // (the estimate is all a guided frame's step does differently)
            return adaptive_select(c, a.film.get(), a.mom.get(), a.desc, active.work, n, a.active[a.cur ^ 1].get(), &n_out,
                                   &n_blocks, st, a.guide);
        });
        if (rc) return rc;
        a.cur ^= 1;
        a.info.samples += (int64_t)n * (ie - ib);
        a.info.iterations += 1;
        a.info.index_done = ie;
        a.info.active_pixels = n_out;
        a.info.active_blocks = n_blocks;
    }
    if (info) *info = a.info;
    return RT_OK;
}

static int impl_rt_adaptive_read(rt_ctx* c, rt_pixel* film, rt_moment* mom, float* block_error, int32_t* active,
                                 int* n_active) {
    if (!c) return RT_E_ARG;
    rt_ctx::Adaptive& a = c->ad;
    if (!a.live) return fail(c, RT_E_STATE, "no adaptive session is open (rt_adaptive_begin first)");
    hipSetDevice(c->device);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const size_t n = (size_t)c->film.res_x * c->film.res_y;
    if (film) HIPCHK(c, hipMemcpy(film, a.film.get(), n * sizeof(float4), hipMemcpyDeviceToHost));
    if (mom) HIPCHK(c, hipMemcpy(mom, a.mom.get(), n * sizeof(float2), hipMemcpyDeviceToHost));
    if (block_error)
        HIPCHK(c, hipMemcpy(block_error, a.block_error.get(), (size_t)adaptive_blocks(c) * sizeof(float),
                            hipMemcpyDeviceToHost));
    if (active && a.info.active_pixels > 0)
        HIPCHK(c, hipMemcpy(active, a.active[a.cur].get(), (size_t)a.info.active_pixels * sizeof(int),
                            hipMemcpyDeviceToHost));
    if (n_active) *n_active = a.info.active_pixels;
    return RT_OK;
}

static int impl_rt_adaptive_end(rt_ctx* c) {
    if (!c) return RT_E_ARG;
    if (!c->ad.live) return fail(c, RT_E_STATE, "no adaptive session is open");
    hipSetDevice(c->device);
    adaptive_release(c);
    return RT_OK;
}

static int impl_rt_render_adaptive(rt_ctx* c, const rt_adaptive_desc* d, rt_pixel* film, rt_moment* mom,
                                   rt_adaptive_info* info) {
    int rc = impl_rt_adaptive_begin(c, d, false);
    if (rc) return rc;
    rt_adaptive_info cur{};
    do {
        rc = impl_rt_adaptive_step(c, &cur);
    } while (!rc && cur.active_pixels > 0 && cur.index_done < d->max_samples);
    if (!rc) rc = impl_rt_adaptive_read(c, film, mom, nullptr, nullptr, nullptr);
    if (rc) {  // close the session, keep the failing call's message
        const std::string msg = c->err;
        impl_rt_adaptive_end(c);
        return fail(c, rc, msg);
    }
    if (info) *info = cur;
    return impl_rt_adaptive_end(c);
}

static int impl_rt_debug_adaptive_select(rt_ctx* c, const rt_adaptive_desc* d, const rt_pixel* film,
                                         const rt_moment* mom, float* block_error, int32_t* active, int* n_active) {
    if (!c) return RT_E_ARG;
    if (!d || !film || !mom) return fail(c, RT_E_ARG, "adaptive select: descriptor, film and moments are required");
    if (!c->have_film) return fail(c, RT_E_STATE, "film not set");
    if (!c->peers.empty()) return fail(c, RT_E_STATE, "adaptive sampling supports one-device contexts only");
    if (c->ad.live) return fail(c, RT_E_STATE, "rt_debug_adaptive_select during an adaptive session");
    int rc = adaptive_check_desc(c, d, false);
    if (rc) return rc;
    hipSetDevice(c->device);
    if ((rc = build_work(c))) return rc;
    if ((rc = adaptive_reserve(c))) return rc;
    const size_t n = (size_t)c->film.res_x * c->film.res_y;
    DevBuf<float4> df;
    DevBuf<float2> dm;
    rt_ctx::Adaptive& a = c->ad;
    hipStream_t st = c->stream;
    int n_out = 0, n_blocks = 0;
    rc = ordered(c, st, [&]() -> int {
        int rc;
        if ((rc = stage_in(c, df, film, n, st)) || (rc = stage_in(c, dm, mom, n, st))) return rc;
        return adaptive_select(c, df.get(), dm.get(), *d, c->d_work.get(), c->n_work, a.active[0].get(), &n_out, &n_blocks,
                               st);
    });
    if (rc) return rc;
    if (block_error)
        HIPCHK(c, hipMemcpy(block_error, a.block_error.get(), (size_t)adaptive_blocks(c) * sizeof(float),
                            hipMemcpyDeviceToHost));
    if (active && n_out > 0)
        HIPCHK(c, hipMemcpy(active, a.active[0].get(), (size_t)n_out * sizeof(int), hipMemcpyDeviceToHost));
    if (n_active) *n_active = n_out;
    adaptive_release(c);
    return RT_OK;
}

// ---- denoiser: the feature pass reuses the reference-mode workspace and the generate / trace kernels;
// the filter runs on device arrays (an adaptive session's own, or staged copies of the caller's host arrays).
namespace {
// chain_depth as the public calls take it: d or d | RT_CHAIN_CURVED with d in 0..RT_CHAIN_MAX
bool chain_depth_valid(int chain_depth) {
    const int d = chain_depth & ~RT_CHAIN_CURVED;
    return d >= 0 && d <= kChainMax;
}
int chain_check_depth(rt_ctx* c, int chain_depth) {
    if (!chain_depth_valid(chain_depth))
        return fail(c, RT_E_ARG, "chain_depth must be 0..RT_CHAIN_MAX, optionally | RT_CHAIN_CURVED");
    return RT_OK;
}

// The sensor albedo table of the scene's materials and texels, on first use after the scene, its textures or the
// sensor changed.
int ensure_albedo_table(rt_ctx* c, hipStream_t st) {
    if (c->alb.valid) return RT_OK;
    const size_t n = (size_t)c->dsc.n_materials + c->tx.n_texels;
    HIPCHK(c, c->alb.table.reserve(n));
    HIPCHK(c, launch_albedo_bake(st, c->d_spec.get(), c->dsc.n_materials, c->dsc.materials, (int)c->tx.n_texels,
                                 c->tx.texels.get(), c->alb.table.get()));
    // a conductor's entry is (1, 1, 1), which leaves it un-demodulated: its colour depends on the angle, and it has no
    // texture detail to protect.  This loop is the only place that knows the rule: a test in k_albedo_film
    // or k_albedo_bake would change those kernels' register figures for every scene
    static const float4 one = make_float4(1.f, 1.f, 1.f, 0.f);
    for (int m = 0; m < c->dsc.n_materials && m < (int)c->tx.mat_flags.size(); ++m)
        if (c->tx.mat_flags[m] & (4 | 8))  // (a rough glass as well, DESIGN.md §3m: it has no colour of its own)
            HIPCHK(c, hipMemcpyAsync(c->alb.table.get() + m, &one, sizeof(one), hipMemcpyHostToDevice, st));
    c->alb.valid = true;
    return RT_OK;
}

// Features of indices [ib, ie) of the full work list added to the device feature film: per batch the camera rays, the
// closest hits as the current integrator's first trace finds them (reference: the culled tile set when the scene
// culls; path: every triangle), then k_feature_film.  Batches as render_device_body's reference loop.
// pos (may be null): the position film of the same hits.
// chain_depth > 0 under a path integrator: the guides of the end of each sample's specular chain.  Per
// level, k_chain_level over the level's queue and, for the rays it appends, the trace of a path bounce; then
// k_chain_film.  The chain's per-slot state uses the reference workspace's wavelength and pdf arrays, which k_generate
// fills and the feature pass never reads.
// alb (may be null): the albedo film of the batch's FIRST hits, added right after the first trace, before
// a chain's levels overwrite the hit records.

int features_device(rt_ctx* c, int ib, int ie, float4* feat, hipStream_t st, float4* pos = nullptr,
                    int chain_arg = 0, float4* alb = nullptr) {
    int rc;
    if ((rc = chain_check_depth(c, chain_arg))) return rc;
    const int chain_depth = chain_arg & ~RT_CHAIN_CURVED;
    const bool curved = (chain_arg & RT_CHAIN_CURVED) != 0;  // (without effect at depth 0)
    if ((rc = pass_checks(c, ib, ie))) return rc;
    if ((rc = build_work(c))) return rc;
    const int n_work = c->n_work;
    const BatchPlan bp = plan_batches(pass_facts(c, n_work, ib, ie), c->knobs);
    if (!bp.nbatch) return RT_OK;
    const bool path = bp.path, dyn = bp.dyn;  // dyn: the bounce rays' trace takes per-wave tickets
    const int B = bp.B, nsh = bp.nsh;
    const size_t ncap = bp.ncap;
    const DevSampler smp = dev_sampler(c);
    const DevCamera cam = dev_camera(c->cam);
    const DevFilm fd = dev_film(c);
    const DevScene sc = pass_scene(c, bp);
    Work& w = c->ws[0];
    if ((rc = ensure_workspace(c, w, ncap, false))) return rc;
    if (alb && (rc = ensure_albedo_table(c, st))) return rc;
    // (the reference integrator consults no material: every chain has length 0)
    const bool chain = path && chain_depth > 0;
    float eta_bk7 = 0.f;
    if (chain) {
        if (ncap > ((size_t)1 << kChainSlotBits)) return fail(c, RT_E_LIMIT, "chain pass: more than 2^28 samples per batch");
        HIPCHK(c, w.b.chainRay.reserve(4 * ncap));
        if (curved) HIPCHK(c, w.b.chainRec.reserve((size_t)(kChainMax + 1) * ncap));
        HIPCHK(c, w.chain_ctr.reserve((size_t)(kChainMax + 1) * kQRegion));
        if (dyn) HIPCHK(c, w.tfb.reserve(ncap));
        eta_bk7 = c->hs.BK7.query(550.f);
    }
    for (int b0 = ib; b0 < ie; b0 += B) {
        const int nIdx = std::min(B, ie - b0);
        const int nS = nIdx * n_work;
        const SampleIds ids = sample_ids(c->d_work.get(), n_work, b0);
        RefIO r = ref_io(c, w.b, nS, nsh);
        if (path) r.tio.set = 0;  // the path integrator traces every triangle
        hipEvent_t e0 = ev_start(c, st);
        HIPCHK(c, launch_generate(st, c->grid, nS, ids, cam, smp, fd, r.go));
        ev_mark(c, st, ST_GEN, e0);
        e0 = ev_start(c, st);
        HIPCHK(c, launch_trace_closest(st, 0, sc.qcap, lane_scene(sc, w), r.tio, c->d_ctr.get()));
        ev_mark(c, st, ST_TRACE, e0);
        if (alb) {
            const AlbedoFilmIO aio{c->d_work.get(), n_work, nIdx, w.b.hitB.get(), w.b.hitPrim.get(), c->alb.table.get(),
                                   c->tx.live ? c->tx.dev.get() : nullptr, path ? 0 : 1, alb};
            HIPCHK(c, launch_albedo_film(st, sc, aio));
        }
        if (!chain) {
            const FeatureIO fio{c->d_work.get(), n_work, nIdx, w.b.rayD(), 1, w.b.hitB.get(), w.b.hitPrim.get(), feat,
                                w.b.rayO(), pos};
            HIPCHK(c, launch_feature_film(st, sc, fio));
            continue;
        }
        const Batch& b = w.b;
        const DevScene dsl = lane_scene(sc, w);
        int* const ctr = w.chain_ctr.get();
        HIPCHK(c, hipMemsetAsync(ctr, 0, (size_t)chain_depth * kQRegion * sizeof(int), st));
        ChainIO cio{};
        cio.hitB = b.hitB.get(); cio.hitPrim = b.hitPrim.get();
        cio.depth = chain_depth;
        cio.eta_bk7 = eta_bk7;
        cio.n[0] = b.lamB.get(); cio.n[1] = b.pdfA.get(); cio.n[2] = b.pdfB.get();
        cio.res = b.lamA.get();
        if (curved) {
            cio.curved = 1;
            cio.kappa = c->d_kappa;
            for (int k = 0; k < kChainMax; ++k) cio.rec[k] = b.chainRec.get() + (size_t)k * ncap;
            cio.seg = b.chainRec.get() + (size_t)kChainMax * ncap;
        }
        const int S = shard_stride(nS, nsh);
        for (int level = 0; level <= chain_depth; ++level) {
            int* const reg = level > 0 ? ctr + (size_t)(level - 1) * kQRegion : nullptr;  // this level's queue
            cio.level = level;
            cio.q = level > 0 ? QueueView{reg + kQLen, S, 0, nsh} : QueueView{nullptr, S, nS, nsh};
            cio.ray = level > 0 ? b.chainRay.get() + 2 * ncap * (size_t)((level - 1) & 1) : b.rayO();
            cio.nray = b.chainRay.get() + 2 * ncap * (size_t)(level & 1);
            cio.nlen = ctr + (size_t)level * kQRegion + kQLen;
            if (level > 0) {  // the continuation rays, traced as a path bounce: every triangle, every shape, no tMax
                TraceIO tio{cio.ray, cio.ray + 1, cio.q, 0, b.hitB.get(), b.hitPrim.get(),
                            dyn ? reg + kQTraceTicket : nullptr, 1};
                if (dyn) {
                    tio.fb_pos = w.tfb.get();
                    tio.fb_len = reg + kQTraceFallback;
                }
                if ((rc = trace_with_fallback(c, st, dsl, tio, bp.trace_fallback))) return rc;
            }
            HIPCHK(c, launch_chain_level(st, c->grid, dsl, cio));
        }
        const ChainFilmIO fio{c->d_work.get(), n_work, nIdx, b.rayO(), b.lamA.get(), feat, pos};
        HIPCHK(c, launch_chain_film(st, fio));
    }
    return RT_OK;
}

int denoise_check_desc(rt_ctx* c, const rt_denoise_desc* d) {
    if (d->iterations < 1 || d->iterations > 6) return fail(c, RT_E_ARG, "denoise: iterations must be 1..6");
    if (d->feature_samples < 1) return fail(c, RT_E_ARG, "denoise: feature_samples must be at least 1");
    if (d->normal_power_log2 < 0 || d->normal_power_log2 > 8)
        return fail(c, RT_E_ARG, "denoise: normal_power_log2 must be 0..8");
    if (!std::isfinite(d->sigma_l) || !(d->sigma_l > 0) || !std::isfinite(d->sigma_z) || !(d->sigma_z > 0))
        return fail(c, RT_E_ARG, "denoise: sigma_l and sigma_z must be finite and > 0");
    if (!std::isfinite(d->lum_floor) || d->lum_floor < 0 || !std::isfinite(d->depth_floor) || d->depth_floor < 0)
        return fail(c, RT_E_ARG, "denoise: lum_floor and depth_floor must be finite and >= 0");
    if (!chain_depth_valid(d->chain_depth))
        return fail(c, RT_E_ARG, "denoise: chain_depth must be 0..RT_CHAIN_MAX, optionally | RT_CHAIN_CURVED");
    return RT_OK;
}

// prepare and the iterations over device arrays of res_x * res_y; out = (c n, n), var (may be null) = the last variance
// alb (may be null): the albedo film to demodulate by, floored at albedo_floor: the albedo prepare, every
// iteration into the ping-pong, and the remodulating finish
int denoise_device(rt_ctx* c, const rt_denoise_desc& d, int res_x, int res_y, const float4* film, const float2* mom,
                   const float4* feat, float4* out, float* var, hipStream_t st, const float4* alb = nullptr,
                   float albedo_floor = 0.f) {
    rt_ctx::Denoise& w = c->dn;
    const size_t n = (size_t)res_x * res_y;
    if (alb) HIPCHK(c, w.a.reserve(n));
    const DemodIO dm{alb, w.a.get(), albedo_floor};
    HIPCHK(c, w.g.reserve(n)); HIPCHK(c, w.gz.reserve(n));
    HIPCHK(c, w.cv[0].reserve(n)); HIPCHK(c, w.cv[1].reserve(n));
    DenoiseIO io{};
    io.res_x = res_x; io.res_y = res_y;
    io.film = film; io.mom = mom; io.feat = feat;
    io.kf = (float)d.feature_samples;
    io.g = w.g.get(); io.gz = w.gz.get();
    io.normal_power_log2 = d.normal_power_log2;
    io.sigma_l = d.sigma_l; io.sigma_z = d.sigma_z; io.lum_floor = d.lum_floor; io.depth_floor = d.depth_floor;
    io.cv_out = w.cv[0].get();
    HIPCHK(c, alb ? launch_denoise_prepare_albedo(st, io, dm) : launch_denoise_prepare(st, io));
    for (int i = 0; i < d.iterations; ++i) {
        io.cv_in = w.cv[i & 1].get();
        io.cv_out = w.cv[(i & 1) ^ 1].get();
        io.step = 1 << i;
        if (i == d.iterations - 1 && !alb) {  // the finish is fused into the last iteration
            io.out = out;
            io.var_out = var;
        }
        HIPCHK(c, launch_denoise_iter(st, io, c->knobs.denoise_lds != 0));
    }
    if (alb) HIPCHK(c, launch_denoise_finish_albedo(st, io, dm, io.cv_out, out, var));
    return RT_OK;
}

int albedo_floor_check(rt_ctx* c, float albedo_floor) {
    if (!std::isfinite(albedo_floor) || !(albedo_floor > 0.f) || albedo_floor > 1.f)
        return fail(c, RT_E_ARG, "denoise: albedo_floor must be finite and in (0, 1]");
    return RT_OK;
}

bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

// A call's host arrays (a null one takes no part).  overlap_kind: 1 when an output overlaps an input, else 2 when two
// outputs overlap, else 0.
struct HostRange {
    const void* p;
    size_t bytes;
};
int overlap_kind(std::initializer_list<HostRange> outs, std::initializer_list<HostRange> ins) {
    const auto hit = [](const HostRange& a, const HostRange& b) {
        return a.p && b.p && ranges_overlap(a.p, a.bytes, b.p, b.bytes);
    };
    for (const HostRange& o : outs)
        for (const HostRange& i : ins)
            if (hit(o, i)) return 1;
    for (const HostRange* a = outs.begin(); a != outs.end(); ++a)
        for (const HostRange* b = a + 1; b != outs.end(); ++b)
            if (hit(*a, *b)) return 2;
    return 0;
}
}  // namespace

// rt_render_features (with_pos false: pos is not looked at), rt_render_features_pos, rt_render_features_chain and, with
// with_alb, rt_render_features_albedo
static int impl_rt_render_features(rt_ctx* c, int ib, int ie, rt_feature* feat, rt_position* pos, bool with_pos,
                                   int chain_depth, rt_albedo* alb, bool with_alb) {
    if (!c || !feat || (with_pos && !pos) || (with_alb && !alb)) return RT_E_ARG;
    int rc = chain_check_depth(c, chain_depth);
    if (rc) return rc;
    if ((rc = check_ready(c))) return rc;
    if (!c->peers.empty()) return fail(c, RT_E_STATE, "the feature pass supports one-device contexts only");
    hipSetDevice(c->device);
    const size_t n = (size_t)c->film.res_x * c->film.res_y;
    if (overlap_kind({{feat, n * sizeof(rt_feature)}, {with_pos ? pos : nullptr, n * sizeof(rt_position)},
                      {with_alb ? alb : nullptr, n * sizeof(rt_albedo)}}, {}))
        return fail(c, RT_E_ARG, with_alb ? "the feature, position and albedo films overlap"
                                          : "the feature film and the position film overlap");
    DevBuf<float4>& d_feat = c->dn.feat;  // (rt_denoise's feature staging, and the temporal entries' position staging)
    DevBuf<float4>& d_pos = c->tp.s_pos;
    DevBuf<float4>& d_alb = c->dn.alb;
    hipStream_t st = c->stream;
    rc = ordered(c, st, [&]() -> int {
        int rc;
        if ((rc = stage_in(c, d_feat, feat, n, st)) || (with_pos && (rc = stage_in(c, d_pos, pos, n, st))) ||
            (with_alb && (rc = stage_in(c, d_alb, alb, n, st))))
            return rc;
        return features_device(c, ib, ie, d_feat.get(), st, with_pos ? d_pos.get() : nullptr, chain_depth,
                               with_alb ? d_alb.get() : nullptr);
    });
    if (rc || (rc = stage_out(c, feat, d_feat, n, st)) || (with_pos && (rc = stage_out(c, pos, d_pos, n, st))) ||
        (with_alb && (rc = stage_out(c, alb, d_alb, n, st))))
        return rc;
    HIPCHK(c, hipStreamSynchronize(st));
    return RT_OK;
}

// rt_denoise and, with with_alb, rt_denoise_albedo
static int impl_rt_denoise(rt_ctx* c, const rt_denoise_desc* d, int res_x, int res_y, const rt_pixel* film,
                           const rt_moment* mom, const rt_feature* feat, rt_pixel* out, float* variance_out,
                           const rt_albedo* alb, bool with_alb, float albedo_floor) {
    if (!c) return RT_E_ARG;
    if (!d || !film || !mom || !feat || !out || (with_alb && !alb))
        return fail(c, RT_E_ARG, with_alb ? "denoise: descriptor, film, moments, features, albedo and out are required"
                                          : "denoise: descriptor, film, moments, features and out are required");
    if (res_x <= 0 || res_y <= 0) return fail(c, RT_E_ARG, "denoise: the resolution must be positive");
    if ((int64_t)res_x * res_y > ((int64_t)1 << 28)) return fail(c, RT_E_LIMIT, "denoise: more than 2^28 pixels");
    int rc = denoise_check_desc(c, d);
    if (rc || (with_alb && (rc = albedo_floor_check(c, albedo_floor)))) return rc;
    const size_t n = (size_t)res_x * res_y;
    if (const int k = overlap_kind({{out, n * sizeof(rt_pixel)}, {variance_out, n * sizeof(float)}},
                                   {{film, n * sizeof(rt_pixel)}, {mom, n * sizeof(rt_moment)}, {feat, n * sizeof(rt_feature)},
                                    {with_alb ? alb : nullptr, n * sizeof(rt_albedo)}}))
        return fail(c, RT_E_ARG, k == 1 ? "denoise: an output overlaps an input" : "denoise: variance_out overlaps out");
    hipSetDevice(c->device);
    rt_ctx::Denoise& w = c->dn;
    HIPCHK(c, w.out.reserve(n)); HIPCHK(c, w.var.reserve(n));
    hipStream_t st = c->stream;
    rc = ordered(c, st, [&]() -> int {
        int rc;
        if ((rc = stage_in(c, w.film, film, n, st)) || (rc = stage_in(c, w.mom, mom, n, st)) ||
            (rc = stage_in(c, w.feat, feat, n, st)) || (with_alb && (rc = stage_in(c, w.alb, alb, n, st))))
            return rc;
        return denoise_device(c, *d, res_x, res_y, w.film.get(), w.mom.get(), w.feat.get(), w.out.get(), w.var.get(), st,
                              with_alb ? w.alb.get() : nullptr, albedo_floor);
    });
    if (rc || (rc = stage_out(c, out, w.out, n, st)) || (variance_out && (rc = stage_out(c, variance_out, w.var, n, st))))
        return rc;
    HIPCHK(c, hipStreamSynchronize(st));
    return RT_OK;
}

// rt_adaptive_denoise and, with with_alb, rt_adaptive_denoise_albedo
static int impl_rt_adaptive_denoise(rt_ctx* c, const rt_denoise_desc* d, rt_pixel* film_out, bool with_alb,
                                    float albedo_floor) {
    if (!c) return RT_E_ARG;
    if (!d || !film_out) return fail(c, RT_E_ARG, "adaptive denoise: descriptor and film_out are required");
    rt_ctx::Adaptive& a = c->ad;
    if (!a.live) return fail(c, RT_E_STATE, "no adaptive session is open (rt_adaptive_begin first)");
    int rc = check_ready(c);
    if (rc) return rc;
    if ((rc = denoise_check_desc(c, d)) || (with_alb && (rc = albedo_floor_check(c, albedo_floor)))) return rc;
    if (d->feature_samples > dev_sampler(c).spp)
        return fail(c, RT_E_ARG, "adaptive denoise: feature_samples exceeds the sampler's samples per pixel");
    hipSetDevice(c->device);
    const size_t n = (size_t)c->film.res_x * c->film.res_y;
    HIPCHK(c, a.feat.reserve(n));
    if (with_alb) HIPCHK(c, a.alb.reserve(n));
    HIPCHK(c, c->dn.out.reserve(n));
    hipStream_t st = c->stream;
    rc = ordered(c, st, [&]() -> int {
        // once per session (again only if the caller changes k or the chain depth); the albedo film is rendered with the
        // features, which come out as the feature pass alone leaves them
        const bool feat_ok = a.feat_k == d->feature_samples && a.feat_chain == d->chain_depth;
        const bool alb_ok = !with_alb || (a.alb_k == d->feature_samples && a.alb_chain == d->chain_depth);
        if (!feat_ok || !alb_ok) {
            a.feat_k = 0;
            if (hipMemsetAsync(a.feat.get(), 0, n * sizeof(float4), st) != hipSuccess)
                return fail(c, RT_E_HIP, "feature film memset");
            if (with_alb) {
                a.alb_k = 0;
                if (hipMemsetAsync(a.alb.get(), 0, n * sizeof(float4), st) != hipSuccess)
                    return fail(c, RT_E_HIP, "albedo film memset");
            }
            if (int rc = features_device(c, 0, d->feature_samples, a.feat.get(), st, nullptr, d->chain_depth,
                                         with_alb ? a.alb.get() : nullptr))
                return rc;
            a.feat_k = d->feature_samples;
            a.feat_chain = d->chain_depth;
            if (with_alb) {
                a.alb_k = d->feature_samples;
                a.alb_chain = d->chain_depth;
            }
        }
        return denoise_device(c, *d, c->film.res_x, c->film.res_y, a.film.get(), a.mom.get(), a.feat.get(),
                              c->dn.out.get(), nullptr, st, with_alb ? a.alb.get() : nullptr, albedo_floor);
    });
    if (rc || (rc = stage_out(c, film_out, c->dn.out, n, st))) return rc;
    HIPCHK(c, hipStreamSynchronize(st));
    return RT_OK;
}

// ---- temporal accumulation: the stage runs on device arrays (a session's own, or staged copies of
// the caller's host arrays); a frame is an adaptive session, a feature + position pass, the stage and the filter.
namespace {
int temporal_check_desc(rt_ctx* c, const rt_temporal_desc* d) {
    if (!std::isfinite(d->normal_min) || d->normal_min < -1.f || d->normal_min > 1.f)
        return fail(c, RT_E_ARG, "temporal: normal_min must be in [-1, 1]");
    if (!std::isfinite(d->plane_rel) || d->plane_rel < 0) return fail(c, RT_E_ARG, "temporal: plane_rel must be finite and >= 0");
    if (!(d->max_history >= 1.f)) return fail(c, RT_E_ARG, "temporal: max_history must be at least 1");
    if (d->feature_samples < 1) return fail(c, RT_E_ARG, "temporal: feature_samples must be at least 1");
    if (!chain_depth_valid(d->chain_depth))
        return fail(c, RT_E_ARG, "temporal: chain_depth must be 0..RT_CHAIN_MAX, optionally | RT_CHAIN_CURVED");
    return RT_OK;
}

// a frame's four device arrays: the current frame's, or a history's
struct TemporalSet {
    const float4* film;
    const float2* mom;
    const float4 *feat, *pos;
};

// the guides, the history and the descriptor's parameters of a kernel launch (hist null: no history, M not read)
TemporalIO temporal_io(const rt_temporal_desc& d, int res_x, int res_y, const TemporalSet& cur, const TemporalSet* hist,
                       const float* M) {
    TemporalIO io{};
    io.res_x = res_x; io.res_y = res_y;
    io.feat = cur.feat; io.pos = cur.pos;
    if (hist) {
        io.hfilm = hist->film; io.hmom = hist->mom; io.hfeat = hist->feat; io.hpos = hist->pos;
        std::memcpy(io.M, M, sizeof(io.M));
    }
    io.kf = (float)d.feature_samples;
    io.normal_min = d.normal_min; io.plane_rel = d.plane_rel; io.max_history = d.max_history;
    return io;
}

// The stage over device arrays of res_x * res_y (hist null: no history, M not read); counts[T_NCLASSES] read back
// after the kernel (blocks until then).
int temporal_device(rt_ctx* c, const rt_temporal_desc& d, int res_x, int res_y, const TemporalSet& cur,
                    const TemporalSet* hist, const float* M, float4* out_film, float2* out_mom, int* counts, hipStream_t st) {
    rt_ctx::Temporal& t = c->tp;
    HIPCHK(c, t.ctr.reserve(kTemporalCtrWords));
    HIPCHK(c, hipMemsetAsync(t.ctr.get(), 0, kTemporalCtrWords * sizeof(unsigned long long), st));
    TemporalIO io = temporal_io(d, res_x, res_y, cur, hist, M);
    io.film = cur.film; io.mom = cur.mom;
    io.out_film = out_film; io.out_mom = out_mom;
    io.ctr = t.ctr.get();
    HIPCHK(c, launch_temporal_accumulate(st, io));
    std::vector<unsigned long long> raw(kTemporalCtrWords);
    HIPCHK(c, hipMemcpyAsync(raw.data(), t.ctr.get(), kTemporalCtrWords * sizeof(unsigned long long),
                             hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    for (int k = 0; k < T_NCLASSES; ++k) {
        unsigned long long s = 0;
        for (int u = 0; u < kCtrSubs; ++u) s += raw[ctr_word(k, u)];
        counts[k] = (int)s;
    }
    return RT_OK;
}

void temporal_fill_info(rt_temporal_info* info, int frames, const int* counts) {
    if (!info) return;
    info->frames = frames;
    info->reprojected = counts[T_REPROJECTED];
    info->disoccluded = counts[T_DISOCCLUDED];
    info->background = counts[T_BACKGROUND];
}

// what rt_temporal_accumulate and rt_temporal_block_error ask of their host arrays' shape: the history is all four
// arrays or none and comes with its matrix; the resolution.  *hist: a history is given.
int temporal_check_arrays(rt_ctx* c, const void* hfilm, const void* hmom, const void* hfeat, const void* hpos,
                          const float* M, int res_x, int res_y, bool* hist) {
    const int n_hist = (hfilm != nullptr) + (hmom != nullptr) + (hfeat != nullptr) + (hpos != nullptr);
    if (n_hist != 0 && n_hist != 4) return fail(c, RT_E_ARG, "temporal: the history is all four arrays or none");
    *hist = n_hist == 4;
    if (*hist && !M) return fail(c, RT_E_ARG, "temporal: a history needs its world-to-film matrix");
    if (res_x <= 0 || res_y <= 0) return fail(c, RT_E_ARG, "temporal: the resolution must be positive");
    if ((int64_t)res_x * res_y > ((int64_t)1 << 28)) return fail(c, RT_E_LIMIT, "temporal: more than 2^28 pixels");
    return RT_OK;
}
}  // namespace

static int impl_rt_temporal_accumulate(rt_ctx* c, const rt_temporal_desc* d, int res_x, int res_y, const rt_pixel* film,
                                       const rt_moment* mom, const rt_feature* feat, const rt_position* pos,
                                       const rt_pixel* hfilm, const rt_moment* hmom, const rt_feature* hfeat,
                                       const rt_position* hpos, const float* M, rt_pixel* out_film, rt_moment* out_mom,
                                       rt_temporal_info* info) {
    if (!c) return RT_E_ARG;
    if (!d || !film || !mom || !feat || !pos || !out_film || !out_mom)
        return fail(c, RT_E_ARG, "temporal: descriptor, film, moments, features, positions and both outputs are required");
    bool hist;
    int rc = temporal_check_arrays(c, hfilm, hmom, hfeat, hpos, M, res_x, res_y, &hist);
    if (rc || (rc = temporal_check_desc(c, d))) return rc;
    const size_t n = (size_t)res_x * res_y;
    const size_t b4 = n * sizeof(float4), b2 = n * sizeof(float2);
    if (const int k = overlap_kind({{out_film, b4}, {out_mom, b2}}, {{film, b4}, {mom, b2}, {feat, b4}, {pos, b4},
                                                                     {hfilm, b4}, {hmom, b2}, {hfeat, b4}, {hpos, b4}}))
        return fail(c, RT_E_ARG, k == 1 ? "temporal: an output overlaps an input" : "temporal: out_film overlaps out_mom");
    hipSetDevice(c->device);
    rt_ctx::Temporal& t = c->tp;
    HIPCHK(c, t.s_out.reserve(n)); HIPCHK(c, t.s_outm.reserve(n));
    hipStream_t st = c->stream;
    int counts[T_NCLASSES] = {};
    rc = ordered(c, st, [&]() -> int {
        int rc;
        if ((rc = stage_in(c, t.s_film, film, n, st)) || (rc = stage_in(c, t.s_mom, mom, n, st)) ||
            (rc = stage_in(c, t.s_feat, feat, n, st)) || (rc = stage_in(c, t.s_pos, pos, n, st)))
            return rc;
        if (hist && ((rc = stage_in(c, t.s_hfilm, hfilm, n, st)) || (rc = stage_in(c, t.s_hmom, hmom, n, st)) ||
                     (rc = stage_in(c, t.s_hfeat, hfeat, n, st)) || (rc = stage_in(c, t.s_hpos, hpos, n, st))))
            return rc;
        const TemporalSet cur{t.s_film.get(), t.s_mom.get(), t.s_feat.get(), t.s_pos.get()};
        const TemporalSet past{t.s_hfilm.get(), t.s_hmom.get(), t.s_hfeat.get(), t.s_hpos.get()};
        return temporal_device(c, *d, res_x, res_y, cur, hist ? &past : nullptr, M, t.s_out.get(), t.s_outm.get(), counts,
                               st);
    });
    if (rc || (rc = stage_out(c, out_film, t.s_out, n, st)) || (rc = stage_out(c, out_mom, t.s_outm, n, st))) return rc;
    HIPCHK(c, hipStreamSynchronize(st));
    temporal_fill_info(info, hist ? 1 : 0, counts);
    return RT_OK;
}

static int impl_rt_temporal_block_error(rt_ctx* c, const rt_temporal_desc* d, const rt_adaptive_desc* ad, int res_x,
                                        int res_y, const rt_pixel* film, const rt_moment* mom, const rt_feature* feat,
                                        const rt_position* pos, const rt_pixel* hfilm, const rt_moment* hmom,
                                        const rt_feature* hfeat, const rt_position* hpos, const float* M,
                                        float* block_error, int32_t* converged) {
    if (!c) return RT_E_ARG;
    if (!d || !ad || !film || !mom || !feat || !pos)
        return fail(c, RT_E_ARG, "temporal block error: both descriptors, film, moments, features and positions are required");
    bool hist;
    int rc = temporal_check_arrays(c, hfilm, hmom, hfeat, hpos, M, res_x, res_y, &hist);
    if (rc || (rc = temporal_check_desc(c, d)) || (rc = adaptive_check_desc(c, ad, false))) return rc;
    const size_t n = (size_t)res_x * res_y, nb = (size_t)((res_x + 7) / 8) * ((res_y + 7) / 8);
    hipSetDevice(c->device);
    rt_ctx::Temporal& t = c->tp;
    DevBuf<float> d_err;
    DevBuf<int> d_conv;
    HIPCHK(c, d_err.reserve(nb)); HIPCHK(c, d_conv.reserve(nb));
    if (hist) HIPCHK(c, t.rec.reserve(n));
    hipStream_t st = c->stream;
    rc = ordered(c, st, [&]() -> int {
        int rc;
        if ((rc = stage_in(c, t.s_film, film, n, st)) || (rc = stage_in(c, t.s_mom, mom, n, st))) return rc;
        if (hist) {  // (without one the guides take no part)
            if ((rc = stage_in(c, t.s_feat, feat, n, st)) || (rc = stage_in(c, t.s_pos, pos, n, st)) ||
                (rc = stage_in(c, t.s_hfilm, hfilm, n, st)) || (rc = stage_in(c, t.s_hmom, hmom, n, st)) ||
                (rc = stage_in(c, t.s_hfeat, hfeat, n, st)) || (rc = stage_in(c, t.s_hpos, hpos, n, st)))
                return rc;
            const TemporalSet cur{t.s_film.get(), t.s_mom.get(), t.s_feat.get(), t.s_pos.get()};
            const TemporalSet past{t.s_hfilm.get(), t.s_hmom.get(), t.s_hfeat.get(), t.s_hpos.get()};
            if (launch_temporal_reproject(st, temporal_io(*d, res_x, res_y, cur, &past, M), t.rec.get()) != hipSuccess)
                return fail(c, RT_E_HIP, "k_temporal_reproject");
        }
        const AdaptiveIO io{res_x, res_y, t.s_film.get(), t.s_mom.get(), ad->rel_error, ad->abs_floor, d_err.get(),
                            d_conv.get(), nullptr};
        if (launch_temporal_error(st, io, hist ? t.rec.get() : nullptr, d->max_history) != hipSuccess)
            return fail(c, RT_E_HIP, "k_temporal_error");
        return RT_OK;
    });
    if (rc || (block_error && (rc = stage_out(c, block_error, d_err, nb, st))) ||
        (converged && (rc = stage_out(c, converged, d_conv, nb, st))))
        return rc;
    HIPCHK(c, hipStreamSynchronize(st));
    return RT_OK;
}

static int impl_rt_temporal_begin(rt_ctx* c, const rt_temporal_desc* d) {
    if (!c) return RT_E_ARG;
    if (!d) return fail(c, RT_E_ARG, "temporal: null descriptor");
    int rc = check_ready(c);
    if (rc) return rc;
    if (!c->peers.empty()) return fail(c, RT_E_STATE, "temporal accumulation supports one-device contexts only");
    rt_ctx::Temporal& t = c->tp;
    if (t.live) return fail(c, RT_E_STATE, "a temporal session is already open (rt_temporal_end first)");
    if (c->ad.live) return fail(c, RT_E_STATE, "rt_temporal_begin inside an adaptive session (rt_adaptive_end first)");
    if ((rc = temporal_check_desc(c, d))) return rc;
    if (d->feature_samples > dev_sampler(c).spp)
        return fail(c, RT_E_ARG, "temporal: feature_samples exceeds the sampler's samples per pixel");
    hipSetDevice(c->device);
    const size_t n = (size_t)c->film.res_x * c->film.res_y;
    for (int k = 0; k < 2; ++k) {
        HIPCHK(c, t.film[k].reserve(n)); HIPCHK(c, t.mom[k].reserve(n));
        HIPCHK(c, t.feat[k].reserve(n)); HIPCHK(c, t.pos[k].reserve(n));
    }
    t.desc = *d;
    t.frames = 0;
    t.cur = 0;
    t.live = true;
    return RT_OK;
}

namespace {
// the frame's guides: the feature and position films of indices [0, feature_samples) into the non-history set
int temporal_frame_guides(rt_ctx* c, hipStream_t st) {
    rt_ctx::Temporal& t = c->tp;
    const int nx = t.cur ^ 1;
    const size_t n = (size_t)c->film.res_x * c->film.res_y;
    int rc = hipMemsetAsync(t.feat[nx].get(), 0, n * sizeof(float4), st) == hipSuccess &&
                     hipMemsetAsync(t.pos[nx].get(), 0, n * sizeof(float4), st) == hipSuccess
                 ? RT_OK : fail(c, RT_E_HIP, "feature and position film memset");
    if (!rc)
        rc = features_device(c, 0, t.desc.feature_samples, t.feat[nx].get(), st, t.pos[nx].get(), t.desc.chain_depth);
    return rc;
}

// the frame inside its adaptive session: steps, feature + position pass, the stage, the filter, the copy out.
// guided: the guides and the reprojection first, and the steps estimate on the accumulated film.
int temporal_frame_body(rt_ctx* c, const rt_adaptive_desc* ad, const rt_denoise_desc* dd, rt_pixel* film_out, int* counts,
                        bool guided, rt_adaptive_info* session) {
    rt_ctx::Temporal& t = c->tp;
    rt_ctx::Adaptive& a = c->ad;
    int rc;
    const int res_x = c->film.res_x, res_y = c->film.res_y, nx = t.cur ^ 1;
    const size_t n = (size_t)res_x * res_y;
    const bool hist = t.frames > 0;
    // the frame (its film and moments are the adaptive session's) and the history it is accumulated against
    const TemporalSet frame{a.film.get(), a.mom.get(), t.feat[nx].get(), t.pos[nx].get()};
    const TemporalSet last{t.film[t.cur].get(), t.mom[t.cur].get(), t.feat[t.cur].get(), t.pos[t.cur].get()};
    const TemporalSet* const past = hist ? &last : nullptr;
    hipStream_t st = c->stream;
    if (guided) {
        if (hist) HIPCHK(c, t.rec.reserve(n));
        rc = ordered(c, st, [&]() -> int {
            if (int rc = temporal_frame_guides(c, st)) return rc;
            if (hist && launch_temporal_reproject(st, temporal_io(t.desc, res_x, res_y, frame, past, t.M), t.rec.get()) !=
                            hipSuccess)
                return fail(c, RT_E_HIP, "k_temporal_reproject");
            return RT_OK;
        });
        if (rc) return rc;
        a.guide.on = true;
        a.guide.rec = hist ? t.rec.get() : nullptr;
        a.guide.max_history = t.desc.max_history;
    }
    rt_adaptive_info cur{};
    do {
        if ((rc = impl_rt_adaptive_step(c, &cur))) return rc;
    } while (cur.active_pixels > 0 && cur.index_done < ad->max_samples);
    if (session) *session = cur;
    if (dd) HIPCHK(c, c->dn.out.reserve(n));
    rc = ordered(c, st, [&]() -> int {
        int rc;
        if (!guided && (rc = temporal_frame_guides(c, st))) return rc;
        if ((rc = temporal_device(c, t.desc, res_x, res_y, frame, past, t.M, t.film[nx].get(), t.mom[nx].get(), counts, st)))
            return rc;
        return dd ? denoise_device(c, *dd, res_x, res_y, t.film[nx].get(), t.mom[nx].get(), t.feat[nx].get(),
                                   c->dn.out.get(), nullptr, st)
                  : RT_OK;
    });
    if (rc || (rc = stage_out(c, film_out, dd ? c->dn.out : t.film[nx], n, st))) return rc;
    HIPCHK(c, hipStreamSynchronize(st));
    return RT_OK;
}
}  // namespace

// rt_temporal_frame and rt_temporal_frame_guided (guided; session: its adaptive session's last info, may be null)
static int impl_rt_temporal_frame(rt_ctx* c, const rt_adaptive_desc* ad, const rt_denoise_desc* dd, const float* M,
                                  rt_pixel* film_out, rt_temporal_info* info, bool guided, rt_adaptive_info* session) {
    if (!c) return RT_E_ARG;
    rt_ctx::Temporal& t = c->tp;
    if (!t.live) return fail(c, RT_E_STATE, "no temporal session is open (rt_temporal_begin first)");
    if (!ad || !M || !film_out)
        return fail(c, RT_E_ARG, "temporal frame: the adaptive descriptor, the matrix and film_out are required");
    int rc;
    if (dd) {
        if ((rc = denoise_check_desc(c, dd))) return rc;
        if (dd->feature_samples != t.desc.feature_samples)
            return fail(c, RT_E_ARG, "temporal frame: the filter's feature_samples differs from the session's");
        if (dd->chain_depth != t.desc.chain_depth)
            return fail(c, RT_E_ARG, "temporal frame: the filter's chain_depth differs from the session's");
    }
    if ((rc = check_ready(c))) return rc;
    if (t.desc.feature_samples > dev_sampler(c).spp)
        return fail(c, RT_E_ARG, "temporal: feature_samples exceeds the sampler's samples per pixel");
    if (c->ad.live) adaptive_release(c);  // (only a frame that ended in an exception leaves its session behind)
    if ((rc = impl_rt_adaptive_begin(c, ad, /*frame_owned=*/true))) return rc;
    int counts[T_NCLASSES] = {};
    rt_adaptive_info cur{};
    rc = temporal_frame_body(c, ad, dd, film_out, counts, guided, &cur);
    const std::string msg = c->err;
    impl_rt_adaptive_end(c);
    if (rc) return fail(c, rc, msg);  // the history is as it was: the failed frame is not part of it
    temporal_fill_info(info, t.frames, counts);
    if (session) *session = cur;
    t.cur ^= 1;
    t.frames += 1;
    std::memcpy(t.M, M, sizeof(t.M));
    return RT_OK;
}

static int impl_rt_temporal_reset(rt_ctx* c) {
    if (!c) return RT_E_ARG;
    if (!c->tp.live) return fail(c, RT_E_STATE, "no temporal session is open");
    c->tp.frames = 0;
    return RT_OK;
}

static int impl_rt_temporal_end(rt_ctx* c) {
    if (!c) return RT_E_ARG;
    if (!c->tp.live) return fail(c, RT_E_STATE, "no temporal session is open");
    hipSetDevice(c->device);
    c->tp = rt_ctx::Temporal{};  // (hipFree waits for the work that still uses the buffers)
    return RT_OK;
}

namespace {
int film_resolve(rt_ctx* c, const rt_pixel* film, uint8_t* out, int srgb) {
    if (!c || !film || !out) return RT_E_ARG;
    if (!c->have_film) return fail(c, RT_E_STATE, "film not set");
    hipSetDevice(c->device);
    size_t n = (size_t)c->film.res_x * c->film.res_y;
    DevBuf<float4> df;
    DevBuf<unsigned char> dout;
    HIPCHK(c, df.reserve(n));
    if (dout.reserve(3 * n) != hipSuccess) return fail(c, RT_E_OOM, "resolve buffer");
    const float* const m = c->d_resolve.get();
    if (hipMemcpy(df.get(), film, n * sizeof(float4), hipMemcpyHostToDevice) != hipSuccess ||
        launch_resolve(c->stream, (int)n, df.get(), m, m + 9, dout.get(), srgb) != hipSuccess ||
        hipMemcpyAsync(out, dout.get(), 3 * n, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return fail(c, RT_E_HIP, "resolve failed");
    return RT_OK;
}
}  // namespace

static int get_stats_one(rt_ctx* c, rt_stats* out) {
    if (!c || !out) return RT_E_ARG;
    hipSetDevice(c->device);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipDeviceSynchronize());
    harvest(c);
    std::vector<unsigned long long> raw(kCtrWords);
    HIPCHK(c, hipMemcpy(raw.data(), c->d_ctr.get(), kCtrWords * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    unsigned long long h[C_NCOUNTERS] = {};
    for (int k = 0; k < C_NCOUNTERS; ++k)
        for (int u = 0; u < kCtrSubs; ++u) h[k] += raw[ctr_word(k, u)];
    rt_stats s = c->stats;
    s.nodes_tested = (int64_t)h[C_NODES];
    s.tris_tested = (int64_t)h[C_TRIS];
    s.hits = (int64_t)h[C_HITS];
    s.rays = (int64_t)h[C_RAYS];
    s.shadow_rays = (int64_t)h[C_SHADOW];
    s.shadow_nodes_tested = (int64_t)h[C_SNODES];
    s.shadow_tris_tested = (int64_t)h[C_STRIS];
    s.samples = (int64_t)h[C_SAMPLES];
    s.fallback_rays = (int64_t)h[C_FALLBACK];
    s.shadow_fallback_rays = (int64_t)h[C_SFALLBACK];
    s.nee_vertices = (int64_t)h[C_NEEVTX];
    s.coop_overflows = (int64_t)h[C_COOPOVF];
#if RT_SIMD_STATS
    unsigned long long sm[8];
    simd_stats_read(sm);
    std::fprintf(stderr, "SIMD closest nodes %.3f tris %.3f | any nodes %.3f tris %.3f | steps %llu %llu %llu %llu\n",
                 sm[1] / (double)(sm[0] + !sm[0]), sm[3] / (double)(sm[2] + !sm[2]), sm[5] / (double)(sm[4] + !sm[4]),
                 sm[7] / (double)(sm[6] + !sm[6]), sm[0] / 64, sm[2] / 64, sm[4] / 64, sm[6] / 64);
#endif
    *out = s;
    return RT_OK;
}

static int reset_stats_one(rt_ctx* c) {
    if (!c) return RT_E_ARG;
    hipSetDevice(c->device);
    HIPCHK(c, hipDeviceSynchronize());
    harvest(c);
    c->stats = rt_stats{};
    c->ms_env_miss = 0;
    HIPCHK(c, hipMemset(c->d_ctr.get(), 0, sizeof(unsigned long long) * kCtrWords));
    return RT_OK;
}

static int impl_rt_octree_get_info(rt_ctx* c, rt_octree_info* out) {
    if (!c || !out) return RT_E_ARG;
    if (!c->have_scene) return fail(c, RT_E_STATE, "no scene");
    *out = c->info;
    return RT_OK;
}

static int impl_rt_octree_export(rt_ctx* c, float* bounds, int32_t* child, int32_t* leaf_first, int32_t* leaf_count, int32_t* refs) {
    if (!c) return RT_E_ARG;
    if (!c->have_scene) return fail(c, RT_E_STATE, "no scene");
    if (bounds) std::memcpy(bounds, c->h_bounds.data(), c->h_bounds.size() * 4);
    if (child) std::memcpy(child, c->h_child.data(), c->h_child.size() * 4);
    if (leaf_first) std::memcpy(leaf_first, c->h_leaf_first.data(), c->h_leaf_first.size() * 4);
    if (leaf_count) std::memcpy(leaf_count, c->h_leaf_count.data(), c->h_leaf_count.size() * 4);
    if (refs) std::memcpy(refs, c->h_refs.data(), c->h_refs.size() * 4);
    return RT_OK;
}

// The fast traversal's BVH as uploaded (tile set `set`): counts always, arrays when the pointers are non-null.
static int impl_rt_bvh_export(rt_ctx* c, int set, int* n_nodes, int* n_tiles, float* consts, float* nodes, float* tiles) {
    if (!c || set < 0 || set > 2) return RT_E_ARG;
    if (!c->have_scene) return fail(c, RT_E_STATE, "no scene");
    if (set == 1 && !c->cull) set = 0;  // the kernels use set 0's arrays when there is no culled set
    if (n_nodes) *n_nodes = c->bvh_count[set][0];
    if (n_tiles) *n_tiles = c->bvh_count[set][1];
    if (consts) { consts[0] = c->dsc.wabs; consts[1] = c->dsc.oguard; }
    hipSetDevice(c->device);
    if (nodes && c->bvh_count[set][0])
        HIPCHK(c, hipMemcpy(nodes, c->dsc.bvh[set], (size_t)c->bvh_count[set][0] * kBvhNodeF4 * 16, hipMemcpyDeviceToHost));
    if (tiles && c->bvh_count[set][1]) {  // the device's compact tiles + ids, exported in the 12-float view
        const int nt = c->bvh_count[set][1];
        std::vector<float> t9(9 * (size_t)nt);
        std::vector<int> tid(nt);
        HIPCHK(c, hipMemcpy(t9.data(), c->dsc.btiles[set], t9.size() * 4, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(tid.data(), c->dsc.btid[set], tid.size() * 4, hipMemcpyDeviceToHost));
        bvh_tiles_logical(t9.data(), tid.data(), nt, tiles);
    }
    return RT_OK;
}

// The same BVH built on the host alone (no device): the upload's world transform, tile-set filter, padding and
// build parameters (read_knobs, as rt_create).  For CPU tests of the traversal.
static int impl_rt_debug_bvh_build(const rt_scene_desc* s, int set, int* n_nodes, int* n_tiles, float* consts,
                                   float* nodes, float* tiles) {
    if (!s || set < 0 || set > 2 || !validate_scene(s, /*geometry_only=*/true).empty()) return RT_E_ARG;
    const Knobs kn = read_knobs();
    float cost = kn.bvh_node_cost;
    int leaf = kn.bvh_max_leaf;
    if (set == kBvhAny && kn.bvh_any_cost > 0) {  // (RTMI_BVH_ANY "0/..": the any-hit walks use set 0's closest-hit BVH)
        cost = kn.bvh_any_cost;
        leaf = kn.bvh_any_leaf;
    }
    SceneWorld sw;
    scene_world(s, sw);
    BvhData b;
    float wabs = 0.f, oguard = 0.f;
    scene_bvh(sw, set == 1 && s->cull_backfaces ? 1 : 0, cost, leaf, b, wabs, oguard);
    if (n_nodes) *n_nodes = (int)(b.nodes.size() / kBvhNodeF4);
    if (n_tiles) *n_tiles = (int)b.tid.size();
    if (consts) { consts[0] = wabs; consts[1] = oguard; }
    if (nodes) std::memcpy(nodes, b.nodes.data(), b.nodes.size() * 16);
    if (tiles) bvh_tiles_logical(b.tiles.data(), b.tid.data(), (int)b.tid.size(), tiles);
    return RT_OK;
}

// n rays given as float[3n] origins / directions, on the device as float4[n] each; the direction's w = tmax[i] or 0
static hipError_t upload_rays(int n, const float* ro, const float* rd, const float* tmax, float4* dO, float4* dD) {
    std::vector<float4> o(n), d(n);
    for (int i = 0; i < n; ++i) {
        o[i] = make_float4(ro[3 * i], ro[3 * i + 1], ro[3 * i + 2], 0.f);
        d[i] = make_float4(rd[3 * i], rd[3 * i + 1], rd[3 * i + 2], tmax ? tmax[i] : 0.f);
    }
    hipError_t e = hipMemcpy(dO, o.data(), 16 * (size_t)n, hipMemcpyHostToDevice);
    return e != hipSuccess ? e : hipMemcpy(dD, d.data(), 16 * (size_t)n, hipMemcpyHostToDevice);
}

static int impl_rt_debug_trace(rt_ctx* c, int n, const float* ro, const float* rd, int use_cull, int32_t* prim, float* bt) {
    if (!c || n < 0 || (n && (!ro || !rd || !prim || !bt))) return RT_E_ARG;
    if (!c->have_scene) return fail(c, RT_E_STATE, "no scene");
    if (n == 0) return RT_OK;
    hipSetDevice(c->device);
    // RTMI_DEBUG_PATH_KERNELS (multi-level scenes): the kernel path mode launches — wave tickets, the BVH walk, the
    // cooperative BFS for the undecided rays (or k_trace_fallback without coop_ok) — instead of the per-thread one
    const bool path_kernel = c->knobs.debug_path && c->dsc.qcap != 1;
    int rc = ensure_ring(c, c->ws[0]);
    if (rc) return rc;
    rc = ordered(c, c->stream, [&]() -> int {
        DevBuf<float4> dO, dD, dH;
        DevBuf<int> dP, dT, dF;
        if (dO.reserve(n) || dD.reserve(n) || dH.reserve(n) || dP.reserve(n) ||
            (path_kernel && (dT.reserve(2 * kQStride) || dF.reserve(n))))
            return fail(c, RT_E_OOM, "debug trace buffers");
        TraceIO io{dO.get(), dD.get(), QueueView{nullptr, shard_stride(n, 1), n, 1}, (use_cull && c->cull) ? 1 : 0,
                   dH.get(), dP.get()};
        if (path_kernel) {  // (ticket counter at dT[0], fallback list length at dT[kQStride])
            io.ticket = dT.get();
            io.fb_pos = dF.get();
            io.fb_len = dT.get() + kQStride;
        }
        const DevScene ls = lane_scene(c->dsc, c->ws[0]);
        if ((path_kernel && hipMemsetAsync(dT.get(), 0, 2 * kQStride * sizeof(int), c->stream) != hipSuccess) ||
            upload_rays(n, ro, rd, nullptr, dO.get(), dD.get()) != hipSuccess ||
            launch_trace_closest(c->stream, 0, c->dsc.qcap, ls, io, c->d_ctr.get()) != hipSuccess ||
            (path_kernel && !c->dsc.coop_ok &&
             launch_trace_fallback(c->stream, 64, c->dsc.qcap, ls, io, c->d_ctr.get()) != hipSuccess) ||
            hipStreamSynchronize(c->stream) != hipSuccess ||
            hipMemcpy(prim, dP.get(), 4 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(bt, dH.get(), 16 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(c, RT_E_HIP, std::string("debug trace: ") + hipGetErrorString(hipGetLastError()));
        return RT_OK;
    });
    if (rc) return rc;
    for (int i = 0; i < n; ++i)
        if (prim[i] < 0) bt[4 * i] = bt[4 * i + 1] = bt[4 * i + 2] = bt[4 * i + 3] = 0.f;
    return RT_OK;
}

static int impl_rt_debug_occluded(rt_ctx* c, int n, const float* ro, const float* rd, const float* tmax, int32_t* occluded) {
    if (!c || n < 0 || (n && (!ro || !rd || !tmax || !occluded))) return RT_E_ARG;
    if (!c->have_scene) return fail(c, RT_E_STATE, "no scene");
    if (n == 0) return RT_OK;
    hipSetDevice(c->device);
    int rc = ensure_ring(c, c->ws[0]);
    if (rc) return rc;
    return ordered(c, c->stream, [&]() -> int {
        DevBuf<float4> dO, dD;
        DevBuf<int> dP;
        if (dO.reserve(n) || dD.reserve(n) || dP.reserve(n)) return fail(c, RT_E_OOM, "debug occlusion buffers");
        if (upload_rays(n, ro, rd, tmax, dO.get(), dD.get()) != hipSuccess ||
            launch_occluded(c->stream, c->dsc.qcap, lane_scene(c->dsc, c->ws[0]), n, dO.get(), dD.get(), dP.get(),
                            c->d_ctr.get(), c->knobs.debug_path && c->dsc.coop_ok) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess ||
            hipMemcpy(occluded, dP.get(), 4 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(c, RT_E_HIP, std::string("debug occlusion: ") + hipGetErrorString(hipGetLastError()));
        return RT_OK;
    });
}

// The coherence sorts alone (rt_sort.hip) on a synthetic sharded queue: kShards shards of stride S, shard j holding
// shard_len[j] items at positions [j S, j S + shard_len[j]) with keys[pos] (and, for the NEE sort, slots[pos]).
// which 0: the ray sort (key bits 3 + 2 bits_a + 3 bits_b; out[pos'] = the queue position of sorted item pos'),
// 1: the NEE sort (key bits 3 bits_a; out = the slots sorted in place).  Sorted item k' sits at position
// (k' / S2) S + k' % S2 with S2 = shard_stride(n, kShards); out_len[j] receives the rewritten shard lengths.
static int impl_rt_debug_sort(rt_ctx* c, int which, int S, const int32_t* shard_len, const uint32_t* keys,
                              const int32_t* slots, int bits_a, int bits_b, int32_t* out, int32_t* out_len) {
    if (!c || (which != 0 && which != 1) || S < 64 || S % 64 || !shard_len || !keys || !out || !out_len ||
        (which == 1 && !slots))
        return c ? fail(c, RT_E_ARG, "debug sort: bad arguments") : RT_E_ARG;
    for (int j = 0; j < kShards; ++j)
        if (shard_len[j] < 0 || shard_len[j] > S) return fail(c, RT_E_ARG, "debug sort: shard length out of range");
    const int kb = which == 0 ? 3 + 2 * bits_a + 3 * bits_b : 3 * bits_a;
    if (bits_a < 0 || bits_a > (which == 0 ? 4 : 9) || bits_b < 0 || bits_b > 9 || kb < 1 || kb > 30)
        return fail(c, RT_E_ARG, "debug sort: key bits out of range");
    hipSetDevice(c->device);
    return ordered(c, c->stream, [&]() -> int {
        const size_t cap = (size_t)kShards * S;
        DevBuf<unsigned> dkey, k0, k1;
        DevBuf<int> dslot, dlen, dout, v0, v1;
        DevBuf<unsigned char> temp;
        if (dkey.reserve(cap) || dslot.reserve(cap) || dlen.reserve((size_t)kShards * kQStride) || dout.reserve(cap) ||
            k0.reserve(cap) || k1.reserve(cap) || v0.reserve(cap) || v1.reserve(cap) || temp.reserve(sort_temp_bytes()))
            return fail(c, RT_E_OOM, "debug sort buffers");
        std::vector<int> hlen((size_t)kShards * kQStride, 0);
        for (int j = 0; j < kShards; ++j) hlen[(size_t)j * kQStride] = shard_len[j];
        std::vector<int> hs(cap, -1);
        if (which == 1) std::memcpy(hs.data(), slots, cap * 4);
        hipError_t e = hipMemcpy(dkey.get(), keys, cap * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dslot.get(), hs.data(), cap * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dlen.get(), hlen.data(), hlen.size() * 4, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemset(dout.get(), 0xff, cap * 4);
        if (e == hipSuccess) {
            if (which == 0) {
                SortRaysIO so{dkey.get(), dout.get(), k0.get(), k1.get(), v0.get(), v1.get(), temp.get(), bits_a, bits_b,
                              dlen.get(), S};
                e = launch_sort_rays(c->stream, so);
            } else {
                SortNeeIO so{dslot.get(), dlen.get(), S, dkey.get(), k0.get(), k1.get(), v0.get(), v1.get(), temp.get(),
                             bits_a};
                e = launch_sort_nee(c->stream, so);
            }
        }
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = hipMemcpy(out, which == 0 ? dout.get() : dslot.get(), cap * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(hlen.data(), dlen.get(), hlen.size() * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) return fail(c, RT_E_HIP, std::string("debug sort: ") + hipGetErrorString(e));
        for (int j = 0; j < kShards; ++j) out_len[j] = hlen[(size_t)j * kQStride];
        return RT_OK;
    });
}

static int impl_rt_debug_samples(rt_ctx* c, int n, const int32_t* pixel_ids, const int32_t* indices, rt_sample_record* out) {
    int rc = check_ready(c);
    if (rc) return rc;
    if (n < 0 || (n && (!pixel_ids || !indices || !out))) return fail(c, RT_E_ARG, "bad arguments");
    if (c->integ.kind != RT_INTEGRATOR_REFERENCE) return fail(c, RT_E_ARG, "records are for the reference integrator");
    if (n == 0) return RT_OK;
    int npx = c->film.res_x * c->film.res_y;
    if ((rc = ensure_sobol(c))) return rc;
    DevSampler smp = dev_sampler(c);
    for (int i = 0; i < n; ++i) {
        if (pixel_ids[i] < 0 || pixel_ids[i] >= npx || indices[i] < 0) return fail(c, RT_E_ARG, "sample out of range");
        if (c->smp.kind == RT_SAMPLER_STRATIFIED && !c->smp.jitter && indices[i] >= smp.spp)
            return fail(c, RT_E_ARG, "StratifiedSampler without jitter supports indices < SamplesPerPixel");
    }
    hipSetDevice(c->device);
    Work& w = c->ws[0];
    if ((rc = ensure_workspace(c, w, (size_t)n, false))) return rc;
    return ordered(c, c->stream, [&]() -> int {
        DevBuf<int> dp, di;
        DevBuf<float> dout;
        static_assert(sizeof(rt_sample_record) == 39 * 4, "record layout");
        if (dp.reserve(n) || di.reserve(n) || dout.reserve((size_t)n * 39)) return fail(c, RT_E_OOM, "record buffers");
        hipMemcpy(dp.get(), pixel_ids, 4 * (size_t)n, hipMemcpyHostToDevice);
        hipMemcpy(di.get(), indices, 4 * (size_t)n, hipMemcpyHostToDevice);
        SampleIds ids{nullptr, 1, 0, dp.get(), di.get()};
        const RefIO r = ref_io(c, w.b, n, 1);
        DevFilm fd = dev_film(c);
        RecordIO rio{n, r.go.rayO, r.go.rayD, r.go.lamA, r.go.lamB, r.go.pdfA, r.go.pdfB, r.tio.hitB, r.tio.hitPrim,
                     dout.get(), 39, 1};
        if (launch_generate(c->stream, 0, n, ids, dev_camera(c->cam), smp, fd, r.go) != hipSuccess ||
            launch_trace_closest(c->stream, 0, c->dsc.qcap, lane_scene(c->dsc, w), r.tio, c->d_ctr.get()) != hipSuccess ||
            launch_records(c->stream, c->dsc, c->d_spec.get(), fd, r.sio, rio) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess ||
            hipMemcpy(out, dout.get(), sizeof(rt_sample_record) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(c, RT_E_HIP, std::string("debug samples: ") + hipGetErrorString(hipGetLastError()));
        return RT_OK;
    });
}

// ---- albedo textures --------------------------------------------------------------------------
// the coefficient table on the device, once per context
static int ensure_rgb_table(rt_ctx* c) {
    if (c->tx.table.get()) return RT_OK;
    const float *z, *co;
    if (!rgb_table_host(&z, &co))
        return fail(c, RT_E_STATE, "the RGB -> sigmoid coefficient table is missing (python __graft_entry__.py build)");
    DevBuf<float> t;
    HIPCHK(c, t.reserve(kRgbRes + kRgbTableFloats));
    HIPCHK(c, hipMemcpy(t.get(), z, sizeof(float) * kRgbRes, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(t.get() + kRgbRes, co, sizeof(float) * kRgbTableFloats, hipMemcpyHostToDevice));
    c->tx.table = std::move(t);
    return RT_OK;
}

static int impl_rt_scene_set_textures(rt_ctx* c, const rt_texture_desc* d) {
    if (!c) return RT_E_ARG;
    if (!c->have_scene) return fail(c, RT_E_STATE, "rt_scene_set_textures needs an uploaded scene");
    if (c->ad.live) return fail(c, RT_E_STATE, "rt_scene_set_textures during an adaptive session (rt_adaptive_end first)");
    if (c->tp.live) return fail(c, RT_E_STATE, "rt_scene_set_textures during a temporal session (rt_temporal_end first)");
    if (!c->peers.empty()) return fail(c, RT_E_STATE, "textures support one-device contexts only");
    hipSetDevice(c->device);
    if (!d || d->n_textures == 0) {  // clear: the untextured kernels again
        HIPCHK(c, hipDeviceSynchronize());  // (passes on a caller's stream included)
        free_textures(c);
        return RT_OK;
    }
    if (d->n_textures < 0 || !d->textures || !d->material_texture || !d->tri_texcoords)
        return fail(c, RT_E_ARG, "texture descriptor: NULL array or negative count");
    if (d->n_materials != c->dsc.n_materials || d->n_triangles != c->n_tris)
        return fail(c, RT_E_ARG, "texture descriptor: n_materials / n_triangles differ from the uploaded scene");
    uint64_t total = 0;
    for (int t = 0; t < d->n_textures; ++t) {
        const rt_texture& x = d->textures[t];
        if (x.width < 1 || x.height < 1) return fail(c, RT_E_ARG, "texture width and height must be >= 1");
        if (x.wrap != RT_TEX_CLAMP && x.wrap != RT_TEX_REPEAT) return fail(c, RT_E_ARG, "unknown texture wrap mode");
        if (!x.rgb) return fail(c, RT_E_ARG, "texture without pixels");
        total += (uint64_t)x.width * (uint64_t)x.height;
    }
    for (int m = 0; m < d->n_materials; ++m) {
        const int t = d->material_texture[m];
        if (t < -1 || t >= d->n_textures) return fail(c, RT_E_ARG, "texture id out of range");
        if (t >= 0 && (c->tx.mat_flags[m] & 1)) return fail(c, RT_E_ARG, "a texture cannot be bound to an emissive material");
        if (t >= 0 && (c->tx.mat_flags[m] & 4))
            return fail(c, RT_E_ARG, "a texture cannot be bound to a conductor material (its colour is F(lambda, angle))");
        if (t >= 0 && (c->tx.mat_flags[m] & 8))
            return fail(c, RT_E_ARG, "a texture cannot be bound to a rough dielectric material (it has no albedo)");
        if (t >= 0 && (c->tx.mat_flags[m] & 2))
            return fail(c, RT_E_ARG, "a texture cannot be bound to a material an analytic shape uses");
    }
    // the NEE record's tag holds n_materials + texel index in 31 bits (rt_internal.h NeeIO)
    if ((uint64_t)d->n_materials + total > 0x7fffffffull)
        return fail(c, RT_E_LIMIT, "n_materials plus the textures' texel count exceeds 2^31 - 1");
    int rc;
    if ((rc = ensure_rgb_table(c))) return rc;
    HIPCHK(c, hipDeviceSynchronize());
    free_textures(c);
    rt_ctx::Textures& T = c->tx;
    std::vector<int4> recs(d->n_textures);
    HIPCHK(c, T.texels.reserve((size_t)total));
    T.n_texels = (size_t)total;
    {
        DevBuf<unsigned char> bytes;  // one texture's RGB8 at a time
        size_t base = 0;
        for (int t = 0; t < d->n_textures; ++t) {
            const rt_texture& x = d->textures[t];
            const size_t n = (size_t)x.width * (size_t)x.height;
            recs[t] = make_int4((int)base, x.width, x.height, x.wrap);
            HIPCHK(c, bytes.reserve(3 * n));
            HIPCHK(c, hipMemcpy(bytes.get(), x.rgb, 3 * n, hipMemcpyHostToDevice));
            HIPCHK(c, launch_texture_bake(c->stream, T.table.get(), (int)n, bytes.get(), T.texels.get() + base));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            base += n;
        }
    }
    HIPCHK(c, T.recs.reserve(recs.size()));
    HIPCHK(c, hipMemcpy(T.recs.get(), recs.data(), sizeof(int4) * recs.size(), hipMemcpyHostToDevice));
    HIPCHK(c, T.matTex.reserve((size_t)d->n_materials));
    HIPCHK(c, hipMemcpy(T.matTex.get(), d->material_texture, sizeof(int) * (size_t)d->n_materials, hipMemcpyHostToDevice));
    HIPCHK(c, T.triUV.reserve(3 * (size_t)d->n_triangles));
    HIPCHK(c, hipMemcpy(T.triUV.get(), d->tri_texcoords, sizeof(float2) * 3 * (size_t)d->n_triangles, hipMemcpyHostToDevice));
    const DevTex dt{T.texels.get(), T.recs.get(), T.matTex.get(), T.triUV.get()};
    HIPCHK(c, T.dev.reserve(1));
    HIPCHK(c, hipMemcpy(T.dev.get(), &dt, sizeof(dt), hipMemcpyHostToDevice));
    T.live = true;
    return RT_OK;
}

static int impl_rt_debug_texture_bake(rt_ctx* c, int n, const uint8_t* rgb, float* coeffs) {
    if (!c || n < 0 || (n && (!rgb || !coeffs))) return c ? fail(c, RT_E_ARG, "texture bake: invalid argument") : RT_E_ARG;
    if (n == 0) return RT_OK;
    hipSetDevice(c->device);
    int rc;
    if ((rc = ensure_rgb_table(c))) return rc;
    return ordered(c, c->stream, [&]() -> int {
        DevBuf<unsigned char> bytes;
        DevBuf<float4> out;
        if (bytes.reserve(3 * (size_t)n) || out.reserve(n)) return fail(c, RT_E_OOM, "texture bake buffers");
        std::vector<float4> h(n);
        if (hipMemcpy(bytes.get(), rgb, 3 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
            launch_texture_bake(c->stream, c->tx.table.get(), n, bytes.get(), out.get()) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess ||
            hipMemcpy(h.data(), out.get(), sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(c, RT_E_HIP, std::string("texture bake: ") + hipGetErrorString(hipGetLastError()));
        for (int i = 0; i < n; ++i) { coeffs[3 * i] = h[i].x; coeffs[3 * i + 1] = h[i].y; coeffs[3 * i + 2] = h[i].z; }
        return RT_OK;
    });
}

static int impl_rt_debug_texture_eval(rt_ctx* c, int n, const int32_t* prim, const float* b, int32_t* texel, float* coeffs) {
    if (!c || n < 0 || (n && (!prim || !b || !texel || !coeffs)))
        return c ? fail(c, RT_E_ARG, "texture eval: invalid argument") : RT_E_ARG;
    if (!c->have_scene) return fail(c, RT_E_STATE, "no scene");
    for (int i = 0; i < n; ++i)
        if (prim[i] < 0 || prim[i] >= c->n_tris) return fail(c, RT_E_ARG, "texture eval: triangle id out of range");
    if (n == 0) return RT_OK;
    hipSetDevice(c->device);
    return ordered(c, c->stream, [&]() -> int {
        DevBuf<int> dp, dt;
        DevBuf<float> db;
        DevBuf<float4> dc;
        if (dp.reserve(n) || dt.reserve(n) || db.reserve(3 * (size_t)n) || dc.reserve(n))
            return fail(c, RT_E_OOM, "texture eval buffers");
        std::vector<float4> h(n);
        if (hipMemcpy(dp.get(), prim, 4 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(db.get(), b, 12 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
            launch_texture_eval(c->stream, c->dsc, c->tx.live ? c->tx.dev.get() : nullptr, n, dp.get(), db.get(), dt.get(),
                                dc.get()) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess ||
            hipMemcpy(texel, dt.get(), 4 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(h.data(), dc.get(), sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(c, RT_E_HIP, std::string("texture eval: ") + hipGetErrorString(hipGetLastError()));
        for (int i = 0; i < n; ++i) { coeffs[3 * i] = h[i].x; coeffs[3 * i + 1] = h[i].y; coeffs[3 * i + 2] = h[i].z; }
        return RT_OK;
    });
}

// the device table of one mesh light
static int impl_rt_debug_meshlight_table(rt_ctx* c, int light, int* n, int32_t* tri, float* cdf, float* area) {
    if (!c || !n || !area) return c ? fail(c, RT_E_ARG, "mesh light table: n and area must not be NULL") : RT_E_ARG;
    if (!c->have_scene) return fail(c, RT_E_STATE, "no scene");
    const rt_ctx::MeshLights& M = c->ml;
    if (light < 0 || light >= (int)M.n.size() || M.n[light] <= 0)
        return fail(c, RT_E_ARG, "mesh light table: light " + std::to_string(light) + " is not a mesh light");
    *n = M.n[light];
    *area = M.area[light];
    hipSetDevice(c->device);
    const size_t bytes = 4 * (size_t)M.n[light];
    if ((tri && hipMemcpy(tri, M.tri + M.first[light], bytes, hipMemcpyDeviceToHost) != hipSuccess) ||
        (cdf && hipMemcpy(cdf, M.cdf + M.first[light], bytes, hipMemcpyDeviceToHost) != hipSuccess))
        return fail(c, RT_E_HIP, std::string("mesh light table: ") + hipGetErrorString(hipGetLastError()));
    return RT_OK;
}

// the path kernels' light_ray on explicit shading points and sample points
static int impl_rt_debug_light_sample(rt_ctx* c, int light, int n, const float* po, const float* u, float* wi, float* tmax,
                                      float* dist2, float* nl, int32_t* tri) {
    if (!c || n < 0 || (n && (!po || !u || !wi || !tmax || !dist2 || !nl || !tri)))
        return c ? fail(c, RT_E_ARG, "light sample: invalid argument") : RT_E_ARG;
    if (!c->have_scene) return fail(c, RT_E_STATE, "no scene");
    if (light < 0 || light >= (int)c->h_lights.size())  // (the environment light: rt_debug_env_sample)
        return fail(c, RT_E_ARG, "light sample: light index out of range");
    if (n == 0) return RT_OK;
    hipSetDevice(c->device);
    return ordered(c, c->stream, [&]() -> int {
        DevBuf<float> dp, du;
        DevBuf<float4> da, db;
        DevBuf<int> dt;
        if (dp.reserve(3 * (size_t)n) || du.reserve(2 * (size_t)n) || da.reserve(n) || db.reserve(n) || dt.reserve(n))
            return fail(c, RT_E_OOM, "light sample buffers");
        std::vector<float4> ha(n), hb(n);
        if (hipMemcpy(dp.get(), po, 12 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(du.get(), u, 8 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
            launch_light_sample(c->stream, c->dsc, light, n, dp.get(), du.get(), da.get(), db.get(), dt.get()) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess ||
            hipMemcpy(ha.data(), da.get(), sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(hb.data(), db.get(), sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(tri, dt.get(), 4 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(c, RT_E_HIP, std::string("light sample: ") + hipGetErrorString(hipGetLastError()));
        for (int i = 0; i < n; ++i) {
            wi[3 * i] = ha[i].x; wi[3 * i + 1] = ha[i].y; wi[3 * i + 2] = ha[i].z;
            tmax[i] = ha[i].w;
            dist2[i] = hb[i].x;
            nl[3 * i] = hb[i].y; nl[3 * i + 1] = hb[i].z; nl[3 * i + 2] = hb[i].w;
        }
        return RT_OK;
    });
}

// ---- image environment light ------------------------------------------------------------------
// what needs no device: the descriptor's sizes, pointers, scale and texels
static int environment_check_desc(rt_ctx* c, const rt_environment_desc* d) {
    if (d->width < 1 || d->height < 1) return fail(c, RT_E_ARG, "environment: width and height must be >= 1");
    if (!d->rgb) return fail(c, RT_E_ARG, "environment: NULL rgb");
    if ((uint64_t)d->width * (uint64_t)d->height > (1ull << 24))
        return fail(c, RT_E_LIMIT, "environment: more than 2^24 texels");
    if (!(d->scale >= 0.f) || !std::isfinite(d->scale)) return fail(c, RT_E_ARG, "environment: scale must be finite and >= 0");
    for (int i = 0; i < 9; ++i)
        if (!std::isfinite(d->world_to_env[i])) return fail(c, RT_E_ARG, "environment: world_to_env is not finite");
    const size_t n = 3 * (size_t)d->width * (size_t)d->height;
    for (size_t i = 0; i < n; ++i)
        if (!(d->rgb[i] >= 0.f) || !std::isfinite(d->rgb[i]))
            return fail(c, RT_E_ARG, "environment: texels must be finite and >= 0");
    return RT_OK;
}

// one device of the context: bake and tabulate the map there, then swap it in (a failure leaves the old state)
static int environment_set_one(rt_ctx* c, const rt_environment_desc* d) {
    hipSetDevice(c->device);
    if (!d || d->width == 0) {  // clear: the scene's own lights and kernels again
        HIPCHK(c, hipDeviceSynchronize());  // (passes on a caller's stream included)
        free_environment(c);
        return RT_OK;
    }
    if ((int)c->h_lights.size() + 1 > kMaxLights)
        return fail(c, RT_E_ARG, "environment: the scene's light list is full (at most " + std::to_string(kMaxLights) + " lights)");
    int rc;
    if ((rc = ensure_rgb_table(c))) return rc;
    const int W = d->width, H = d->height;
    const size_t n = (size_t)W * (size_t)H;
    rt_ctx::Environment E;
    DevBuf<float> rgb, wgt, rowsum, total;
    HIPCHK(c, rgb.reserve(3 * n)); HIPCHK(c, wgt.reserve(n)); HIPCHK(c, rowsum.reserve(H)); HIPCHK(c, total.reserve(1));
    HIPCHK(c, E.coef.reserve(n)); HIPCHK(c, E.cond.reserve(n)); HIPCHK(c, E.marg.reserve(H));
    HIPCHK(c, E.lights.reserve(c->h_lights.size() + 1));
    HIPCHK(c, hipMemcpy(rgb.get(), d->rgb, sizeof(float) * 3 * n, hipMemcpyHostToDevice));
    HIPCHK(c, launch_env_bake(c->stream, c->tx.table.get(), W, H, rgb.get(), E.coef.get(), wgt.get()));
    HIPCHK(c, launch_env_table(c->stream, W, H, wgt.get(), E.cond.get(), rowsum.get(), E.marg.get(), total.get()));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(&E.total, total.get(), sizeof(float), hipMemcpyDeviceToHost));
    if (!(E.total > 0.f) || !std::isfinite(E.total))
        return fail(c, RT_E_ARG, "environment: the total of the map's weights is not a positive finite float");
    E.W = W; E.H = H;
    E.dev = DevLight{};
    E.dev.type = kLightEnv;
    E.dev.material = -1;
    E.dev.shape = -1;
    E.dev.scale = d->scale;
    for (int i = 0; i < 9; ++i) E.dev.o2r[i] = d->world_to_env[i];
    env_pack(E.dev, EnvTab{E.coef.get(), E.cond.get(), E.marg.get(), W, H});
    std::vector<DevLight> lights = c->h_lights;
    lights.push_back(E.dev);
    HIPCHK(c, hipMemcpy(E.lights.get(), lights.data(), sizeof(DevLight) * lights.size(), hipMemcpyHostToDevice));
    HIPCHK(c, hipDeviceSynchronize());  // (passes still reading the old list or the old map)
    free_environment(c);
    c->env = std::move(E);
    c->env.live = true;
    c->dsc.lights = c->env.lights.get();
    c->dsc.n_lights = (int)lights.size();
    return RT_OK;
}

static int impl_rt_debug_env_table(rt_ctx* c, int* w, int* h, float* coeffs4, float* cond, float* marg, float* total) {
    if (!c || !w || !h || !total) return c ? fail(c, RT_E_ARG, "environment table: w, h and total must not be NULL") : RT_E_ARG;
    if (!c->env.live) return fail(c, RT_E_STATE, "no environment is bound");
    const rt_ctx::Environment& E = c->env;
    *w = E.W; *h = E.H; *total = E.total;
    hipSetDevice(c->device);
    const size_t n = (size_t)E.W * (size_t)E.H;
    if ((coeffs4 && hipMemcpy(coeffs4, E.coef.get(), sizeof(float4) * n, hipMemcpyDeviceToHost) != hipSuccess) ||
        (cond && hipMemcpy(cond, E.cond.get(), sizeof(float) * n, hipMemcpyDeviceToHost) != hipSuccess) ||
        (marg && hipMemcpy(marg, E.marg.get(), sizeof(float) * (size_t)E.H, hipMemcpyDeviceToHost) != hipSuccess))
        return fail(c, RT_E_HIP, std::string("environment table: ") + hipGetErrorString(hipGetLastError()));
    return RT_OK;
}

static int impl_rt_debug_env_sample(rt_ctx* c, int n, const float* u, float* wi, float* pdf, int32_t* texel) {
    if (!c || n < 0 || (n && (!u || !wi || !pdf || !texel)))
        return c ? fail(c, RT_E_ARG, "environment sample: invalid argument") : RT_E_ARG;
    if (!c->env.live) return fail(c, RT_E_STATE, "no environment is bound");
    if (n == 0) return RT_OK;
    hipSetDevice(c->device);
    return ordered(c, c->stream, [&]() -> int {
        DevBuf<float> du;
        DevBuf<float4> dw;
        DevBuf<int> dt;
        if (du.reserve(2 * (size_t)n) || dw.reserve(n) || dt.reserve(n)) return fail(c, RT_E_OOM, "environment sample buffers");
        std::vector<float4> hw(n);
        if (hipMemcpy(du.get(), u, 8 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
            launch_env_sample(c->stream, c->env.dev, n, du.get(), dw.get(), dt.get()) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess ||
            hipMemcpy(hw.data(), dw.get(), sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(texel, dt.get(), 4 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(c, RT_E_HIP, std::string("environment sample: ") + hipGetErrorString(hipGetLastError()));
        for (int i = 0; i < n; ++i) {
            wi[3 * i] = hw[i].x; wi[3 * i + 1] = hw[i].y; wi[3 * i + 2] = hw[i].z;
            pdf[i] = hw[i].w;
        }
        return RT_OK;
    });
}

static int impl_rt_debug_env_eval(rt_ctx* c, int n, const float* dir, int32_t* texel, float* pdf) {
    if (!c || n < 0 || (n && (!dir || !texel || !pdf)))
        return c ? fail(c, RT_E_ARG, "environment eval: invalid argument") : RT_E_ARG;
    if (!c->env.live) return fail(c, RT_E_STATE, "no environment is bound");
    if (n == 0) return RT_OK;
    hipSetDevice(c->device);
    return ordered(c, c->stream, [&]() -> int {
        DevBuf<float> dd, dp;
        DevBuf<int> dt;
        if (dd.reserve(3 * (size_t)n) || dp.reserve(n) || dt.reserve(n)) return fail(c, RT_E_OOM, "environment eval buffers");
        if (hipMemcpy(dd.get(), dir, 12 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
            launch_env_eval(c->stream, c->env.dev, n, dd.get(), dt.get(), dp.get()) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess ||
            hipMemcpy(texel, dt.get(), 4 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(pdf, dp.get(), 4 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(c, RT_E_HIP, std::string("environment eval: ") + hipGetErrorString(hipGetLastError()));
        return RT_OK;
    });
}

// the miss stage's HIP-event time since the last rt_reset_stats (also part of rt_stats.ms_shade)
static int impl_rt_debug_env_stats(rt_ctx* c, double* ms_miss, int64_t* launches) {
    if (!c || !ms_miss) return c ? fail(c, RT_E_ARG, "environment stats: NULL") : RT_E_ARG;
    hipSetDevice(c->device);
    HIPCHK(c, hipDeviceSynchronize());
    harvest(c);
    *ms_miss = c->ms_env_miss;
    if (launches) {
        long long n[6];
        tabled_launch_counts(n);
        for (int i = 0; i < 6; ++i) launches[i] = n[i];
    }
    return RT_OK;
}

// ---- rough reflector: the shade kernel's GGX device functions on explicit inputs
static int impl_rt_debug_ggx_sample(rt_ctx* c, float alpha, int n, const float* normal, const float* dir, const float* u,
                                    float* disk_out, float* wi, float* wb, float* pdf) {
    if (!c || n < 0 || !ggx_alpha_ok(alpha) || (n && (!normal || !dir || !u || !disk_out || !wi || !wb || !pdf)))
        return c ? fail(c, RT_E_ARG, "ggx sample: invalid argument") : RT_E_ARG;
    if (n == 0) return RT_OK;
    hipSetDevice(c->device);
    return ordered(c, c->stream, [&]() -> int {
        DevBuf<float> dn, dd, du;
        DevBuf<float2> dk, dp;
        DevBuf<float4> dw;
        if (dn.reserve(3 * (size_t)n) || dd.reserve(3 * (size_t)n) || du.reserve(2 * (size_t)n) || dk.reserve(n) ||
            dp.reserve(n) || dw.reserve(n))
            return fail(c, RT_E_OOM, "ggx sample buffers");
        std::vector<float4> hw(n);
        std::vector<float2> hp(n);
        if (hipMemcpy(dn.get(), normal, 12 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(dd.get(), dir, 12 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(du.get(), u, 8 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
            launch_ggx_sample(c->stream, alpha, n, dn.get(), dd.get(), du.get(), dk.get(), dw.get(), dp.get()) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess ||
            hipMemcpy(disk_out, dk.get(), 8 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(hw.data(), dw.get(), sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(hp.data(), dp.get(), sizeof(float2) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(c, RT_E_HIP, std::string("ggx sample: ") + hipGetErrorString(hipGetLastError()));
        for (int i = 0; i < n; ++i) {
            wi[3 * i] = hw[i].x; wi[3 * i + 1] = hw[i].y; wi[3 * i + 2] = hw[i].z;
            wb[i] = hp[i].x; pdf[i] = hp[i].y;
        }
        return RT_OK;
    });
}

static int impl_rt_debug_ggx_eval(rt_ctx* c, float alpha, int n, const float* normal, const float* dir, const float* wi,
                                  float* fcos, float* pdf) {
    if (!c || n < 0 || !ggx_alpha_ok(alpha) || (n && (!normal || !dir || !wi || !fcos || !pdf)))
        return c ? fail(c, RT_E_ARG, "ggx eval: invalid argument") : RT_E_ARG;
    if (n == 0) return RT_OK;
    hipSetDevice(c->device);
    return ordered(c, c->stream, [&]() -> int {
        DevBuf<float> dn, dd, dw;
        DevBuf<float2> dp;
        if (dn.reserve(3 * (size_t)n) || dd.reserve(3 * (size_t)n) || dw.reserve(3 * (size_t)n) || dp.reserve(n))
            return fail(c, RT_E_OOM, "ggx eval buffers");
        std::vector<float2> hp(n);
        if (hipMemcpy(dn.get(), normal, 12 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(dd.get(), dir, 12 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(dw.get(), wi, 12 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
            launch_ggx_eval(c->stream, alpha, n, dn.get(), dd.get(), dw.get(), dp.get()) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess ||
            hipMemcpy(hp.data(), dp.get(), sizeof(float2) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(c, RT_E_HIP, std::string("ggx eval: ") + hipGetErrorString(hipGetLastError()));
        for (int i = 0; i < n; ++i) { fcos[i] = hp[i].x; pdf[i] = hp[i].y; }
        return RT_OK;
    });
}

// launches of the RGH instantiations by the context's last path pass (render_path counts them)
static int impl_rt_debug_rough_stats(rt_ctx* c, int64_t* launches) {
    if (!c || !launches) return c ? fail(c, RT_E_ARG, "rough stats: NULL") : RT_E_ARG;
    launches[0] = c->rgh_launches[0];
    launches[1] = c->rgh_launches[1];
    return RT_OK;
}

// ---- rough glass: the level-3 kernels' device functions at a rough-glass vertex, on explicit inputs
static bool roughglass_er_ok(float er) { return er > 0.f && er < 3.0e38f; }
static int impl_rt_debug_roughglass_sample(rt_ctx* c, float alpha, float er, int n, const float* normal, const float* dir,
                                           const float* u, float* disk_out, float* wi, float* w, float* pdf, int32_t* branch) {
    if (!c || n < 0 || !ggx_alpha_ok(alpha) || !roughglass_er_ok(er) ||
        (n && (!normal || !dir || !u || !disk_out || !wi || !w || !pdf || !branch)))
        return c ? fail(c, RT_E_ARG, "roughglass sample: invalid argument") : RT_E_ARG;
    if (n == 0) return RT_OK;
    hipSetDevice(c->device);
    return ordered(c, c->stream, [&]() -> int {
        DevBuf<float> dn, dd, du;
        DevBuf<float2> dk, dp;
        DevBuf<float4> dw;
        if (dn.reserve(3 * (size_t)n) || dd.reserve(3 * (size_t)n) || du.reserve(3 * (size_t)n) || dk.reserve(n) ||
            dp.reserve(n) || dw.reserve(n))
            return fail(c, RT_E_OOM, "roughglass sample buffers");
        std::vector<float4> hw(n);
        std::vector<float2> hp(n);
        if (hipMemcpy(dn.get(), normal, 12 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(dd.get(), dir, 12 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(du.get(), u, 12 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
            launch_roughglass_sample(c->stream, alpha, er, n, dn.get(), dd.get(), du.get(), dk.get(), dw.get(), dp.get()) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess ||
            hipMemcpy(disk_out, dk.get(), 8 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(hw.data(), dw.get(), sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(hp.data(), dp.get(), sizeof(float2) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(c, RT_E_HIP, std::string("roughglass sample: ") + hipGetErrorString(hipGetLastError()));
        for (int i = 0; i < n; ++i) {
            wi[3 * i] = hw[i].x; wi[3 * i + 1] = hw[i].y; wi[3 * i + 2] = hw[i].z;
            branch[i] = (int32_t)hw[i].w;
            w[i] = hp[i].x; pdf[i] = hp[i].y;
        }
        return RT_OK;
    });
}

static int impl_rt_debug_roughglass_eval(rt_ctx* c, float alpha, float er, int n, const float* normal, const float* dir,
                                         const float* wi, float* fcos, float* pdf) {
    if (!c || n < 0 || !ggx_alpha_ok(alpha) || !roughglass_er_ok(er) || (n && (!normal || !dir || !wi || !fcos || !pdf)))
        return c ? fail(c, RT_E_ARG, "roughglass eval: invalid argument") : RT_E_ARG;
    if (n == 0) return RT_OK;
    hipSetDevice(c->device);
    return ordered(c, c->stream, [&]() -> int {
        DevBuf<float> dn, dd, dw;
        DevBuf<float2> dp;
        if (dn.reserve(3 * (size_t)n) || dd.reserve(3 * (size_t)n) || dw.reserve(3 * (size_t)n) || dp.reserve(n))
            return fail(c, RT_E_OOM, "roughglass eval buffers");
        std::vector<float2> hp(n);
        if (hipMemcpy(dn.get(), normal, 12 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(dd.get(), dir, 12 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(dw.get(), wi, 12 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
            launch_roughglass_eval(c->stream, alpha, er, n, dn.get(), dd.get(), dw.get(), dp.get()) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess ||
            hipMemcpy(hp.data(), dp.get(), sizeof(float2) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(c, RT_E_HIP, std::string("roughglass eval: ") + hipGetErrorString(hipGetLastError()));
        for (int i = 0; i < n; ++i) { fcos[i] = hp[i].x; pdf[i] = hp[i].y; }
        return RT_OK;
    });
}

// launches of the level-3 instantiations by the context's last path pass (render_path counts them)
static int impl_rt_debug_roughglass_stats(rt_ctx* c, int64_t* launches) {
    if (!c || !launches) return c ? fail(c, RT_E_ARG, "roughglass stats: NULL") : RT_E_ARG;
    launches[0] = c->rgl_launches[0];
    launches[1] = c->rgl_launches[1];
    return RT_OK;
}

// ---- absorbing media
static int impl_rt_scene_set_media(rt_ctx* c, const rt_medium* media, int n) {
    if (!c) return RT_E_ARG;
    if (!c->have_scene) return fail(c, RT_E_STATE, "rt_scene_set_media needs an uploaded scene");
    if (c->ad.live) return fail(c, RT_E_STATE, "rt_scene_set_media during an adaptive session (rt_adaptive_end first)");
    if (c->tp.live) return fail(c, RT_E_STATE, "rt_scene_set_media during a temporal session (rt_temporal_end first)");
    if (!c->peers.empty()) return fail(c, RT_E_STATE, "media support one-device contexts only");
    hipSetDevice(c->device);
    if (!media || n == 0) {  // clear: no absorb stage again
        HIPCHK(c, hipDeviceSynchronize());  // (passes on a caller's stream included)
        free_media(c);
        return RT_OK;
    }
    if (n != c->dsc.n_materials || (size_t)n != c->med.mat_type.size())
        return fail(c, RT_E_ARG, "media: n_materials differs from the uploaded scene's");
    bool any = false;
    for (int m = 0; m < n; ++m) {
        const rt_medium& x = media[m];
        const std::string at = "media: material " + std::to_string(m) + ": ";
        if (!(x.sigma >= 0.f && x.sigma < std::numeric_limits<float>::infinity()))
            return fail(c, RT_E_ARG, at + "sigma must be finite and >= 0");
        if (!(x.sigma > 0.f)) continue;
        for (int k = 0; k < 3; ++k)
            if (!std::isfinite(x.sigmoid[k]))
                return fail(c, RT_E_ARG, at + "sigmoid[" + std::to_string(k) + "] must be finite when sigma > 0");
        if (c->med.mat_emits[m]) return fail(c, RT_E_ARG, at + "sigma > 0 on an emissive material");
        if (c->med.mat_type[m] != RT_MAT_DIELECTRIC && c->med.mat_type[m] != RT_MAT_ROUGH_DIELECTRIC)
            return fail(c, RT_E_ARG, at + "sigma > 0 on a material whose type is neither RT_MAT_DIELECTRIC nor "
                                          "RT_MAT_ROUGH_DIELECTRIC");
        any = true;
    }
    std::vector<float4> h((size_t)n);
    for (int m = 0; m < n; ++m) h[m] = make_float4(media[m].sigmoid[0], media[m].sigmoid[1], media[m].sigmoid[2], media[m].sigma);
    HIPCHK(c, hipDeviceSynchronize());
    DevBuf<float4> t;  // (a failure below leaves the media bound before in place)
    HIPCHK(c, t.reserve((size_t)n));
    HIPCHK(c, hipMemcpy(t.get(), h.data(), sizeof(float4) * (size_t)n, hipMemcpyHostToDevice));
    c->med.table = std::move(t);
    c->med.bound.assign(media, media + n);
    c->med.live = any;
    return RT_OK;
}

static bool medium_items_ok(const rt_medium* m, int n, const float* lambda, const float* len, const float* out) {
    return n >= 0 && (n == 0 || (m && lambda && len && out));
}
static int impl_rt_debug_medium_eval(rt_ctx* c, const rt_medium* m, int n, const float* lambda, const float* len, float* out) {
    if (!c || !medium_items_ok(m, n, lambda, len, out)) return c ? fail(c, RT_E_ARG, "medium eval: invalid argument") : RT_E_ARG;
    if (n == 0) return RT_OK;
    hipSetDevice(c->device);
    return ordered(c, c->stream, [&]() -> int {
        DevBuf<float4> dm;
        DevBuf<float> dl, dn, dout;
        if (dm.reserve(n) || dl.reserve(8 * (size_t)n) || dn.reserve(n) || dout.reserve(8 * (size_t)n))
            return fail(c, RT_E_OOM, "medium eval buffers");
        std::vector<float4> hm(n);
        for (int i = 0; i < n; ++i) hm[i] = make_float4(m[i].sigmoid[0], m[i].sigmoid[1], m[i].sigmoid[2], m[i].sigma);
        if (hipMemcpy(dm.get(), hm.data(), sizeof(float4) * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(dl.get(), lambda, 32 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(dn.get(), len, 4 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
            launch_medium_eval(c->stream, n, dm.get(), dl.get(), dn.get(), dout.get()) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess ||
            hipMemcpy(out, dout.get(), 32 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(c, RT_E_HIP, std::string("medium eval: ") + hipGetErrorString(hipGetLastError()));
        return RT_OK;
    });
}

// launches of k_medium_absorb and the segments it attenuated in the context's last path pass (render_path zeroes both)
static int impl_rt_debug_medium_stats(rt_ctx* c, int* launches, unsigned long long* segments) {
    if (!c || !launches || !segments) return c ? fail(c, RT_E_ARG, "medium stats: NULL") : RT_E_ARG;
    *launches = c->med.launches;
    *segments = 0;
    if (!c->med.counted || !c->med.ctr.get()) return RT_OK;
    hipSetDevice(c->device);
    HIPCHK(c, hipDeviceSynchronize());  // (passes on a caller's stream included)
    std::vector<unsigned long long> raw(kMediumCtrWords);
    HIPCHK(c, hipMemcpy(raw.data(), c->med.ctr.get(), kMediumCtrWords * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int u = 0; u < kCtrSubs; ++u) *segments += raw[ctr_word(0, u)];
    return RT_OK;
}

// ---- metal: the level-2 kernels' device functions for a light's wi, on explicit inputs
static int impl_rt_debug_conductor_eval(rt_ctx* c, int metal, float alpha, int n, const float* normal, const float* dir,
                                        const float* wi, const float* lambda, float* fcos, float* pdf, float* F) {
    if (!c || n < 0 || metal < 0 || metal >= kMetals || !ggx_alpha_ok(alpha) ||
        (n && (!normal || !dir || !wi || !lambda || !fcos || !pdf || !F)))
        return c ? fail(c, RT_E_ARG, "conductor eval: invalid argument") : RT_E_ARG;
    if (n == 0) return RT_OK;
    hipSetDevice(c->device);
    return ordered(c, c->stream, [&]() -> int {
        DevBuf<float> dn, dd, dw, dl;
        DevBuf<float4> dp;
        if (dn.reserve(3 * (size_t)n) || dd.reserve(3 * (size_t)n) || dw.reserve(3 * (size_t)n) || dl.reserve(n) ||
            dp.reserve(n))
            return fail(c, RT_E_OOM, "conductor eval buffers");
        std::vector<float4> hp(n);
        if (hipMemcpy(dn.get(), normal, 12 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(dd.get(), dir, 12 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(dw.get(), wi, 12 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(dl.get(), lambda, 4 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
            launch_conductor_eval(c->stream, c->d_spec.get(), metal, alpha, n, dn.get(), dd.get(), dw.get(), dl.get(),
                                  dp.get()) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess ||
            hipMemcpy(hp.data(), dp.get(), sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(c, RT_E_HIP, std::string("conductor eval: ") + hipGetErrorString(hipGetLastError()));
        for (int i = 0; i < n; ++i) { fcos[i] = hp[i].x; pdf[i] = hp[i].y; F[i] = hp[i].z; }
        return RT_OK;
    });
}

// launches of the level-2 instantiations by the context's last path pass (render_path counts them)
static int impl_rt_debug_conductor_stats(rt_ctx* c, int64_t* launches) {
    if (!c || !launches) return c ? fail(c, RT_E_ARG, "conductor stats: NULL") : RT_E_ARG;
    launches[0] = c->cnd_launches[0];
    launches[1] = c->cnd_launches[1];
    return RT_OK;
}

// the albedo bake kernel alone, on explicit coefficients under the current sensor
static int impl_rt_debug_albedo_bake(rt_ctx* c, int n, const float* coeffs, float* rgb) {
    if (!c || n < 0 || (n && (!coeffs || !rgb))) return c ? fail(c, RT_E_ARG, "albedo bake: invalid argument") : RT_E_ARG;
    if (n == 0) return RT_OK;
    hipSetDevice(c->device);
    return ordered(c, c->stream, [&]() -> int {
        DevBuf<float4> in, out;
        if (in.reserve(n) || out.reserve(n)) return fail(c, RT_E_OOM, "albedo bake buffers");
        std::vector<float4> h(n);
        for (int i = 0; i < n; ++i) h[i] = make_float4(coeffs[3 * i], coeffs[3 * i + 1], coeffs[3 * i + 2], 0.f);
        if (hipMemcpy(in.get(), h.data(), sizeof(float4) * (size_t)n, hipMemcpyHostToDevice) != hipSuccess ||
            launch_albedo_bake(c->stream, c->d_spec.get(), 0, nullptr, n, in.get(), out.get()) != hipSuccess ||
            hipStreamSynchronize(c->stream) != hipSuccess ||
            hipMemcpy(h.data(), out.get(), sizeof(float4) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(c, RT_E_HIP, std::string("albedo bake: ") + hipGetErrorString(hipGetLastError()));
        for (int i = 0; i < n; ++i) { rgb[3 * i] = h[i].x; rgb[3 * i + 1] = h[i].y; rgb[3 * i + 2] = h[i].z; }
        return RT_OK;
    });
}

// ---- multi-device wrappers: configuration goes to every device of the context -------------------------------
extern "C++" template <class F>
static int on_all(rt_ctx* c, F f) {
    int rc = f(c);
    for (size_t j = 0; !rc && j < c->peers.size(); ++j) {
        rt_ctx* p = c->peers[j];
        hipSetDevice(p->device);
        if ((rc = f(p))) fail(c, rc, "device " + std::to_string(p->device) + ": " + p->err);
    }
    hipSetDevice(c->device);
    return rc;
}

static int impl_rt_create(const rt_options* opt, rt_ctx** out) {
    if (!out) return RT_E_ARG;
    *out = nullptr;
    int nd = opt ? opt->n_devices : 0;
    if (nd <= 1) return create_one(opt, out);
    if (nd > RT_MAX_DEVICES) return RT_E_ARG;
    rt_options o = *opt;
    o.n_devices = 0;
    o.device = opt->devices[0];
    rt_ctx* c = nullptr;
    int rc = create_one(&o, &c);
    if (rc) return rc;
    for (int j = 1; j < nd; ++j) {
        rt_ctx* p = nullptr;
        o.device = opt->devices[j];
        if ((rc = create_one(&o, &p))) { rt_destroy(c); return rc; }
        c->peers.push_back(p);
        c->links.emplace_back();
        if (p->device != c->device) {  // direct xGMI peer copies both ways where the platform allows them
            int ok = 0;
            if (hipDeviceCanAccessPeer(&ok, c->device, p->device) == hipSuccess && ok) {
                hipSetDevice(c->device);
                if (hipDeviceEnablePeerAccess(p->device, 0) != hipSuccess) (void)hipGetLastError();
                hipSetDevice(p->device);
                if (hipDeviceEnablePeerAccess(c->device, 0) != hipSuccess) (void)hipGetLastError();
            }
        }
        hipSetDevice(p->device);
        if (hipEventCreateWithFlags(&p->gathered, hipEventDisableTiming) != hipSuccess) { rt_destroy(c); return RT_E_HIP; }
    }
    hipSetDevice(c->device);
    if (hipEventCreateWithFlags(&c->gathered, hipEventDisableTiming) != hipSuccess) { rt_destroy(c); return RT_E_HIP; }
    if ((rc = rt_set_shard(c, 32, 1, 0))) { rt_destroy(c); return rc; }
    *out = c;
    return RT_OK;
}

static void impl_rt_destroy(rt_ctx* c) {
    if (!c) return;
    for (rt_ctx* p : c->peers) destroy_one(p);  // (each on its own device; its exchange buffer with it)
    destroy_one(c);                             // the peer links' buffers live on c's device
}

static int impl_rt_scene_upload(rt_ctx* c, const rt_scene_desc* s) {
    if (!c) return RT_E_ARG;
    return on_all(c, [&](rt_ctx* x) { return scene_upload_one(x, s); });
}
static int impl_rt_scene_set_environment(rt_ctx* c, const rt_environment_desc* d) {
    if (!c) return RT_E_ARG;
    if (!c->have_scene) return fail(c, RT_E_STATE, "rt_scene_set_environment needs an uploaded scene");
    if (c->ad.live) return fail(c, RT_E_STATE, "rt_scene_set_environment during an adaptive session (rt_adaptive_end first)");
    if (c->tp.live) return fail(c, RT_E_STATE, "rt_scene_set_environment during a temporal session (rt_temporal_end first)");
    if (d && d->width != 0)
        if (int rc = environment_check_desc(c, d)) return rc;
    // every device first bakes into buffers of its own: a device that refuses leaves the others' bound map for the
    // caller to clear or replace (the first device's refusal, the usual one, changes nothing anywhere)
    return on_all(c, [&](rt_ctx* x) { return environment_set_one(x, d); });
}

static int impl_rt_camera_set(rt_ctx* c, const rt_camera_desc* d) {
    if (!c) return RT_E_ARG;
    return on_all(c, [&](rt_ctx* x) { return camera_set_one(x, d); });
}
static int impl_rt_sampler_set(rt_ctx* c, const rt_sampler_desc* d) {
    if (!c) return RT_E_ARG;
    return on_all(c, [&](rt_ctx* x) { return sampler_set_one(x, d); });
}
static int impl_rt_film_set(rt_ctx* c, const rt_film_desc* d) {
    if (!c) return RT_E_ARG;
    return on_all(c, [&](rt_ctx* x) { return film_set_one(x, d); });
}
static int impl_rt_integrator_set(rt_ctx* c, const rt_integrator_desc* d) {
    if (!c) return RT_E_ARG;
    return on_all(c, [&](rt_ctx* x) { return integrator_set_one(x, d); });
}
static int impl_rt_reset_stats(rt_ctx* c) {
    if (!c) return RT_E_ARG;
    return on_all(c, [&](rt_ctx* x) { return reset_stats_one(x); });
}
// the caller's shard (tile t, t % n_shards == shard_id) is split over the context's D devices: device k takes the
// tiles with (t / n_shards) % D == k, i.e. shard (n_shards·D, shard_id + n_shards·k) of the frame
// counters and kernel times summed over the context's devices
static int impl_rt_get_stats(rt_ctx* c, rt_stats* out) {
    if (!c || !out) return RT_E_ARG;
    rt_stats sum{};
    int rc = on_all(c, [&](rt_ctx* x) -> int {
        rt_stats s{};
        int r = get_stats_one(x, &s);
        if (r) return r;
        sum.samples += s.samples; sum.rays += s.rays; sum.shadow_rays += s.shadow_rays;
        sum.nodes_tested += s.nodes_tested; sum.tris_tested += s.tris_tested; sum.hits += s.hits;
        sum.shadow_nodes_tested += s.shadow_nodes_tested; sum.shadow_tris_tested += s.shadow_tris_tested;
        sum.ms_generate += s.ms_generate; sum.ms_trace += s.ms_trace; sum.ms_shade += s.ms_shade;
        sum.ms_shadow += s.ms_shadow; sum.ms_film += s.ms_film; sum.ms_sort += s.ms_sort;
        sum.launches_trace += s.launches_trace; sum.launches_shade += s.launches_shade;
        sum.fallback_rays += s.fallback_rays; sum.shadow_fallback_rays += s.shadow_fallback_rays;
        sum.nee_vertices += s.nee_vertices;
        sum.coop_overflows += s.coop_overflows;
        return RT_OK;
    });
    if (!rc) *out = sum;
    return rc;
}

static int impl_rt_set_shard(rt_ctx* c, int tile_size, int n_shards, int shard_id) {
    if (!c || n_shards <= 0 || shard_id < 0 || shard_id >= n_shards)
        return c ? fail(c, RT_E_ARG, "invalid shard") : RT_E_ARG;
    const int D = 1 + (int)c->peers.size();
    int rc = set_shard_one(c, tile_size, n_shards * D, shard_id);
    for (size_t j = 0; !rc && j < c->peers.size(); ++j)
        if ((rc = set_shard_one(c->peers[j], tile_size, n_shards * D, shard_id + n_shards * (int)(j + 1))))
            fail(c, rc, c->peers[j]->err);
    return rc;
}

}  // extern "C"

// ---- the exception firewall around every entry point (rt_guard.h)
namespace {
// an entry point with a context: impl(c, args...) inside the firewall, an exception's message to rt_last_error
template <class Impl, class... Args>
int entry(rt_ctx* c, Impl impl, Args... args) {
    return guarded([&] { return impl(c, args...); }, [&](const std::string& m) { set_error(c, m); });
}
}  // namespace

extern "C" {
int rt_film_matrices(rt_ctx* c, float* xyz_from_sensor9, float* rgb_from_xyz9) {
    return entry(c, impl_rt_film_matrices, xyz_from_sensor9, rgb_from_xyz9);
}
int rt_render_pass_device(rt_ctx* c, int ib, int ie, void* d_film, void* stream) {
    return entry(c, impl_rt_render_pass_device, ib, ie, d_film, stream);
}
int rt_render_pass(rt_ctx* c, int ib, int ie, rt_pixel* film) { return entry(c, impl_rt_render_pass, ib, ie, film); }
int rt_adaptive_begin(rt_ctx* c, const rt_adaptive_desc* d) { return entry(c, impl_rt_adaptive_begin, d, false); }
int rt_adaptive_step(rt_ctx* c, rt_adaptive_info* info) { return entry(c, impl_rt_adaptive_step, info); }
int rt_adaptive_read(rt_ctx* c, rt_pixel* film, rt_moment* mom, float* block_error, int32_t* active, int* n_active) {
    return entry(c, impl_rt_adaptive_read, film, mom, block_error, active, n_active);
}
int rt_adaptive_end(rt_ctx* c) { return entry(c, impl_rt_adaptive_end); }
int rt_render_adaptive(rt_ctx* c, const rt_adaptive_desc* d, rt_pixel* film, rt_moment* mom, rt_adaptive_info* info) {
    return entry(c, impl_rt_render_adaptive, d, film, mom, info);
}
int rt_debug_adaptive_select(rt_ctx* c, const rt_adaptive_desc* d, const rt_pixel* film, const rt_moment* mom,
                             float* block_error, int32_t* active, int* n_active) {
    return entry(c, impl_rt_debug_adaptive_select, d, film, mom, block_error, active, n_active);
}
int rt_render_features(rt_ctx* c, int ib, int ie, rt_feature* feat) {
    return entry(c, impl_rt_render_features, ib, ie, feat, nullptr, false, 0, nullptr, false);
}
int rt_denoise(rt_ctx* c, const rt_denoise_desc* d, int res_x, int res_y, const rt_pixel* film, const rt_moment* mom,
               const rt_feature* feat, rt_pixel* out, float* variance_out) {
    return entry(c, impl_rt_denoise, d, res_x, res_y, film, mom, feat, out, variance_out, nullptr, false, 0.f);
}
int rt_denoise_albedo(rt_ctx* c, const rt_denoise_desc* d, float albedo_floor, int res_x, int res_y, const rt_pixel* film,
                      const rt_moment* mom, const rt_feature* feat, const rt_albedo* albedo, rt_pixel* out,
                      float* variance_out) {
    return entry(c, impl_rt_denoise, d, res_x, res_y, film, mom, feat, out, variance_out, albedo, true, albedo_floor);
}
int rt_adaptive_denoise(rt_ctx* c, const rt_denoise_desc* d, rt_pixel* film_out) {
    return entry(c, impl_rt_adaptive_denoise, d, film_out, false, 0.f);
}
int rt_adaptive_denoise_albedo(rt_ctx* c, const rt_denoise_desc* d, float albedo_floor, rt_pixel* film_out) {
    return entry(c, impl_rt_adaptive_denoise, d, film_out, true, albedo_floor);
}
int rt_render_features_chain(rt_ctx* c, int ib, int ie, int chain_depth, rt_feature* feat, rt_position* pos) {
    return entry(c, impl_rt_render_features, ib, ie, feat, pos, pos != nullptr, chain_depth, nullptr, false);
}
int rt_render_features_albedo(rt_ctx* c, int ib, int ie, int chain_depth, rt_feature* feat, rt_position* pos,
                              rt_albedo* albedo) {
    return entry(c, impl_rt_render_features, ib, ie, feat, pos, pos != nullptr, chain_depth, albedo, true);
}
int rt_render_features_pos(rt_ctx* c, int ib, int ie, rt_feature* feat, rt_position* pos) {
    return entry(c, impl_rt_render_features, ib, ie, feat, pos, true, 0, nullptr, false);
}
int rt_temporal_accumulate(rt_ctx* c, const rt_temporal_desc* d, int res_x, int res_y, const rt_pixel* film,
                           const rt_moment* mom, const rt_feature* feat, const rt_position* pos, const rt_pixel* hist_film,
                           const rt_moment* hist_mom, const rt_feature* hist_feat, const rt_position* hist_pos,
                           const float* world_to_film_prev, rt_pixel* out_film, rt_moment* out_mom, rt_temporal_info* info) {
    return entry(c, impl_rt_temporal_accumulate, d, res_x, res_y, film, mom, feat, pos, hist_film, hist_mom, hist_feat,
                 hist_pos, world_to_film_prev, out_film, out_mom, info);
}
int rt_temporal_begin(rt_ctx* c, const rt_temporal_desc* d) { return entry(c, impl_rt_temporal_begin, d); }
int rt_temporal_frame(rt_ctx* c, const rt_adaptive_desc* adaptive, const rt_denoise_desc* denoise, const float* world_to_film,
                      rt_pixel* film_out, rt_temporal_info* info) {
    return entry(c, impl_rt_temporal_frame, adaptive, denoise, world_to_film, film_out, info, false, nullptr);
}
int rt_temporal_frame_guided(rt_ctx* c, const rt_adaptive_desc* adaptive, const rt_denoise_desc* denoise,
                             const float* world_to_film, rt_pixel* film_out, rt_temporal_info* info,
                             rt_adaptive_info* session_info) {
    return entry(c, impl_rt_temporal_frame, adaptive, denoise, world_to_film, film_out, info, true, session_info);
}
int rt_temporal_block_error(rt_ctx* c, const rt_temporal_desc* d, const rt_adaptive_desc* adaptive, int res_x, int res_y,
                            const rt_pixel* film, const rt_moment* mom, const rt_feature* feat, const rt_position* pos,
                            const rt_pixel* hist_film, const rt_moment* hist_mom, const rt_feature* hist_feat,
                            const rt_position* hist_pos, const float* world_to_film_prev, float* block_error,
                            int32_t* converged) {
    return entry(c, impl_rt_temporal_block_error, d, adaptive, res_x, res_y, film, mom, feat, pos, hist_film, hist_mom,
                 hist_feat, hist_pos, world_to_film_prev, block_error, converged);
}
int rt_temporal_reset(rt_ctx* c) { return entry(c, impl_rt_temporal_reset); }
int rt_temporal_end(rt_ctx* c) { return entry(c, impl_rt_temporal_end); }
int rt_film_resolve(rt_ctx* c, const rt_pixel* film, uint8_t* out) { return entry(c, film_resolve, film, out, 0); }
int rt_film_resolve_srgb(rt_ctx* c, const rt_pixel* film, uint8_t* out) { return entry(c, film_resolve, film, out, 1); }
int rt_octree_get_info(rt_ctx* c, rt_octree_info* out) { return entry(c, impl_rt_octree_get_info, out); }
int rt_octree_export(rt_ctx* c, float* bounds, int32_t* child, int32_t* leaf_first, int32_t* leaf_count, int32_t* refs) {
    return entry(c, impl_rt_octree_export, bounds, child, leaf_first, leaf_count, refs);
}
int rt_bvh_export(rt_ctx* c, int set, int* n_nodes, int* n_tiles, float* consts, float* nodes, float* tiles) {
    return entry(c, impl_rt_bvh_export, set, n_nodes, n_tiles, consts, nodes, tiles);
}
// (no context: no message to keep)
int rt_debug_bvh_build(const rt_scene_desc* s, int set, int* n_nodes, int* n_tiles, float* consts, float* nodes, float* tiles) {
    return guarded([&] { return impl_rt_debug_bvh_build(s, set, n_nodes, n_tiles, consts, nodes, tiles); }, [](const std::string&) {});
}
int rt_debug_trace(rt_ctx* c, int n, const float* ro, const float* rd, int use_cull, int32_t* prim, float* bt) {
    return entry(c, impl_rt_debug_trace, n, ro, rd, use_cull, prim, bt);
}
int rt_debug_occluded(rt_ctx* c, int n, const float* ro, const float* rd, const float* tmax, int32_t* occluded) {
    return entry(c, impl_rt_debug_occluded, n, ro, rd, tmax, occluded);
}
int rt_debug_samples(rt_ctx* c, int n, const int32_t* pixel_ids, const int32_t* indices, rt_sample_record* out) {
    return entry(c, impl_rt_debug_samples, n, pixel_ids, indices, out);
}
int rt_scene_set_textures(rt_ctx* c, const rt_texture_desc* d) { return entry(c, impl_rt_scene_set_textures, d); }
int rt_debug_texture_bake(rt_ctx* c, int n, const uint8_t* rgb, float* coeffs) {
    return entry(c, impl_rt_debug_texture_bake, n, rgb, coeffs);
}
int rt_debug_texture_eval(rt_ctx* c, int n, const int32_t* prim, const float* b, int32_t* texel, float* coeffs) {
    return entry(c, impl_rt_debug_texture_eval, n, prim, b, texel, coeffs);
}
int rt_debug_meshlight_table(rt_ctx* c, int light, int* n, int32_t* tri, float* cdf, float* area) {
    return entry(c, impl_rt_debug_meshlight_table, light, n, tri, cdf, area);
}
int rt_debug_light_sample(rt_ctx* c, int light, int n, const float* po, const float* u, float* wi, float* tmax,
                          float* dist2, float* nl, int32_t* tri) {
    return entry(c, impl_rt_debug_light_sample, light, n, po, u, wi, tmax, dist2, nl, tri);
}
int rt_scene_set_environment(rt_ctx* c, const rt_environment_desc* d) { return entry(c, impl_rt_scene_set_environment, d); }
int rt_env_texel(int width, int height, const float* world_to_env, const float* dir, int* x, int* y, float* jac) {
    if (width < 1 || height < 1 || !world_to_env || !dir || !x || !y || !jac) return RT_E_ARG;
    float l2;
    env_dir_to_texel(width, height, world_to_env, dir, *x, *y, l2);
    *jac = env_pdf_omega(1.f, l2);
    return RT_OK;
}
int rt_debug_env_table(rt_ctx* c, int* w, int* h, float* coeffs4, float* cond, float* marg, float* total) {
    return entry(c, impl_rt_debug_env_table, w, h, coeffs4, cond, marg, total);
}
int rt_debug_env_sample(rt_ctx* c, int n, const float* u, float* wi, float* pdf, int32_t* texel) {
    return entry(c, impl_rt_debug_env_sample, n, u, wi, pdf, texel);
}
int rt_debug_env_eval(rt_ctx* c, int n, const float* dir, int32_t* texel, float* pdf) {
    return entry(c, impl_rt_debug_env_eval, n, dir, texel, pdf);
}
int rt_debug_env_stats(rt_ctx* c, double* ms_miss, int64_t* launches) {
    return entry(c, impl_rt_debug_env_stats, ms_miss, launches);
}
int rt_ggx_eval(float alpha, int n, const float* wo, const float* wi, float* fcos, float* pdf) {
    if (n < 0 || !ggx_alpha_ok(alpha) || (n && (!wo || !wi || !fcos || !pdf))) return RT_E_ARG;
    for (int i = 0; i < n; ++i)
        ggx_eval(alpha, V3{wo[3 * i], wo[3 * i + 1], wo[3 * i + 2]}, V3{wi[3 * i], wi[3 * i + 1], wi[3 * i + 2]}, fcos[i],
                 pdf[i]);
    return RT_OK;
}
int rt_ggx_sample(float alpha, int n, const float* wo, const float* disk, float* wi, float* wb, float* pdf) {
    if (n < 0 || !ggx_alpha_ok(alpha) || (n && (!wo || !disk || !wi || !wb || !pdf))) return RT_E_ARG;
    for (int i = 0; i < n; ++i) {
        V3 w;
        ggx_sample_disk(alpha, V3{wo[3 * i], wo[3 * i + 1], wo[3 * i + 2]}, disk[2 * i], disk[2 * i + 1], w, wb[i], pdf[i]);
        wi[3 * i] = w.x; wi[3 * i + 1] = w.y; wi[3 * i + 2] = w.z;
    }
    return RT_OK;
}
int rt_debug_ggx_sample(rt_ctx* c, float alpha, int n, const float* normal, const float* dir, const float* u,
                        float* disk_out, float* wi, float* wb, float* pdf) {
    return entry(c, impl_rt_debug_ggx_sample, alpha, n, normal, dir, u, disk_out, wi, wb, pdf);
}
int rt_debug_ggx_eval(rt_ctx* c, float alpha, int n, const float* normal, const float* dir, const float* wi, float* fcos,
                      float* pdf) {
    return entry(c, impl_rt_debug_ggx_eval, alpha, n, normal, dir, wi, fcos, pdf);
}
int rt_debug_rough_stats(rt_ctx* c, int64_t* launches) { return entry(c, impl_rt_debug_rough_stats, launches); }
int rt_roughglass_eval(float alpha, float eta_r, int n, const float* wo, const float* wi, float* fcos, float* pdf) {
    return guarded([&] {
        if (n < 0 || !ggx_alpha_ok(alpha) || !roughglass_er_ok(eta_r) || (n && (!wo || !wi || !fcos || !pdf))) return (int)RT_E_ARG;
        for (int i = 0; i < n; ++i)
            roughglass_eval(alpha, eta_r, V3{wo[3 * i], wo[3 * i + 1], wo[3 * i + 2]},
                            V3{wi[3 * i], wi[3 * i + 1], wi[3 * i + 2]}, fcos[i], pdf[i]);
        return (int)RT_OK;
    }, [](const std::string&) {});
}
int rt_roughglass_sample(float alpha, float eta_r, int n, const float* wo, const float* disk, const float* u, float* wi,
                         float* w, float* pdf, int32_t* branch) {
    return guarded([&] {
        if (n < 0 || !ggx_alpha_ok(alpha) || !roughglass_er_ok(eta_r) ||
            (n && (!wo || !disk || !u || !wi || !w || !pdf || !branch)))
            return (int)RT_E_ARG;
        for (int i = 0; i < n; ++i) {
            V3 v;
            branch[i] = roughglass_sample(alpha, eta_r, V3{wo[3 * i], wo[3 * i + 1], wo[3 * i + 2]}, disk[2 * i],
                                          disk[2 * i + 1], u[i], v, w[i], pdf[i]);
            wi[3 * i] = v.x; wi[3 * i + 1] = v.y; wi[3 * i + 2] = v.z;
        }
        return (int)RT_OK;
    }, [](const std::string&) {});
}
int rt_debug_roughglass_sample(rt_ctx* c, float alpha, float eta_r, int n, const float* normal, const float* dir,
                               const float* u, float* disk_out, float* wi, float* w, float* pdf, int32_t* branch) {
    return entry(c, impl_rt_debug_roughglass_sample, alpha, eta_r, n, normal, dir, u, disk_out, wi, w, pdf, branch);
}
int rt_debug_roughglass_eval(rt_ctx* c, float alpha, float eta_r, int n, const float* normal, const float* dir,
                             const float* wi, float* fcos, float* pdf) {
    return entry(c, impl_rt_debug_roughglass_eval, alpha, eta_r, n, normal, dir, wi, fcos, pdf);
}
int rt_debug_roughglass_stats(rt_ctx* c, int64_t* launches) { return entry(c, impl_rt_debug_roughglass_stats, launches); }
int rt_scene_set_media(rt_ctx* c, const rt_medium* media, int n_materials) {
    return entry(c, impl_rt_scene_set_media, media, n_materials);
}
// (rt_medium_transmittance: rt_medium_host.cpp)
int rt_debug_medium_eval(rt_ctx* c, const rt_medium* m, int n, const float* lambda, const float* len, float* out) {
    return entry(c, impl_rt_debug_medium_eval, m, n, lambda, len, out);
}
int rt_debug_medium_stats(rt_ctx* c, int* launches, unsigned long long* segments) {
    return entry(c, impl_rt_debug_medium_stats, launches, segments);
}
int rt_metal_nk(int metal, int n, const float* lambda, float* n_out, float* k_out) {
    return guarded([&] {
        if (metal < 0 || metal >= kMetals || n < 0 || (n && (!lambda || !n_out || !k_out))) return (int)RT_E_ARG;
        const float* t = metal_nk_table().data() + 2 * (size_t)metal * kMetalSpecN;
        for (int i = 0; i < n; ++i) {
            const float l = lambda[i];
            const long off = l > 0.f && l < 2000.f ? metal_index(l) : -1;  // (a NaN or a huge value is never cast)
            const bool in = off >= 0 && off < kMetalSpecN;
            n_out[i] = in ? t[2 * off] : 0.f;
            k_out[i] = in ? t[2 * off + 1] : 0.f;
        }
        return (int)RT_OK;
    }, [](const std::string&) {});
}
int rt_fresnel_conductor(int count, const float* cos, const float* n, const float* k, float* F) {
    return guarded([&] {
        if (count < 0 || (count && (!cos || !n || !k || !F))) return (int)RT_E_ARG;
        for (int i = 0; i < count; ++i) F[i] = fresnel_conductor(cos[i], n[i], k[i]);
        return (int)RT_OK;
    }, [](const std::string&) {});
}
int rt_debug_conductor_eval(rt_ctx* c, int metal, float alpha, int n, const float* normal, const float* dir,
                            const float* wi, const float* lambda, float* fcos, float* pdf, float* F) {
    return entry(c, impl_rt_debug_conductor_eval, metal, alpha, n, normal, dir, wi, lambda, fcos, pdf, F);
}
int rt_debug_conductor_stats(rt_ctx* c, int64_t* launches) { return entry(c, impl_rt_debug_conductor_stats, launches); }
int rt_debug_albedo_bake(rt_ctx* c, int n, const float* coeffs, float* rgb) {
    return entry(c, impl_rt_debug_albedo_bake, n, coeffs, rgb);
}
int rt_texel_index(int width, int height, int wrap, float u, float v) {
    if (width < 1 || height < 1 || (wrap != RT_TEX_CLAMP && wrap != RT_TEX_REPEAT)) return RT_E_ARG;
    return rtmi::texel_index(width, height, wrap, u, v);
}
int rt_debug_sort(rt_ctx* c, int which, int S, const int32_t* shard_len, const uint32_t* keys, const int32_t* slots,
                  int bits_a, int bits_b, int32_t* out, int32_t* out_len) {
    return entry(c, impl_rt_debug_sort, which, S, shard_len, keys, slots, bits_a, bits_b, out, out_len);
}
// (no context yet)
int rt_create(const rt_options* opt, rt_ctx** out) {
    return guarded([&] { return impl_rt_create(opt, out); }, [&](const std::string& m) { set_error(nullptr, m); });
}
int rt_scene_upload(rt_ctx* c, const rt_scene_desc* s) { return entry(c, impl_rt_scene_upload, s); }
int rt_camera_set(rt_ctx* c, const rt_camera_desc* d) { return entry(c, impl_rt_camera_set, d); }
int rt_sampler_set(rt_ctx* c, const rt_sampler_desc* d) { return entry(c, impl_rt_sampler_set, d); }
int rt_film_set(rt_ctx* c, const rt_film_desc* d) { return entry(c, impl_rt_film_set, d); }
int rt_integrator_set(rt_ctx* c, const rt_integrator_desc* d) { return entry(c, impl_rt_integrator_set, d); }
int rt_reset_stats(rt_ctx* c) { return entry(c, impl_rt_reset_stats); }
int rt_get_stats(rt_ctx* c, rt_stats* out) { return entry(c, impl_rt_get_stats, out); }
int rt_set_shard(rt_ctx* c, int tile_size, int n_shards, int shard_id) {
    return entry(c, impl_rt_set_shard, tile_size, n_shards, shard_id);
}
// (exempt from fault injection: an injected fault would only leak what it frees)
void rt_destroy(rt_ctx* c) {
    guarded([&] { impl_rt_destroy(c); return 0; }, [](const std::string&) {}, /*inject=*/false);
}

}  // extern "C"
