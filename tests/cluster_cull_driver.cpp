// The single-leaf cluster cull (csrc/rt_cull.h) against float64 on the host: no HIP library, no GPU.
//   cluster_cull_driver <triangles.txt> <seed> <segments> [<dx> <dy> <dz>]
// triangles.txt: 9 floats per line, a leaf's triangles in leaf order.  The boxes are rt_host.cpp leaf_clusters' (runs
// of 2 triangles, pad 1e-5 ext + 1e-3 + 2^-22 |centre|, guard = 8 extents around the centre); dx dy dz move the scene.  Every segment is tested against every
// cluster: where the float64 segment meets the UNPADDED bounds of the cluster's triangles, cluster_hit_fma (and
// cluster_hit) must answer true.  Prints counts; tests/test_cluster_cull.py asserts on them.
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../computational_ray_tracer_amd/csrc/rt_cull.h"

using namespace rtmi;

struct Rng {  // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    double u() { return (double)(next() >> 11) * 0x1p-53; }          // [0, 1)
    double s1() { return 2.0 * u() - 1.0; }                          // [-1, 1)
    int below(int n) { return (int)(next() % (uint64_t)n); }
};

struct Box { float lo[3], hi[3]; };  // unpadded bounds of a cluster's triangles
struct Seg { float o[3], d[3], tmax; };

// float64: does o + t d, t in [0, tmax], meet [lo, hi] (closed)?  tmax = FLT_MAX stands for the open ray.
static bool meets(const Box& b, const Seg& s) {
    double t0 = 0.0, t1 = s.tmax == FLT_MAX ? INFINITY : (double)s.tmax;
    for (int a = 0; a < 3; ++a) {
        const double o = s.o[a], d = s.d[a], lo = b.lo[a], hi = b.hi[a];
        if (d == 0.0) {
            if (o < lo || o > hi) return false;
            continue;
        }
        double ta = (lo - o) / d, tb = (hi - o) / d;
        if (ta > tb) { const double x = ta; ta = tb; tb = x; }
        if (ta > t0) t0 = ta;
        if (tb < t1) t1 = tb;
    }
    return t0 <= t1;
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    FILE* f = std::fopen(argv[1], "r");
    if (!f) return 2;
    std::vector<float> v;
    for (float x; std::fscanf(f, "%f", &x) == 1;) v.push_back(x);
    std::fclose(f);
    const int nt = (int)v.size() / 9;
    for (int a = 0; a < 3 && argc >= 7; ++a) {  // the scene moved away from the coordinate origin, in float
        const float off = std::strtof(argv[4 + a], nullptr);
        for (size_t i = a; i < v.size(); i += 3) v[i] += off;
    }
    Rng rng{(uint64_t)std::strtoull(argv[2], nullptr, 10)};
    const long nseg = std::strtol(argv[3], nullptr, 10);
    if (nt < 2 || nseg < 1) return 2;

    // leaf_clusters: the root bounds, the pad, the guard, the boxes
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = 0; i < nt * 3; ++i)
        for (int a = 0; a < 3; ++a) { mn[a] = std::fmin(mn[a], v[3 * i + a]); mx[a] = std::fmax(mx[a], v[3 * i + a]); }
    const float ext = std::fmax(std::fmax(mx[0] - mn[0], mx[1] - mn[1]), mx[2] - mn[2]);
    const float cen[3] = {.5f * (mn[0] + mx[0]), .5f * (mn[1] + mx[1]), .5f * (mn[2] + mx[2])};
    const float cmax = std::fmax(std::fmax(std::fabs(cen[0]), std::fabs(cen[1])), std::fabs(cen[2]));
    const float pad = 1e-5f * ext + 1e-3f + 0x1p-22f * cmax;  // (the last term: RT_CULL_FMA's, the default build)
    const double guard_r = 8.0 * ext;
    std::vector<Box> box;
    std::vector<float4> A, B;
    for (int k0 = 0; k0 < nt; k0 += 2) {
        Box b{{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}};
        for (int k = k0; k < nt && k < k0 + 2; ++k)
            for (int j = 0; j < 3; ++j)
                for (int a = 0; a < 3; ++a) {
                    b.lo[a] = std::fmin(b.lo[a], v[9 * k + 3 * j + a]);
                    b.hi[a] = std::fmax(b.hi[a], v[9 * k + 3 * j + a]);
                }
        box.push_back(b);
        float4 a4, b4;
        a4.x = b.lo[0] - pad; a4.y = b.lo[1] - pad; a4.z = b.lo[2] - pad; a4.w = 0.f;
        b4.x = b.hi[0] + pad; b4.y = b.hi[1] + pad; b4.z = b.hi[2] + pad; b4.w = 0.f;
        A.push_back(a4);
        B.push_back(b4);
    }
    const int ncl = (int)box.size();

    auto unit = [&](float d[3]) {
        double x, y, z, n;
        do { x = rng.s1(); y = rng.s1(); z = rng.s1(); n = x * x + y * y + z * z; } while (n > 1.0 || n < 1e-6);
        n = std::sqrt(n);
        d[0] = (float)(x / n); d[1] = (float)(y / n); d[2] = (float)(z / n);
    };
    auto origin = [&](float o[3]) {  // half inside the scene's bounds, half anywhere inside the guard
        if (rng.below(2)) {
            for (int a = 0; a < 3; ++a) o[a] = (float)(mn[a] + rng.u() * (mx[a] - mn[a]));
        } else {
            float d[3];
            unit(d);
            const double r = guard_r * 0.999 * std::cbrt(rng.u());
            for (int a = 0; a < 3; ++a) o[a] = (float)(cen[a] + r * d[a]);
        }
    };
    auto box_point = [&](const Box& b, float p[3]) {  // a corner, or a point of an edge, a face or the inside
        for (int a = 0; a < 3; ++a) {
            const int w = rng.below(3);
            p[a] = w == 0 ? b.lo[a] : w == 1 ? b.hi[a] : (float)(b.lo[a] + rng.u() * (b.hi[a] - b.lo[a]));
        }
    };

    long ref_hits = 0, viol_fma = 0, viol_old = 0, disagree = 0, fma_true = 0, old_true = 0, tests = 0, per_class[6] = {},
         dis_class[6] = {};
    long zero_pat[8] = {};
    for (long i = 0; i < nseg; ++i) {
        Seg s;
        const int cls = (int)(i % 6);
        origin(s.o);
        unit(s.d);
        switch (cls) {
            case 0: break;  // general
            case 1: {       // every pattern of zero components (1..6: not all three)
                const int m = 1 + (int)((i / 6) % 6);
                for (int a = 0; a < 3; ++a)
                    if (m >> a & 1) s.d[a] = rng.below(2) ? 0.f : -0.f;
                break;
            }
            case 2: {  // the origin on a face plane of a box, padded or not; the direction in that plane or not
                const int c = rng.below(ncl), a = rng.below(3), w = rng.below(4);
                s.o[a] = w == 0 ? box[c].lo[a] : w == 1 ? box[c].hi[a] : w == 2 ? (&A[c].x)[a] : (&B[c].x)[a];
                if (rng.below(2)) s.d[a] = 0.f;
                break;
            }
            case 3: {  // tiny components: 1 / d large or infinite, o / d beyond FLT_MAX
                const int a = rng.below(3);
                s.d[a] = (float)std::ldexp(rng.s1(), -(100 + rng.below(50)));
                if (rng.below(3) == 0) s.d[(a + 1) % 3] = (float)std::ldexp(rng.s1(), -(100 + rng.below(50)));
                break;
            }
            case 4: {  // aimed at a corner / edge / face point of a cluster's bounds
                float p[3];
                box_point(box[rng.below(ncl)], p);
                const double dx = (double)p[0] - s.o[0], dy = (double)p[1] - s.o[1], dz = (double)p[2] - s.o[2];
                const double n = std::sqrt(dx * dx + dy * dy + dz * dz);
                if (n > 0) { s.d[0] = (float)(dx / n); s.d[1] = (float)(dy / n); s.d[2] = (float)(dz / n); }
                break;
            }
            case 5: {  // along an edge of a cluster's bounds: from a corner, two zero components
                float p[3];
                const Box& b = box[rng.below(ncl)];
                for (int a = 0; a < 3; ++a) p[a] = rng.below(2) ? b.lo[a] : b.hi[a];
                const int a = rng.below(3);
                for (int k = 0; k < 3; ++k) { s.o[k] = p[k]; s.d[k] = 0.f; }
                s.d[a] = rng.below(2) ? 1.f : -1.f;
                s.o[a] = (float)(p[a] - s.d[a] * rng.u() * ext);
                break;
            }
        }
        // a shadow ray's finite tMax, or the closest-hit walk's FLT_MAX
        s.tmax = rng.below(2) ? FLT_MAX : (float)(rng.u() * 3.0 * ext);
        {   // inside the guard (rays from farther out never skip a cluster: nothing to test there)
            const double gx = (double)s.o[0] - cen[0], gy = (double)s.o[1] - cen[1], gz = (double)s.o[2] - cen[2];
            if (gx * gx + gy * gy + gz * gz > guard_r * guard_r) { --i; continue; }
        }
        ++per_class[cls];
        ++zero_pat[(s.d[0] == 0.f) | (s.d[1] == 0.f) << 1 | (s.d[2] == 0.f) << 2];
        const V3 o = {s.o[0], s.o[1], s.o[2]};
        const V3 inv = {1 / s.d[0], 1 / s.d[1], 1 / s.d[2]};
        const V3 oi = cluster_oi(o, inv);
        for (int c = 0; c < ncl; ++c) {
            const bool ref = meets(box[c], s);
            const bool hf = cluster_hit_fma(A[c], B[c], oi, inv, s.tmax);
            const bool ho = cluster_hit(A[c], B[c], o, inv, s.tmax);
            ++tests;
            ref_hits += ref;
            fma_true += hf;
            old_true += ho;
            disagree += hf != ho;
            dis_class[cls] += hf != ho;
            if (ref && !hf) {
                if (viol_fma++ < 10)
                    std::printf("miss_fma class %d cluster %d o %a %a %a d %a %a %a tmax %a\n", cls, c, s.o[0], s.o[1], s.o[2],
                                s.d[0], s.d[1], s.d[2], s.tmax);
            }
            viol_old += ref && !ho;
        }
    }
    std::printf("clusters %d\nsegments %ld\ntests %ld\nref_hits %ld\nfma_true %ld\nold_true %ld\nviolations_fma %ld\n"
                "violations_old %ld\ndisagree %ld\npad_e6 %ld\n", ncl, nseg, tests, ref_hits, fma_true, old_true, viol_fma, viol_old, disagree,
                (long)(pad * 1e6f));
    for (int k = 0; k < 6; ++k) std::printf("class%d %ld\ndisagree_class%d %ld\n", k, per_class[k], k, dis_class[k]);
    for (int k = 0; k < 8; ++k) std::printf("zeros%d %ld\n", k, zero_pat[k]);
    return 0;
}
