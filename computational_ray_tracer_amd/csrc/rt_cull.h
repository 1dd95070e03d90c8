// The conservative box test of the single-leaf culling clusters (rt_kernels.hip cluster_mask; boxes built by
// rt_host.cpp leaf_clusters).  Plain C++ (host: tests/cluster_cull_driver.cpp) or HIP (device), like rt_mathf.h:
// explicit fma only, no contraction (-ffp-contract=off on both sides).
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RT_CULL_HD __host__ __device__ __forceinline__
#else
#include <hip/hip_vector_types.h>
#include <math.h>
#define RT_CULL_HD inline
#endif

// 1: the slab distances of the cluster cull are one FMA each, plane * inv - (o * inv), the products o * inv formed once
// per ray (cluster_hit_fma); 0: (plane - o) * inv per plane (cluster_hit).
#ifndef RT_CULL_FMA
#define RT_CULL_FMA 1
#endif

namespace rtmi {

struct V3 { float x, y, z; };

// helpers.h:50-54
RT_CULL_HD float gamma_n(int n) {
    const float me = 0x1p-24f;  // numeric_limits<float>::epsilon() * 0.5
    return ((float)n * me) / (1.0f - (float)n * me);
}

// Conservative box test for the single-leaf culling clusters only — never an octree node, whose test keeps
// Bounds3::IntersectP's exact operations (rt_device.h box_hit).  Same slab distances and tFar factor as box_hit, reduced
// with v_min/v_max (IEEE minNum/maxNum) instead of compare-and-select chains.  The one behavioural difference: a plane
// distance that is NaN (d_axis == 0 with the origin exactly on that plane) makes the other plane of the axis decide
// the slab; such a ray lies in the box's face plane, at least the cluster pad away from every triangle of the
// cluster (rt_host.cpp upload), so no candidate test of the cluster can pass and skipping it is exact.
RT_CULL_HD bool cluster_hit(float4 a, float4 b, V3 o, V3 inv, float tMax) {
    const float g = 1 + 2 * gamma_n(3);
    const float x0 = (a.x - o.x) * inv.x, x1 = (b.x - o.x) * inv.x;
    const float y0 = (a.y - o.y) * inv.y, y1 = (b.y - o.y) * inv.y;
    const float z0 = (a.z - o.z) * inv.z, z1 = (b.z - o.z) * inv.z;
    const float mn = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fmaxf(fminf(z0, z1), 0.f));
    const float mx = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1)) * g;
    return mn <= fminf(mx, tMax);
}

// The FMA form (RT_CULL_FMA): per ray oi = o * inv (cluster_oi), per plane fma(plane, inv, -oi): 18 VALU per box
// instead of 24.  The cull is a filter, no part of the parity contract: it only must never reject a box whose
// triangles' candidate tests could pass.  Conservative, next to the pad argument of rt_host.cpp leaf_clusters
// (u = 2^-24, per axis, c = the guard's centre, ext = the scene's extent):
//   * oi = o inv (1 + e1), and the fma rounds once: x = (plane inv - o inv (1 + e1)) (1 + e2) = inv (plane'' - o)
//     with |plane'' - plane| <= u |o| + u (1 + u) |plane - o|, i.e. the exact slab distance of a plane moved by at
//     most u (2 |o| + |plane|) (1 + u) <= 2^-23 (|plane| + |o|) along its axis.  (cluster_hit moves it by up to
//     2 u |plane - o|.)  The reduction, g, the clamp to [0, tMax] and the compare are cluster_hit's.
//   * Rays that may skip a box start inside the guard, |o - c| <= 8 ext, and a plane lies within .5 ext + pad of c, so
//     the move is <= u (3 |c| + 16.5 ext + pad) (1 + u): 0.99e-6 ext + 3 u |c|.  inv = fl(1 / d) itself scales an
//     axis' distances by (1 + e), another u |plane - o| <= 0.5e-6 ext (cluster_hit has it too).  With the 2.4e-6 ext
//     the candidate test needs that is 3.9e-6 ext + 3 u |c|.  The first part is under the pad's 1e-5 ext + 1e-3, so
//     kClusterPadRel stays; the second does not scale with the extent (a small scene far from the coordinate origin),
//     so leaf_clusters adds 2^-22 |c| = 4 u |c| to the pad, |c| = the centre's largest |coordinate| (the Cornell
//     box: 6.7e-5 on 6.6e-3).  The fourth u |c| pays for the rounding of the stored planes themselves, fl(bound -+ pad).
//   * Overflow.  o inv can overflow to +-inf with inv finite (|d_axis| < |o| / FLT_MAX); fma(plane, inv, -+inf) would
//     then be -+inf for BOTH planes whatever side they lie on and reject a slab the ray is inside of.  cluster_oi
//     turns an infinite oi into NaN (fma(0, oi, oi): 0 inf = NaN; exact for finite oi), so both distances are NaN,
//     fminf/fmaxf drop the slab and the other axes decide: culls less, never more.  The same happens for
//     d_axis == 0 (inv = +-inf: oi is +-inf, or NaN for o == 0), where cluster_hit gives (-inf, +inf) inside the
//     slab.  plane inv - oi overflowing with oi finite gives the infinity of the right sign.
//   * Underflow of oi or of the result moves the distance by <= 2^-126, a plane by <= 2^-126 |d_axis|: nothing.
RT_CULL_HD V3 cluster_oi(V3 o, V3 inv) {
    const float x = o.x * inv.x, y = o.y * inv.y, z = o.z * inv.z;
    return {__builtin_fmaf(0.f, x, x), __builtin_fmaf(0.f, y, y), __builtin_fmaf(0.f, z, z)};
}
RT_CULL_HD bool cluster_hit_fma(float4 a, float4 b, V3 oi, V3 inv, float tMax) {
    const float g = 1 + 2 * gamma_n(3);
    const float x0 = __builtin_fmaf(a.x, inv.x, -oi.x), x1 = __builtin_fmaf(b.x, inv.x, -oi.x);
    const float y0 = __builtin_fmaf(a.y, inv.y, -oi.y), y1 = __builtin_fmaf(b.y, inv.y, -oi.y);
    const float z0 = __builtin_fmaf(a.z, inv.z, -oi.z), z1 = __builtin_fmaf(b.z, inv.z, -oi.z);
    const float mn = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fmaxf(fminf(z0, z1), 0.f));
    const float mx = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fmaxf(z0, z1)) * g;
    return mn <= fminf(mx, tMax);
}

}  // namespace rtmi
