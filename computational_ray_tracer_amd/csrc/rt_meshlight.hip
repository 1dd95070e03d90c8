// Mesh area lights (RT_LIGHT_MESH): the device table of a light's emissive triangles — areas, their
// inclusive prefix sums in a fixed order, the normalised cdf — built at upload once triWorld is resident, and the
// kernels' own light_ray (rt_device.h) on explicit inputs (parity entry point).  float32 throughout, nothing fused
// (-ffp-contract=off), so tests/meshlight_reference.py restates every bit in numpy.
#include "rt_device.h"

namespace rtmi {

// One block of one wave per light (blockIdx.x = the light's job).  The wave walks the light's n triangles 64 at a
// time: area_i = 0.5f sqrtf(cr . cr), cr = (p0 - p2) x (p1 - p2); inside a chunk the shuffle-up scan of
// k_adaptive_scan (v += shfl_up(v, o) for o = 1 .. 32, lanes below o keep theirs); S_i = carry + v, carry = the S of
// the previous chunk's last entry (0 for the first chunk).  A second walk divides by A = S_{n-1}: cdf_i = S_i / A, so
// cdf_{n-1} is exactly 1.  sums is scratch of the table's size; area[job] = A.
struct MeshLightJob {
    int first, n;  // the light's slice of tri / cdf
};
__global__ void __launch_bounds__(64) k_meshlight_table(const float4* __restrict__ triWorld,
                                                        const MeshLightJob* __restrict__ jobs,
                                                        const int* __restrict__ tri, float* __restrict__ sums,
                                                        float* __restrict__ cdf, float* __restrict__ area) {
    const MeshLightJob job = jobs[blockIdx.x];
    const int l = (int)threadIdx.x;
    float carry = 0.f;
    for (int base = 0; base < job.n; base += 64) {
        const int i = base + l;
        float v = 0.f;
        if (i < job.n) {
            const int t = tri[job.first + i];
            const float4 P0 = triWorld[3 * t], P1 = triWorld[3 * t + 1], P2 = triWorld[3 * t + 2];
            const V3 p0 = v3(P0.x, P0.y, P0.z), p1 = v3(P1.x, P1.y, P1.z), p2 = v3(P2.x, P2.y, P2.z);
            const V3 cr = vcross(vsub(p0, p2), vsub(p1, p2));
            v = 0.5f * sqrtf(vdot(cr, cr));
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float u = __shfl_up(v, o);
            if (l >= o) v += u;
        }
        const float S = carry + v;
        if (i < job.n) sums[job.first + i] = S;
        // the chunk's last entry: lane 63, or the lane of S_{n-1} in the last chunk (a tail lane's scan value sums the
        // same areas in another association, so it is not read)
        const int rem = job.n - 1 - base;
        carry = __shfl(S, rem < 63 ? rem : 63);
    }
    const float A = carry;  // S_{n-1}; each lane divides the sums it wrote itself
    for (int i = l; i < job.n; i += 64) cdf[job.first + i] = sums[job.first + i] / A;
    if (l == 0) area[blockIdx.x] = A;
}

hipError_t launch_meshlight_table(hipStream_t st, const float4* triWorld, int n_jobs, const int* jobs2, const int* tri,
                                  float* sums, float* cdf, float* area) {
    if (n_jobs <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_meshlight_table, dim3(n_jobs), dim3(64), 0, st, triWorld,
                       reinterpret_cast<const MeshLightJob*>(jobs2), tri, sums, cdf, area);
    return hipGetLastError();
}

// light_ray as k_path_shade_full and k_path_nee call it (the TL = 1 instantiation), one sample per thread:
// out[i] = (wi, tmax), (dist2, nl), tri; nl = the light's n and tri = -1 unless the light is a mesh light
__global__ void __launch_bounds__(kBlockThreads) k_light_sample(DevScene sc, int light, int n,
                                                                const float* __restrict__ po,
                                                                const float* __restrict__ u, float4* __restrict__ a,
                                                                float4* __restrict__ b, int* __restrict__ tri) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const DevLight Lt = sc.lights[light];
    MeshSample ms;
    ms.nl = v3(Lt.n[0], Lt.n[1], Lt.n[2]);
    ms.tri = -1;
    const LightRay r = light_ray<1>(Lt, v3(po[3 * i], po[3 * i + 1], po[3 * i + 2]), u[2 * i], u[2 * i + 1],
                                       sc.triWorld, ms);
    a[i] = make_float4(r.wi.x, r.wi.y, r.wi.z, r.tmax);
    b[i] = make_float4(r.dist2, ms.nl.x, ms.nl.y, ms.nl.z);
    tri[i] = ms.tri;
}

hipError_t launch_light_sample(hipStream_t st, const DevScene& sc, int light, int n, const float* po, const float* u,
                               float4* a, float4* b, int* tri) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_light_sample, dim3((n + kBlockThreads - 1) / kBlockThreads), dim3(kBlockThreads), 0, st, sc,
                       light, n, po, u, a, b, tri);
    return hipGetLastError();
}

}  // namespace rtmi
