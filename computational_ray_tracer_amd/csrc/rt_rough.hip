// Rough reflector (RT_MAT_ROUGH): the path kernels' own device functions (rt_ggx.h through rt_device.h:
// ggx_frame, ggx_to_local, disk_concentric, ggx_sample_disk, ggx_eval, ggx_to_world) on explicit inputs, one item per
// thread, exactly as k_path_shade_full<.., RGH> calls them at a rough vertex (parity entry points).  float32 throughout,
// nothing fused (-ffp-contract=off), so tests/rough_reference.py restates every bit in numpy.
#include "rt_device.h"

namespace rtmi {

// nrm: the shading-side normal, dir: the incoming ray's direction (wo = -dir), u: the bounce's Get2D
__global__ void __launch_bounds__(kBlockThreads) k_ggx_sample(float alpha, int n, const float* __restrict__ nrm,
                                                              const float* __restrict__ dir, const float* __restrict__ u,
                                                              float2* __restrict__ disk, float4* __restrict__ wi,
                                                              float2* __restrict__ wbpdf) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const V3 nr = v3(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]);
    V3 ss, tt;
    ggx_frame(nr, ss, tt);
    const V3 wol = ggx_to_local(v3(-dir[3 * i], -dir[3 * i + 1], -dir[3 * i + 2]), ss, tt, nr);
    float dx, dy, wb, pdf;
    disk_concentric(u[2 * i], u[2 * i + 1], dx, dy);
    V3 wil, w = v3(0.f, 0.f, 0.f);
    if (ggx_sample_disk(alpha, wol, dx, dy, wil, wb, pdf)) w = ggx_to_world(wil, ss, tt, nr);
    disk[i] = make_float2(dx, dy);
    wi[i] = make_float4(w.x, w.y, w.z, 0.f);
    wbpdf[i] = make_float2(wb, pdf);
}

__global__ void __launch_bounds__(kBlockThreads) k_ggx_eval(float alpha, int n, const float* __restrict__ nrm,
                                                            const float* __restrict__ dir, const float* __restrict__ wi,
                                                            float2* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const V3 nr = v3(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]);
    V3 ss, tt;
    ggx_frame(nr, ss, tt);
    const V3 wol = ggx_to_local(v3(-dir[3 * i], -dir[3 * i + 1], -dir[3 * i + 2]), ss, tt, nr);
    const V3 wil = ggx_to_local(v3(wi[3 * i], wi[3 * i + 1], wi[3 * i + 2]), ss, tt, nr);
    float fc, pdf;
    ggx_eval(alpha, wol, wil, fc, pdf);
    out[i] = make_float2(fc, pdf);
}

hipError_t launch_ggx_sample(hipStream_t st, float alpha, int n, const float* nrm, const float* dir, const float* u,
                             float2* disk, float4* wi, float2* wbpdf) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_ggx_sample, dim3((n + kBlockThreads - 1) / kBlockThreads), dim3(kBlockThreads), 0, st, alpha, n,
                       nrm, dir, u, disk, wi, wbpdf);
    return hipGetLastError();
}
hipError_t launch_ggx_eval(hipStream_t st, float alpha, int n, const float* nrm, const float* dir, const float* wi,
                           float2* out) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_ggx_eval, dim3((n + kBlockThreads - 1) / kBlockThreads), dim3(kBlockThreads), 0, st, alpha, n,
                       nrm, dir, wi, out);
    return hipGetLastError();
}

}  // namespace rtmi
