// Rough glass (RT_MAT_ROUGH_DIELECTRIC): the path kernels' own device functions (rt_ggx.h and
// rt_roughglass.h through rt_device.h: ggx_frame, ggx_to_local, disk_concentric, roughglass_sample, roughglass_eval,
// ggx_to_world) on explicit inputs, one item per thread, exactly as k_path_shade_full<.., RGH = 3> calls them at a
// rough-glass vertex (parity entry points).  float32 throughout, nothing fused (-ffp-contract=off), so
// tests/roughglass_reference.py restates every bit in numpy.
#include "rt_device.h"

namespace rtmi {

// nrm: the shading-side normal, dir: the incoming ray's direction (wo = -dir), u: the bounce's Get2D then its Get1D,
// er: the relative index of the shading side
__global__ void __launch_bounds__(kBlockThreads) k_roughglass_sample(float alpha, float er, int n,
                                                                     const float* __restrict__ nrm,
                                                                     const float* __restrict__ dir,
                                                                     const float* __restrict__ u,
                                                                     float2* __restrict__ disk, float4* __restrict__ wi,
                                                                     float2* __restrict__ wpdf) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const V3 nr = v3(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]);
    V3 ss, tt;
    ggx_frame(nr, ss, tt);
    const V3 wol = ggx_to_local(v3(-dir[3 * i], -dir[3 * i + 1], -dir[3 * i + 2]), ss, tt, nr);
    float dx, dy, w, pdf;
    disk_concentric(u[3 * i], u[3 * i + 1], dx, dy);
    V3 wil, ww = v3(0.f, 0.f, 0.f);
    const int br = roughglass_sample(alpha, er, wol, dx, dy, u[3 * i + 2], wil, w, pdf);
    if (br) ww = ggx_to_world(wil, ss, tt, nr);
    disk[i] = make_float2(dx, dy);
    wi[i] = make_float4(ww.x, ww.y, ww.z, (float)br);
    wpdf[i] = make_float2(w, pdf);
}

__global__ void __launch_bounds__(kBlockThreads) k_roughglass_eval(float alpha, float er, int n,
                                                                   const float* __restrict__ nrm,
                                                                   const float* __restrict__ dir,
                                                                   const float* __restrict__ wi,
                                                                   float2* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const V3 nr = v3(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]);
    V3 ss, tt;
    ggx_frame(nr, ss, tt);
    const V3 wol = ggx_to_local(v3(-dir[3 * i], -dir[3 * i + 1], -dir[3 * i + 2]), ss, tt, nr);
    const V3 wil = ggx_to_local(v3(wi[3 * i], wi[3 * i + 1], wi[3 * i + 2]), ss, tt, nr);
    float fc, pdf;
    roughglass_eval(alpha, er, wol, wil, fc, pdf);
    out[i] = make_float2(fc, pdf);
}

hipError_t launch_roughglass_sample(hipStream_t st, float alpha, float er, int n, const float* nrm, const float* dir,
                                    const float* u, float2* disk, float4* wi, float2* wpdf) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_roughglass_sample, dim3((n + kBlockThreads - 1) / kBlockThreads), dim3(kBlockThreads), 0, st,
                       alpha, er, n, nrm, dir, u, disk, wi, wpdf);
    return hipGetLastError();
}
hipError_t launch_roughglass_eval(hipStream_t st, float alpha, float er, int n, const float* nrm, const float* dir,
                                  const float* wi, float2* out) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_roughglass_eval, dim3((n + kBlockThreads - 1) / kBlockThreads), dim3(kBlockThreads), 0, st, alpha,
                       er, n, nrm, dir, wi, out);
    return hipGetLastError();
}

}  // namespace rtmi
