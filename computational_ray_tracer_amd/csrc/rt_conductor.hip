// Metal (RT_MAT_CONDUCTOR): the path kernels' own device functions (rt_ggx.h and rt_fresnel.h through
// rt_device.h: ggx_frame, ggx_to_local, ggx_eval_h, metal_nk_query, fresnel_conductor) on explicit inputs, one item per
// thread, exactly as k_path_shade_full<.., 2> and k_path_nee<.., 2> call them for a light's wi at a conductor vertex
// (parity entry point).  float32 throughout, nothing fused (-ffp-contract=off), so tests/metal_reference.py restates every
// bit in numpy.
#include "rt_device.h"

namespace rtmi {

// nrm: the shading-side normal, dir: the incoming ray's direction (wo = -dir), wi: the light's direction (world space),
// lambda: the wavelength -> out = (fcos, pdf, F(lambda, wo.h), wo.h)
__global__ void __launch_bounds__(kBlockThreads) k_conductor_eval(const DevSpectra* __restrict__ sp, int metal, float alpha,
                                                                  int n, const float* __restrict__ nrm,
                                                                  const float* __restrict__ dir,
                                                                  const float* __restrict__ wi,
                                                                  const float* __restrict__ lambda,
                                                                  float4* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const V3 nr = v3(nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]);
    V3 ss, tt;
    ggx_frame(nr, ss, tt);
    const V3 wol = ggx_to_local(v3(-dir[3 * i], -dir[3 * i + 1], -dir[3 * i + 2]), ss, tt, nr);
    const V3 wil = ggx_to_local(v3(wi[3 * i], wi[3 * i + 1], wi[3 * i + 2]), ss, tt, nr);
    float fc, pdf, ch;
    ggx_eval_h(alpha, wol, wil, fc, pdf, ch);
    const float2 nk = metal_nk_query(sp, metal, lambda[i]);
    out[i] = make_float4(fc, pdf, fresnel_conductor(ch, nk.x, nk.y), ch);
}

hipError_t launch_conductor_eval(hipStream_t st, const DevSpectra* sp, int metal, float alpha, int n, const float* nrm,
                                 const float* dir, const float* wi, const float* lambda, float4* out) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_conductor_eval, dim3((n + kBlockThreads - 1) / kBlockThreads), dim3(kBlockThreads), 0, st, sp,
                       metal, alpha, n, nrm, dir, wi, lambda, out);
    return hipGetLastError();
}

}  // namespace rtmi
