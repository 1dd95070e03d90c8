// Albedo textures: the bake of RGB8 texels into sigmoid coefficients, and the shade kernels' fetch on
// explicit inputs (parity entry point).  The fetch itself lives in rt_device.h (tex_fetch) and is compiled into the TEX
// instantiations of k_path_shade_full and k_path_nee (rt_kernels.hip).  Plain global loads and stores: the fetch is
// nearest-texel and must be bit-reproducible, so no texture object and no filtering hardware.
#include "rt_device.h"

namespace rtmi {

// One thread per texel: rgb = byte / 255.f per channel, as a division (RayTracerTestApp.h:236), then
// RGBToSpectrumTable::operator() (rt_texture.h rgb_to_sigmoid, the text rt_rgb_to_sigmoid runs on the host).
__global__ void __launch_bounds__(kBlockThreads) k_texture_bake(const float* __restrict__ table, int n,
                                                                const unsigned char* __restrict__ rgb,
                                                                float4* __restrict__ out) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;  // (n < 2^31: the last block's ids stay below 2^32)
    if (i >= (unsigned)n) return;
    const size_t o = 3 * (size_t)i;
    const float c[3] = {(float)rgb[o] / 255.f, (float)rgb[o + 1] / 255.f, (float)rgb[o + 2] / 255.f};
    float k[3];
    rgb_to_sigmoid(table, table + kRgbRes, c, k);
    out[i] = make_float4(k[0], k[1], k[2], 0.f);
}

template <bool TEX>
__global__ void __launch_bounds__(kBlockThreads) k_texture_eval(DevScene sc, const DevTex* tex, int n,
                                                                const int* __restrict__ prim,
                                                                const float* __restrict__ b, int* __restrict__ texel,
                                                                float4* __restrict__ coeffs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int p = prim[i];
    const int mid = sc.triMaterial[p];
    const DevMaterial mt = sc.materials[mid];
    float c0 = mt.c0, c1 = mt.c1, c2 = mt.c2;
    int idx = -1;
    if constexpr (TEX) {
        const DevTex tx = *tex;
        int gidx;
        idx = tex_fetch(tx, p, mid, b[3 * i], b[3 * i + 1], b[3 * i + 2], gidx, c0, c1, c2);
    }
    texel[i] = idx;
    coeffs[i] = make_float4(c0, c1, c2, 0.f);
}

hipError_t launch_texture_bake(hipStream_t st, const float* table, int n, const unsigned char* rgb, float4* out) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_texture_bake, dim3((n + kBlockThreads - 1) / kBlockThreads), dim3(kBlockThreads), 0, st, table,
                       n, rgb, out);
    return hipGetLastError();
}

hipError_t launch_texture_eval(hipStream_t st, const DevScene& sc, const DevTex* tex, int n, const int* prim,
                               const float* b, int* texel, float4* coeffs) {
    if (n <= 0) return hipSuccess;
    const dim3 g((n + kBlockThreads - 1) / kBlockThreads), t(kBlockThreads);
    if (tex) hipLaunchKernelGGL(k_texture_eval<true>, g, t, 0, st, sc, tex, n, prim, b, texel, coeffs);
    else hipLaunchKernelGGL(k_texture_eval<false>, g, t, 0, st, sc, tex, n, prim, b, texel, coeffs);
    return hipGetLastError();
}

}  // namespace rtmi
