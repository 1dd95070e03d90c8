// Albedo demodulation: the sensor-RGB albedo of every material and texel, and the albedo film of a
// feature pass's first hits.  The filter's demodulating variants live in rt_denoise.hip.
//
//   k_albedo_bake   one thread per entry: A_c = sum_k (bar_c[k] D65[k]) R(360 + k) / sum_k bar_c[k] D65[k] over the 471
//                   integer nanometres, k ascending, with SPK = {SR, SG, SB, D65} staged in LDS as the shade kernels do
//   k_albedo_film   one thread per owned pixel: adds (A, 1) of the batch's first hits, in increasing index order
//
// Everything is float32 in the order written (-ffp-contract=off) with only + - * / and sqrtf: the albedo guide is
// build-defined like the filter, and tests/albedo_reference.py restates it in numpy to the bit.
#include "rt_device.h"
#include "rt_internal.h"

namespace rtmi {

namespace {

constexpr int kBlock = kBlockThreads;

__global__ void __launch_bounds__(kBlock) k_albedo_bake(const DevSpectra* __restrict__ sp, int n_mat,
                                                        const DevMaterial* __restrict__ mats, unsigned n,
                                                        const float4* __restrict__ coeffs, float4* __restrict__ out) {
    __shared__ float4 l_spk[kSpecN];
    for (int k = threadIdx.x; k < kSpecN; k += blockDim.x) l_spk[k] = sp->SPK[k];
    __syncthreads();
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;  // (n < 2^31: the last block's ids stay below 2^32)
    if (i >= n) return;
    float c0, c1, c2;
    if (i < (unsigned)n_mat) {
        const DevMaterial m = mats[i];
        c0 = m.c0; c1 = m.c1; c2 = m.c2;
    } else {
        const float4 t = coeffs[i - (unsigned)n_mat];
        c0 = t.x; c1 = t.y; c2 = t.z;
    }
    float num[3] = {0.f, 0.f, 0.f}, den[3] = {0.f, 0.f, 0.f};
    for (int k = 0; k < kSpecN; ++k) {
        const float lam = (float)(360 + k);
        const float x = (lam * c0 + c1) * lam + c2;  // (not fused, unlike sigmoid_eval: numpy has no fmaf)
        float s;
        if (__builtin_isinf(x)) s = x > 0 ? 1.f : 0.f;
        else s = 0.5f + x / (2.f * sqrtf(1.f + x * x));
        const float4 t = l_spk[k];
        const float w[3] = {t.x * t.w, t.y * t.w, t.z * t.w};
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
            num[ch] = num[ch] + w[ch] * s;
            den[ch] = den[ch] + w[ch];
        }
    }
    out[i] = make_float4(num[0] / den[0], num[1] / den[1], num[2] / den[2], 0.f);
}

template <bool TEX>
__global__ void __launch_bounds__(kBlock) k_albedo_film(DevScene sc, AlbedoFilmIO io) {
    DevTex tx{};
    if constexpr (TEX) tx = *io.tex;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < io.n_pixels; j += gridDim.x * blockDim.x) {
        const int pixel = io.work_pixels[j];
        float4 f = io.alb[pixel];
        for (int i = 0; i < io.n_index; ++i) {
            const int s = i * io.n_pixels + j;
            const int prim = io.hitPrim[s];
            if (prim < 0) continue;
            float4 a = make_float4(1.f, 1.f, 1.f, 0.f);
            if (!io.reference) {
                const bool tri = prim < sc.n_tris;
                const int mid = tri ? sc.triMaterial[prim] : sc.shapes[prim - sc.n_tris].material;
                const DevMaterial mt = sc.materials[mid];
                if (!(mt.emit > 0 || mt.cls == 1)) {  // emitters and specular surfaces are not demodulated
                    int e = mid;
                    if constexpr (TEX) {
                        if (tri) {
                            const float4 hb = io.hitB[s];
                            int gidx;
                            float c0, c1, c2;
                            if (tex_fetch(tx, prim, mid, hb.x, hb.y, hb.z, gidx, c0, c1, c2) >= 0)
                                e = sc.n_materials + gidx;
                        }
                    }
                    a = io.table[e];
                }
            }
            f.x += a.x;
            f.y += a.y;
            f.z += a.z;
            f.w += 1.f;
        }
        io.alb[pixel] = f;
    }
}

}  // namespace

hipError_t launch_albedo_bake(hipStream_t st, const DevSpectra* sp, int n_mat, const DevMaterial* mats, int n_coeffs,
                              const float4* coeffs, float4* out) {
    const unsigned n = (unsigned)n_mat + (unsigned)n_coeffs;
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_albedo_bake, dim3((n + kBlock - 1) / kBlock), dim3(kBlock), 0, st, sp, n_mat, mats, n, coeffs,
                       out);
    return hipGetLastError();
}

hipError_t launch_albedo_film(hipStream_t st, const DevScene& sc, const AlbedoFilmIO& io) {
    if (io.n_pixels <= 0 || io.n_index <= 0) return hipSuccess;
    const dim3 grid((io.n_pixels + kBlock - 1) / kBlock), block(kBlock);
    if (io.tex) hipLaunchKernelGGL(k_albedo_film<true>, grid, block, 0, st, sc, io);
    else hipLaunchKernelGGL(k_albedo_film<false>, grid, block, 0, st, sc, io);
    return hipGetLastError();
}

}  // namespace rtmi
