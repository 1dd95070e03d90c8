// Denoiser: the first-hit feature film and the variance-guided a-trous filter.
//
//   k_feature_film     one thread per owned pixel: adds the shading-side geometric normal and t of the batch's first
//                      hits, in increasing index order (the normal is k_path_shade_full's "surface" block); <true> also
//                      adds the hit point o + t d and a hit count to the position film
//   k_denoise_prepare  per pixel: c = rgb / n, the variance of the mean from the moment film, the guides
//                      g = (normal, depth) / k and the screen-space depth gradient
//   k_denoise_iter     one a-trous iteration with step s: the 3x3 blur of the variance, then the 25 taps in row-major
//                      order; <LDS> stages the block's tile with its 2s halo in LDS (steps 1 and 2), otherwise every
//                      tap is a plain load.  The last iteration also writes out = (c n, n) and the variance.
//   k_denoise_prepare_albedo, k_denoise_finish_albedo   albedo demodulation: prepare that also divides
//                      (c, var) by the pixel's floored albedo, and the multiplication back after the last iteration
//
// Everything is float32 in the order written (the build's -ffp-contract=off; / and sqrtf are correctly rounded) with
// only + - * /, sqrtf, fmaxf and fabsf, so a numpy float32 restatement gives the same bits (tests/denoise_reference.py).
#include "rt_device.h"
#include "rt_internal.h"

namespace rtmi {

namespace {

constexpr int kBlock = kBlockThreads;

template <bool POS>  // POS: also the position film, the sums of (o + t d, 1) over the same hits
__global__ void __launch_bounds__(kBlock) k_feature_film(DevScene sc, FeatureIO io) {
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < io.n_pixels; j += gridDim.x * blockDim.x) {
        const int pixel = io.work_pixels[j];
        float4 f = io.feat[pixel];
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (POS) q = io.pos[pixel];
        for (int i = 0; i < io.n_index; ++i) {
            const int s = i * io.n_pixels + j;
            const int prim = io.hitPrim[s];
            if (prim < 0) continue;
            const float4 d4 = io.rayD[(size_t)s << io.rsh];
            const float4 hb = io.hitB[s];
            const V3 rdw = v3(d4.x, d4.y, d4.z);
            V3 nrm;
            if (prim < sc.n_tris) {
                const float4 P0 = sc.triWorld[3 * prim], P1 = sc.triWorld[3 * prim + 1], P2 = sc.triWorld[3 * prim + 2];
                const V3 p0 = v3(P0.x, P0.y, P0.z), p1 = v3(P1.x, P1.y, P1.z), p2 = v3(P2.x, P2.y, P2.z);
                const V3 ng = vnorm(vcross(vsub(p0, p2), vsub(p1, p2)));
                nrm = ng;
                if (vdot(ng, vnorm(rdw)) > 0) nrm = v3(-ng.x, -ng.y, -ng.z);
            } else {
                const DevShape& sh = sc.shapes[prim - sc.n_tris];
                const V3 rdo = vnorm(m4_dir(sh.r2o, rdw));
                V3 no = shape_normal_obj(sh, v3(hb.x, hb.y, hb.z));
                if (vdot(no, rdo) > 0) no = v3(-no.x, -no.y, -no.z);
                nrm = vnorm(m3_mul(sh.n2r, no));
            }
            f.x += nrm.x;
            f.y += nrm.y;
            f.z += nrm.z;
            f.w += hb.w;
            if constexpr (POS) {
                const float4 o4 = io.rayO[(size_t)s << io.rsh];
                q.x += o4.x + hb.w * d4.x;
                q.y += o4.y + hb.w * d4.y;
                q.z += o4.z + hb.w * d4.z;
                q.w += 1.f;
            }
        }
        io.feat[pixel] = f;
        if constexpr (POS) io.pos[pixel] = q;
    }
}

// ------------------------------------------------------------------------------------------------ the filter
constexpr int kTX = 32, kTY = 8;  // pixels per thread block (kTX * kTY == kBlock)
static_assert(kTX * kTY == kBlock, "one thread per pixel of the tile");

__device__ __forceinline__ int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// One pixel of prepare.  ALB: the albedo variant, which divides c by the floored mean albedo a of the
// pixel's albedo film entry, the variance by the square of a's mean sa, and keeps (a, sa) for the finish.
template <bool ALB>
__device__ __forceinline__ void prepare_pixel(const DenoiseIO& io, const DemodIO* dm, int x, int y) {
    const int W = io.res_x, p = y * W + x;
    const float4 f = io.film[p];
    const float n = f.w;
    float4 cv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (n > 0.f) {
        cv.x = f.x / n;
        cv.y = f.y / n;
        cv.z = f.z / n;
    }
    if (n >= 2.f) {  // (as k_adaptive_error)
        const float2 m = io.mom[p];
        const float mean = m.x / n;
        const float d = fmaxf(m.y - m.x * mean, 0.f);
        cv.w = (d / (n - 1.f)) / n;
    }
    const float kf = io.kf;
    const float4 ft = io.feat[p];
    const int xl = clampi(x - 1, W - 1), xr = clampi(x + 1, W - 1), yd = clampi(y - 1, io.res_y - 1),
              yu = clampi(y + 1, io.res_y - 1);
    const float zl = io.feat[y * W + xl].w / kf, zr = io.feat[y * W + xr].w / kf;
    const float zd = io.feat[yd * W + x].w / kf, zu = io.feat[yu * W + x].w / kf;
    if constexpr (ALB) {
        const float4 al = dm->alb[p];
        float4 a = make_float4(1.f, 1.f, 1.f, 1.f);
        if (al.w > 0.f) {
            a.x = fmaxf(al.x / al.w, dm->floor);
            a.y = fmaxf(al.y / al.w, dm->floor);
            a.z = fmaxf(al.z / al.w, dm->floor);
        }
        a.w = ((a.x + a.y) + a.z) / 3.f;
        cv.x = cv.x / a.x;
        cv.y = cv.y / a.y;
        cv.z = cv.z / a.z;
        cv.w = cv.w / (a.w * a.w);
        dm->a[p] = a;
    }
    io.cv_out[p] = cv;
    io.g[p] = make_float4(ft.x / kf, ft.y / kf, ft.z / kf, ft.w / kf);
    io.gz[p] = make_float2((zr - zl) * 0.5f, (zu - zd) * 0.5f);
}

__global__ void __launch_bounds__(kBlock) k_denoise_prepare(DenoiseIO io) {
    const int x = (int)blockIdx.x * kTX + (int)(threadIdx.x % kTX), y = (int)blockIdx.y * kTY + (int)(threadIdx.x / kTX);
    if (x >= io.res_x || y >= io.res_y) return;
    prepare_pixel<false>(io, nullptr, x, y);
}

__global__ void __launch_bounds__(kBlock) k_denoise_prepare_albedo(DenoiseIO io, DemodIO dm) {
    const int x = (int)blockIdx.x * kTX + (int)(threadIdx.x % kTX), y = (int)blockIdx.y * kTY + (int)(threadIdx.x / kTX);
    if (x >= io.res_x || y >= io.res_y) return;
    prepare_pixel<true>(io, &dm, x, y);
}

// The albedo variant's finish: the last iteration's (c', var') times the albedo kept by prepare.
__global__ void __launch_bounds__(kBlock) k_denoise_finish_albedo(DenoiseIO io, DemodIO dm, const float4* __restrict__ cv,
                                                                  float4* __restrict__ out, float* __restrict__ var_out) {
    const int x = (int)blockIdx.x * kTX + (int)(threadIdx.x % kTX), y = (int)blockIdx.y * kTY + (int)(threadIdx.x / kTX);
    if (x >= io.res_x || y >= io.res_y) return;
    const int p = y * io.res_x + x;
    const float4 r = cv[p], a = dm.a[p];
    const float n = io.film[p].w;
    out[p] = make_float4((r.x * a.x) * n, (r.y * a.y) * n, (r.z * a.z) * n, n);
    if (var_out) var_out[p] = r.w * (a.w * a.w);
}

// the compact kernel e(x) = q^8, q = max(1 - x / 8, 0)
__device__ __forceinline__ float e8(float x) {
    float q = fmaxf(1.f - x * 0.125f, 0.f);
    q = q * q;
    q = q * q;
    return q * q;
}

// One pixel of an iteration.  at(xq, yq, cq, gq) loads (c, var) and the guide of an in-image pixel; var_at(xq, yq) its
// variance alone.
template <class At, class VarAt>
__device__ __forceinline__ void denoise_pixel(const DenoiseIO& io, int x, int y, At at, VarAt var_at) {
    const int W = io.res_x, H = io.res_y, s = io.step, p = y * W + x;
    float vbar = 0.f;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
            const float wgt = (dx == 0 ? 0.5f : 0.25f) * (dy == 0 ? 0.5f : 0.25f);
            vbar = vbar + wgt * var_at(clampi(x + dx, W - 1), clampi(y + dy, H - 1));
        }
    float4 cp, gp;
    at(x, y, cp, gp);
    const float2 gz = io.gz[p];
    const float lp = (cp.x + cp.y) + cp.z;
    const float den_l = (io.sigma_l * sqrtf(vbar) + io.lum_floor) + 1e-30f;
    const float dz = io.depth_floor * gp.w;
    float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, sv = 0.f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
        const float ky = dy == 0 ? 0.375f : (dy == 1 || dy == -1 ? 0.25f : 0.0625f);
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const float kx = dx == 0 ? 0.375f : (dx == 1 || dx == -1 ? 0.25f : 0.0625f);
            const float h = kx * ky;
            const int ox = s * dx, oy = s * dy;
            const int xq = x + ox, yq = y + oy;
            float w;
            float4 cq;
            if (dx == 0 && dy == 0) {
                w = h;
                cq = cp;
            } else {
                if (xq < 0 || xq >= W || yq < 0 || yq >= H) continue;
                float4 gq;
                at(xq, yq, cq, gq);
                float wn = fmaxf((gp.x * gq.x + gp.y * gq.y) + gp.z * gq.z, 0.f);
                for (int j = 0; j < io.normal_power_log2; ++j) wn = wn * wn;
                const float xz = fabsf(gq.w - gp.w) /
                                 (((io.sigma_z * fabsf(gz.x * (float)ox + gz.y * (float)oy)) + dz) + 1e-30f);
                const float lq = (cq.x + cq.y) + cq.z;
                const float xl = fabsf(lq - lp) / den_l;
                w = ((h * wn) * e8(xz)) * e8(xl);
            }
            sw = sw + w;
            sr = sr + w * cq.x;
            sg = sg + w * cq.y;
            sb = sb + w * cq.z;
            sv = sv + (w * w) * cq.w;
        }
    }
    const float4 r = make_float4(sr / sw, sg / sw, sb / sw, sv / (sw * sw));
    if (io.out) {  // the last iteration: finish
        const float n = io.film[p].w;
        io.out[p] = make_float4(r.x * n, r.y * n, r.z * n, n);
        if (io.var_out) io.var_out[p] = r.w;
    } else {
        io.cv_out[p] = r;
    }
}

template <int S>  // S > 0: the tile and its 2 S halo staged in LDS (io.step == S); 0: plain loads
__global__ void __launch_bounds__(kBlock) k_denoise_iter(DenoiseIO io) {
    const int tx = (int)(threadIdx.x % kTX), ty = (int)(threadIdx.x / kTX);
    const int x0 = (int)blockIdx.x * kTX, y0 = (int)blockIdx.y * kTY;
    const int x = x0 + tx, y = y0 + ty;
    const int W = io.res_x, H = io.res_y;
    if constexpr (S > 0) {
        constexpr int R = 2 * S, LW = kTX + 2 * R, LH = kTY + 2 * R;
        __shared__ float4 l_cv[LH * LW];
        __shared__ float4 l_g[LH * LW];
        for (int k = (int)threadIdx.x; k < LW * LH; k += kBlock) {
            const int ly = k / LW, lx = k - ly * LW;
            const int gx = x0 - R + lx, gy = y0 - R + ly;
            if (gx >= 0 && gx < W && gy >= 0 && gy < H) {  // (entries outside the image are never read)
                l_cv[k] = io.cv_in[gy * W + gx];
                l_g[k] = io.g[gy * W + gx];
            }
        }
        __syncthreads();
        if (x >= W || y >= H) return;
        denoise_pixel(
            io, x, y,
            [&](int xq, int yq, float4& c, float4& g) {
                const int k = (yq - y0 + R) * LW + (xq - x0 + R);
                c = l_cv[k];
                g = l_g[k];
            },
            [&](int xq, int yq) { return l_cv[(yq - y0 + R) * LW + (xq - x0 + R)].w; });
    } else {
        if (x >= W || y >= H) return;
        denoise_pixel(
            io, x, y,
            [&](int xq, int yq, float4& c, float4& g) {
                c = io.cv_in[yq * W + xq];
                g = io.g[yq * W + xq];
            },
            [&](int xq, int yq) { return io.cv_in[yq * W + xq].w; });
    }
}

dim3 tile_grid(const DenoiseIO& io) { return dim3((io.res_x + kTX - 1) / kTX, (io.res_y + kTY - 1) / kTY); }

}  // namespace

hipError_t launch_feature_film(hipStream_t st, const DevScene& sc, const FeatureIO& io) {
    if (io.n_pixels <= 0 || io.n_index <= 0) return hipSuccess;
    const dim3 grid((io.n_pixels + kBlock - 1) / kBlock), block(kBlock);
    if (io.pos) hipLaunchKernelGGL(k_feature_film<true>, grid, block, 0, st, sc, io);
    else hipLaunchKernelGGL(k_feature_film<false>, grid, block, 0, st, sc, io);
    return hipGetLastError();
}

hipError_t launch_denoise_prepare(hipStream_t st, const DenoiseIO& io) {
    hipLaunchKernelGGL(k_denoise_prepare, tile_grid(io), dim3(kBlock), 0, st, io);
    return hipGetLastError();
}

hipError_t launch_denoise_prepare_albedo(hipStream_t st, const DenoiseIO& io, const DemodIO& dm) {
    hipLaunchKernelGGL(k_denoise_prepare_albedo, tile_grid(io), dim3(kBlock), 0, st, io, dm);
    return hipGetLastError();
}

hipError_t launch_denoise_finish_albedo(hipStream_t st, const DenoiseIO& io, const DemodIO& dm, const float4* cv,
                                        float4* out, float* var_out) {
    hipLaunchKernelGGL(k_denoise_finish_albedo, tile_grid(io), dim3(kBlock), 0, st, io, dm, cv, out, var_out);
    return hipGetLastError();
}

hipError_t launch_denoise_iter(hipStream_t st, const DenoiseIO& io, bool lds) {
    const dim3 grid = tile_grid(io), block(kBlock);
    if (lds && io.step == 1) hipLaunchKernelGGL(k_denoise_iter<1>, grid, block, 0, st, io);
    else if (lds && io.step == 2) hipLaunchKernelGGL(k_denoise_iter<2>, grid, block, 0, st, io);
    else hipLaunchKernelGGL(k_denoise_iter<0>, grid, block, 0, st, io);
    return hipGetLastError();
}

}  // namespace rtmi
