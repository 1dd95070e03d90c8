// Image environment light (RT_LIGHT_ENV): the upload-time bake and cdf table of the map, the per-depth
// miss stage of the general path integrator, and the kernels' own env_sample / env_eval (rt_device.h) on explicit inputs
// (parity entry points).  float32 throughout, nothing fused (-ffp-contract=off), so tests/envlight_reference.py restates
// every bit of the bake weights, the table, the sampling and the lookup in numpy.
#include "rt_device.h"

namespace rtmi {

// One thread per texel: (c0, c1, c2, m) with m = 2 max(r, g, b) and the coefficients of rgb / m (the texture bake's
// rgb_to_sigmoid; every component <= 0.5), all 0 for a black texel; and the distribution's weight
// max(r, g, b) / (l2 sqrtf(l2)), l2 = p . p at the texel centre: brightness times the texel's solid angle up to 4 / (W H).
__global__ void __launch_bounds__(kBlockThreads) k_env_bake(const float* __restrict__ table, int W, int H,
                                                            const float* __restrict__ rgb, float4* __restrict__ coef,
                                                            float* __restrict__ wgt) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;  // (W H <= 2^24)
    if (i >= (unsigned)(W * H)) return;
    const size_t o = 3 * (size_t)i;
    const float r = rgb[o], g = rgb[o + 1], b = rgb[o + 2];
    const float mx = max3f(r, g, b);
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f);
    if (mx > 0.f) {
        const float m = 2.f * mx;
        const float q[3] = {r / m, g / m, b / m};
        float k[3];
        rgb_to_sigmoid(table, table + kRgbRes, q, k);
        c = make_float4(k[0], k[1], k[2], m);
    }
    coef[i] = c;
    const int x = (int)(i % (unsigned)W), y = (int)(i / (unsigned)W);
    float p[3];
    env_st_to_point(((float)x + 0.5f) / (float)W, ((float)y + 0.5f) / (float)H, p);
    const float l2 = (p[0] * p[0] + p[1] * p[1]) + p[2] * p[2];
    wgt[i] = mx / (l2 * sqrtf(l2));
}

// One block of one wave per row (blockIdx.x = the row) of a rows x n array: the row's inclusive prefix sums in
// k_meshlight_table's order — 64 entries per step, v += shfl_up(v, o) for o = 1 .. 32 (lanes below o keep theirs),
// S_i = carry + v, carry = the S of the previous chunk's last entry — then cdf_i = S_i / S_{n-1}, each lane dividing the
// sums it wrote itself; a row whose total is 0 gets cdf_i = 0 (never selected: its marginal step is 0).  total[row] =
// S_{n-1}.  The marginal is the same kernel over the one row of row totals.
__global__ void __launch_bounds__(64) k_env_table(int n, const float* __restrict__ in, float* __restrict__ cdf,
                                                  float* __restrict__ total) {
    const size_t row = (size_t)blockIdx.x * (size_t)n;
    const int l = (int)threadIdx.x;
    float carry = 0.f;
    for (int base = 0; base < n; base += 64) {
        const int i = base + l;
        float v = i < n ? in[row + i] : 0.f;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const float u = __shfl_up(v, o);
            if (l >= o) v += u;
        }
        const float S = carry + v;
        if (i < n) cdf[row + i] = S;
        const int rem = n - 1 - base;  // (the chunk's last entry: lane 63, or the lane of S_{n-1}; §3i)
        carry = __shfl(S, rem < 63 ? rem : 63);
    }
    const float A = carry;
    for (int i = l; i < n; i += 64) cdf[row + i] = A > 0.f ? cdf[row + i] / A : 0.f;
    if (l == 0) total[blockIdx.x] = A;
}

hipError_t launch_env_bake(hipStream_t st, const float* table, int W, int H, const float* rgb, float4* coef, float* wgt) {
    const int n = W * H;
    if (n <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_env_bake, dim3((n + kBlockThreads - 1) / kBlockThreads), dim3(kBlockThreads), 0, st, table, W,
                       H, rgb, coef, wgt);
    return hipGetLastError();
}

hipError_t launch_env_table(hipStream_t st, int W, int H, const float* wgt, float* cond, float* rowsum, float* marg,
                            float* total) {
    if (W <= 0 || H <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_env_table, dim3(H), dim3(64), 0, st, W, wgt, cond, rowsum);
    hipLaunchKernelGGL(k_env_table, dim3(1), dim3(64), 0, st, H, rowsum, marg, total);
    return hipGetLastError();
}

// ---- the miss stage
// Queue positions in order, a wave per 64 consecutive positions of one shard (entry e = chunk e / ns of shard e % ns,
// waves striding over the entries): hitPrim and the rays' (o, d) pairs are read coalesced in queue order; only the
// misses touch their slot's record (multi-level scenes: one 128-B record per slot, so a scattered slot is one line;
// single-leaf scenes: SoA fields with slots almost in queue order).  The D65 table is staged in LDS: the misses' hero
// wavelengths are spread over 360..830 nm.
__shared__ float g_d65[kSpecN];
__device__ __forceinline__ float env_d65(float lambda) {  // dense_query (spectrum.h:386-398) over the staged table
    const long off = (long)roundf(lambda) - 360;
    if (off < 0 || off >= kSpecN) return 0.f;
    return g_d65[off];
}
__device__ __forceinline__ int env_qlen(const QueueView& q, int j) {
    if (q.len) return q.len[j * kQStride];
    const int c = q.n - j * q.S;
    return c < 0 ? 0 : (c > q.S ? q.S : c);
}
__device__ __forceinline__ float4* env_recf(const RecView& r, int slot, int f) {
    return r.p + (size_t)f * r.fs + (size_t)slot * r.ss;
}
__device__ __forceinline__ void env_load8(const float4* q, size_t fs, float v[8]) {
    const float4 a = q[0], b = q[fs];
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

__global__ void __launch_bounds__(kBlockThreads) k_env_miss(const DevSpectra* __restrict__ sp, EnvMissIO io) {
    for (int i = threadIdx.x; i < kSpecN; i += blockDim.x) g_d65[i] = sp->D65[i];
    __syncthreads();
    const int lane = (int)(threadIdx.x & 63u);
    const int nw = (int)(gridDim.x * (blockDim.x >> 6)), w0 = (int)(blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    int mx = 0;
    for (int j = 0; j < io.q.ns; ++j) {
        const int l = env_qlen(io.q, j);
        mx = l > mx ? l : mx;
    }
    const int per_shard = (mx + 63) / 64, nent = io.q.ns * per_shard;
    const bool d0 = io.lean && io.depth == 0;  // lean depth 0: beta = 1 was never stored (the shade zeroed L)
    for (int e = w0; e < nent; e += nw) {
        const int j = e % io.q.ns, idx = (e / io.q.ns) * 64 + lane;
        if (idx >= env_qlen(io.q, j)) continue;
        const int k = j * io.q.S + idx;
        if (io.hitPrim[k] >= 0) continue;
        const float4 o4 = io.ray[2 * k], d4 = io.ray[2 * k + 1];
        const int slot = io.depth == 0 ? k : __float_as_int(o4.w);  // (as the shade kernels)
        const float prevPdf = env_recf(io.rec, slot, R_MISC)->y;
        if (prevPdf != 0.f && !io.mis) continue;  // a BSDF-sampled miss without MIS: NEE alone covers the map
        int texel;
        const float pdf = env_eval(io.env, v3(d4.x, d4.y, d4.z), texel);
        const float4 ec = env_tab(io.env).coef[texel];
        float lam[8], beta[8], L[8];
        env_load8(env_recf(io.rec, slot, R_LAM), io.rec.fs, lam);
        if (d0) {
#pragma unroll
            for (int i = 0; i < 8; ++i) beta[i] = 1.f;
        } else {
            env_load8(env_recf(io.rec, slot, R_BETA), io.rec.fs, beta);
        }
        float4* Lp = env_recf(io.rec, slot, R_L);
        env_load8(Lp, io.rec.fs, L);
        if (prevPdf == 0.f) {
#pragma unroll
            for (int i = 0; i < 8; ++i) L[i] += beta[i] * env_le(io.env.scale, ec, lam[i], env_d65(lam[i]));
        } else {
            const float wb = power_heuristic(prevPdf, pdf);
#pragma unroll
            for (int i = 0; i < 8; ++i) L[i] += (beta[i] * env_le(io.env.scale, ec, lam[i], env_d65(lam[i]))) * wb;
        }
        Lp[0] = make_float4(L[0], L[1], L[2], L[3]);
        Lp[io.rec.fs] = make_float4(L[4], L[5], L[6], L[7]);
    }
}

hipError_t launch_env_miss(hipStream_t st, int grid, const DevSpectra* sp, const EnvMissIO& io) {
    if (io.env.type != kLightEnv || io.q.ns < 1 || io.q.ns > kShards) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_env_miss, dim3(grid > 0 ? grid : 1), dim3(kBlockThreads), 0, st, sp, io);
    return hipGetLastError();
}

// ---- parity entries: env_sample / env_eval as the path kernels call them, one item per thread
__global__ void __launch_bounds__(kBlockThreads) k_env_sample(DevLight env, int n, const float* __restrict__ u,
                                                              float4* __restrict__ wi, int* __restrict__ texel) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const EnvSample s = env_sample(env, u[2 * i], u[2 * i + 1]);
    wi[i] = make_float4(s.wi.x, s.wi.y, s.wi.z, s.pdf);
    texel[i] = s.texel;
}
__global__ void __launch_bounds__(kBlockThreads) k_env_eval(DevLight env, int n, const float* __restrict__ dir,
                                                            int* __restrict__ texel, float* __restrict__ pdf) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int t;
    pdf[i] = env_eval(env, v3(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]), t);
    texel[i] = t;
}

hipError_t launch_env_sample(hipStream_t st, const DevLight& env, int n, const float* u, float4* wi, int* texel) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_env_sample, dim3((n + kBlockThreads - 1) / kBlockThreads), dim3(kBlockThreads), 0, st, env, n,
                       u, wi, texel);
    return hipGetLastError();
}
hipError_t launch_env_eval(hipStream_t st, const DevLight& env, int n, const float* dir, int* texel, float* pdf) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_env_eval, dim3((n + kBlockThreads - 1) / kBlockThreads), dim3(kBlockThreads), 0, st, env, n,
                       dir, texel, pdf);
    return hipGetLastError();
}

}  // namespace rtmi
