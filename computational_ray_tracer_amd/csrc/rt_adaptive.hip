// Adaptive sampling: the per-block error estimate and the stable compaction of the active pixel list.
//
//   k_adaptive_error    one wave64 per image-aligned 8x8 block: standard error of the mean and mean per pixel from
//                       the moment film, both summed over the block by the xor butterfly, E = S / (M + abs_floor)
//   k_adaptive_count    per wave of the active list: how many of its 64 pixels lie in a block that is not converged
//   k_adaptive_scan     exclusive scan of the wave counts (one thread block), the total = the new list's length; it
//                       also counts the blocks that are not converged
//   k_adaptive_scatter  every kept pixel to scan[wave] + its rank in the wave's ballot: the list keeps its order
//
// Everything is float32 in the order written (the build's -ffp-contract=off; / and sqrtf are correctly rounded), so
// a numpy float32 restatement gives the same bits (tests/test_gpu_adaptive.py).
#include "rt_internal.h"

namespace rtmi {

namespace {

constexpr int kBlock = kBlockThreads;
constexpr int kWaves = kBlock / 64;

__device__ __forceinline__ int lane() { return (int)(threadIdx.x & 63u); }

__global__ void __launch_bounds__(kBlock) k_adaptive_error(AdaptiveIO io, int nbx, int nblocks) {
    const int b = (int)blockIdx.x * kWaves + (int)(threadIdx.x >> 6);  // wave-uniform
    if (b >= nblocks) return;
    const int by = b / nbx, bx = b - by * nbx;
    const int l = lane();
    const int x = bx * 8 + (l & 7), y = by * 8 + (l >> 3);
    float sem = 0.f, mean = 0.f;
    if (x < io.res_x && y < io.res_y) {
        const int p = y * io.res_x + x;
        const float n = io.film[p].w;
        if (n >= 2.f) {
            const float2 m = io.mom[p];
            mean = m.x / n;
            const float d = fmaxf(m.y - m.x * mean, 0.f);
            sem = sqrtf((d / (n - 1.f)) / n);
        }
    }
    float S = sem, M = mean;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {  // (count_add's order: every lane ends with the same bits)
        S += __shfl_xor(S, o);
        M += __shfl_xor(M, o);
    }
    if (l == 0) {
        const float E = S / (M + io.abs_floor);
        const int conv = E <= io.rel_error ? 1 : 0;
        io.block_error[b] = E;
        io.converged[b] = conv;
    }
}

// pixel in[k] stays active: its block has not converged
__device__ __forceinline__ bool keeps(const int* __restrict__ in, int n, int k, const int* __restrict__ converged,
                                      int res_x, int nbx) {
    if (k >= n) return false;
    const int p = in[k];
    const int y = p / res_x, x = p - y * res_x;
    return converged[(y >> 3) * nbx + (x >> 3)] == 0;
}

__global__ void __launch_bounds__(kBlock) k_adaptive_count(const int* __restrict__ in, int n,
                                                           const int* __restrict__ converged, int res_x, int nbx,
                                                           int* __restrict__ wave_count) {
    const int k = (int)blockIdx.x * kBlock + (int)threadIdx.x;
    const unsigned long long mask = __ballot(keeps(in, n, k, converged, res_x, nbx));
    if (lane() == 0 && k < n) wave_count[k >> 6] = __popcll(mask);
}

// wave_offset[i] = sum of wave_count[0, i); totals[0] = the whole sum.  One thread block walks the counts kBlock at a
// time: an inclusive shuffle scan per wave, the waves' totals through LDS, the running carry in a register.  The same
// block then counts the blocks that are not converged into totals[1] (one atomic per such block on one word, from the
// error kernel, serialised: 302 us instead of 14 us per launch at 1080p).
__global__ void __launch_bounds__(kBlock) k_adaptive_scan(const int* __restrict__ wave_count, int nw,
                                                          int* __restrict__ wave_offset,
                                                          const int* __restrict__ converged, int nblocks,
                                                          int* __restrict__ totals) {
    __shared__ int wsum[kWaves];
    const int t = (int)threadIdx.x, l = lane(), w = t >> 6;
    int carry = 0;
    for (int base = 0; base < nw; base += kBlock) {
        const int i = base + t;
        const int v = i < nw ? wave_count[i] : 0;
        int inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(inc, o);
            if (l >= o) inc += u;
        }
        if (l == 63) wsum[w] = inc;
        __syncthreads();
        int before = 0, all = 0;
#pragma unroll
        for (int j = 0; j < kWaves; ++j) {
            const int s = wsum[j];
            if (j < w) before += s;
            all += s;
        }
        if (i < nw) wave_offset[i] = carry + before + inc - v;
        carry += all;
        __syncthreads();  // wsum is rewritten by the next round
    }
    int open = 0;
    for (int b = t; b < nblocks; b += kBlock) open += converged[b] == 0;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) open += __shfl_xor(open, o);
    if (l == 0) wsum[w] = open;
    __syncthreads();
    if (t == 0) {
        int all = 0;
#pragma unroll
        for (int j = 0; j < kWaves; ++j) all += wsum[j];
        totals[0] = carry;
        totals[1] = all;
    }
}

__global__ void __launch_bounds__(kBlock) k_adaptive_scatter(const int* __restrict__ in, int n,
                                                             const int* __restrict__ converged, int res_x, int nbx,
                                                             const int* __restrict__ wave_offset,
                                                             int* __restrict__ out) {
    const int k = (int)blockIdx.x * kBlock + (int)threadIdx.x;
    const bool keep = keeps(in, n, k, converged, res_x, nbx);
    const unsigned long long mask = __ballot(keep);
    if (keep) {  // (k < n; the rank is < the wave's count, so the position is < the scan's total <= n)
        const int rank = __popcll(mask & ((1ull << lane()) - 1ull));
        out[wave_offset[k >> 6] + rank] = in[k];
    }
}

}  // namespace

hipError_t launch_adaptive_error(hipStream_t st, const AdaptiveIO& io) {
    const int nbx = (io.res_x + 7) / 8, nby = (io.res_y + 7) / 8, nblocks = nbx * nby;
    hipLaunchKernelGGL(k_adaptive_error, dim3((nblocks + kWaves - 1) / kWaves), dim3(kBlock), 0, st, io, nbx, nblocks);
    return hipGetLastError();
}

hipError_t launch_adaptive_compact(hipStream_t st, const AdaptiveIO& io, const int* in, int n, int* out,
                                   int* wave_count, int* wave_offset) {
    const int nbx = (io.res_x + 7) / 8, nblocks = nbx * ((io.res_y + 7) / 8);
    if (n < 0) n = 0;
    const dim3 grid((n + kBlock - 1) / kBlock), block(kBlock);
    if (n) hipLaunchKernelGGL(k_adaptive_count, grid, block, 0, st, in, n, io.converged, io.res_x, nbx, wave_count);
    hipLaunchKernelGGL(k_adaptive_scan, dim3(1), block, 0, st, wave_count, adaptive_waves(n), wave_offset, io.converged,
                       nblocks, io.totals);
    if (n) hipLaunchKernelGGL(k_adaptive_scatter, grid, block, 0, st, in, n, io.converged, io.res_x, nbx, wave_offset, out);
    return hipGetLastError();
}

}  // namespace rtmi
