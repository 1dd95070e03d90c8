// Absorbing media inside glass: the per-depth Beer-Lambert stage of the general path integrator and the
// transmittance function of rt_medium.h on explicit inputs (parity entry point).  float32 in the order written, nothing
// fused beyond sigmoid_eval's own two fmaf (-ffp-contract=off), so tests/medium_reference.py restates every bit in numpy.
#include "rt_device.h"
#include "rt_medium.h"

namespace rtmi {

// ---- the absorb stage
// Queue positions in order, a wave per 64 consecutive positions of one shard, waves striding over the entries, exactly
// as k_env_miss: hitPrim is read coalesced in queue order; only the hits on a material with sigma > 0 read their ray
// pair, hit record and triangle.  The back-face hits among them are a minority of a wave's lanes (a fifth of the rays of
// §3n's report scene), and each costs eight double-precision exponentials: a wave therefore parks its back-face hits as
// (slot, len, material) in a list of its own in LDS and applies them 64 at a time, every lane busy, and the rest at its
// end.  Which lane multiplies a slot's beta does not change its bits, and a slot is met once per launch.  The applied
// items touch their slot through RecView (multi-level scenes: one 128-B record, so lambda and beta share a line;
// single-leaf scenes: SoA fields).  The per-material table (16 B per material) is staged in LDS when the scene has at
// most kLdsMedia materials; larger tables are read through the pointer.
static constexpr int kLdsMedia = 256;
static constexpr int kMedWaves = kBlockThreads / 64;
static constexpr int kMedPend = 128;  // a wave's list: below 64 parked items plus at most 64 new ones
__shared__ float4 g_med[kLdsMedia];
__shared__ int g_pslot[kMedWaves][kMedPend];
__shared__ float g_plen[kMedWaves][kMedPend];
__shared__ int g_pmid[kMedWaves][kMedPend];
__device__ __forceinline__ void med_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ int med_qlen(const QueueView& q, int j) {
    if (q.len) return q.len[j * kQStride];
    const int c = q.n - j * q.S;
    return c < 0 ? 0 : (c > q.S ? q.S : c);
}
__device__ __forceinline__ float4* med_recf(const RecView& r, int slot, int f) {
    return r.p + (size_t)f * r.fs + (size_t)slot * r.ss;
}
// beta of `slot` times the transmittance of a segment of length len in material mid's medium
__device__ __forceinline__ void med_apply(const MediumIO& io, bool lds, int slot, float len, int mid) {
    const float4 m = lds ? g_med[mid] : io.media[mid];
    const float4 la = *med_recf(io.rec, slot, R_LAM), lb = med_recf(io.rec, slot, R_LAM)[io.rec.fs];
    float4* bp = med_recf(io.rec, slot, R_BETA);
    float4 ba = bp[0], bb = bp[io.rec.fs];
    ba.x *= medium_transmittance(m.x, m.y, m.z, m.w, la.x, len);
    ba.y *= medium_transmittance(m.x, m.y, m.z, m.w, la.y, len);
    ba.z *= medium_transmittance(m.x, m.y, m.z, m.w, la.z, len);
    ba.w *= medium_transmittance(m.x, m.y, m.z, m.w, la.w, len);
    bb.x *= medium_transmittance(m.x, m.y, m.z, m.w, lb.x, len);
    bb.y *= medium_transmittance(m.x, m.y, m.z, m.w, lb.y, len);
    bb.z *= medium_transmittance(m.x, m.y, m.z, m.w, lb.z, len);
    bb.w *= medium_transmittance(m.x, m.y, m.z, m.w, lb.w, len);
    bp[0] = ba;
    bp[io.rec.fs] = bb;
}

__global__ void __launch_bounds__(kBlockThreads) k_medium_absorb(MediumIO io) {
    const bool lds = io.n_media <= kLdsMedia;
    if (lds) {
        for (int i = threadIdx.x; i < io.n_media; i += blockDim.x) g_med[i] = io.media[i];
        __syncthreads();
    }
    const int lane = (int)(threadIdx.x & 63u), wv = (int)(threadIdx.x >> 6);
    const int nw = (int)(gridDim.x * (blockDim.x >> 6)), w0 = (int)(blockIdx.x * (blockDim.x >> 6) + wv);
    int* const ps = g_pslot[wv];
    float* const pl = g_plen[wv];
    int* const pm = g_pmid[wv];
    int mx = 0;
    for (int j = 0; j < io.q.ns; ++j) {
        const int l = med_qlen(io.q, j);
        mx = l > mx ? l : mx;
    }
    const int per_shard = (mx + 63) / 64, nent = io.q.ns * per_shard;
    unsigned long long segs = 0;  // wave-uniform: the segments this wave attenuates
    int pend = 0;                 // wave-uniform: parked items, < 64 between iterations
    for (int e = w0; e < nent; e += nw) {
        const int j = e % io.q.ns, idx = (e / io.q.ns) * 64 + lane;
        bool back = false;
        int slot = 0, mid = 0;
        float len = 0.f;
        if (idx < med_qlen(io.q, j)) {
            const int k = j * io.q.S + idx;
            const int prim = io.hitPrim[k];
            if (prim >= 0) {
                mid = prim < io.n_tris ? io.triMaterial[prim] : io.shapes[prim - io.n_tris].material;
                float sigma = 0.f;
                if (mid >= 0 && mid < io.n_media) sigma = lds ? g_med[mid].w : io.media[mid].w;
                if (sigma > 0.f) {
                    const float4 o4 = io.ray[2 * k], d4 = io.ray[2 * k + 1], hb = io.hitB[k];
                    const V3 rdw = v3(d4.x, d4.y, d4.z);
                    // front, by the test of k_path_shade_full's surface block
                    if (prim < io.n_tris) {
                        const float4 P0 = io.triWorld[3 * prim], P1 = io.triWorld[3 * prim + 1], P2 = io.triWorld[3 * prim + 2];
                        const V3 p0 = v3(P0.x, P0.y, P0.z), p1 = v3(P1.x, P1.y, P1.z), p2 = v3(P2.x, P2.y, P2.z);
                        const V3 ng = vnorm(vcross(vsub(p0, p2), vsub(p1, p2)));
                        back = !(vdot(ng, vnorm(rdw)) < 0);
                    } else {
                        const DevShape& s = io.shapes[prim - io.n_tris];
                        const V3 rdo = vnorm(m4_dir(s.r2o, rdw));
                        const V3 no = shape_normal_obj(s, v3(hb.x, hb.y, hb.z));
                        back = vdot(no, rdo) > 0;  // flip: front = !flip
                    }
                    slot = __float_as_int(o4.w);  // (depth >= 1: as the shade kernels)
                    len = hb.w * sqrtf((d4.x * d4.x + d4.y * d4.y) + d4.z * d4.z);
                }
            }
        }
        const unsigned long long mask = __ballot(back);
        if (mask == 0) continue;  // (wave-uniform)
        if (back) {
            const int r = pend + __popcll(mask & ((1ull << lane) - 1ull));  // < 64 + 64
            ps[r] = slot;
            pl[r] = len;
            pm[r] = mid;
        }
        const int add = __popcll(mask);
        pend += add;
        segs += (unsigned long long)add;
        med_wave_sync();
        if (pend >= 64) {
            med_apply(io, lds, ps[lane], pl[lane], pm[lane]);
            const int rest = pend - 64;  // < 64: moved to the front
            int s = 0, m = 0;
            float l = 0.f;
            if (lane < rest) { s = ps[64 + lane]; l = pl[64 + lane]; m = pm[64 + lane]; }
            med_wave_sync();
            if (lane < rest) { ps[lane] = s; pl[lane] = l; pm[lane] = m; }
            med_wave_sync();
            pend = rest;
        }
    }
    if (lane < pend) med_apply(io, lds, ps[lane], pl[lane], pm[lane]);
    // per wave: one non-returning add into the wave's word of the spread counter (ctr_word, as the kernels' counter slots)
    if (lane == 0 && segs) atomicAdd(io.ctr + ctr_word(0, w0 & (kCtrSubs - 1)), segs);
}

hipError_t launch_medium_absorb(hipStream_t st, int grid, const MediumIO& io) {
    if (io.q.ns < 1 || io.q.ns > kShards || io.n_media < 1 || !io.media || !io.ctr || io.depth < 1)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_medium_absorb, dim3(grid > 0 ? grid : 1), dim3(kBlockThreads), 0, st, io);
    return hipGetLastError();
}

// ---- parity entry: medium_transmittance as the stage calls it, one item per thread
// item i: medium m[i] = (c0, c1, c2, sigma), lambda[8 i ..], len[i] -> out[8 i ..]
__global__ void __launch_bounds__(kBlockThreads) k_medium_eval(int n, const float4* __restrict__ m,
                                                               const float* __restrict__ lambda,
                                                               const float* __restrict__ len, float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float4 c = m[i];
    const float l = len[i];
#pragma unroll
    for (int k = 0; k < 8; ++k) out[8 * (size_t)i + k] = medium_transmittance(c.x, c.y, c.z, c.w, lambda[8 * (size_t)i + k], l);
}

hipError_t launch_medium_eval(hipStream_t st, int n, const float4* m, const float* lambda, const float* len, float* out) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_medium_eval, dim3((n + kBlockThreads - 1) / kBlockThreads), dim3(kBlockThreads), 0, st, n, m,
                       lambda, len, out);
    return hipGetLastError();
}

}  // namespace rtmi
