// Temporal accumulation: the previous frame's accumulated film and moments, reprojected through the
// previous camera, rejected where the geometry disagrees and blended with the current frame by sample count.
//
//   k_temporal_accumulate  one thread per pixel, in the filter's 32 x 8 tiles: the pixel's mean first-hit point is
//                          projected into the previous frame's film space, the four bilinear taps around it are
//                          tested (sample count, hit count, normal, plane distance) and the survivors' means are
//                          blended with the current mean, alpha = n / n', n' = min(history + n, max_history).
//                          out = (mean n', n') and (m1 n', m2 n'): an ordinary film and moment film.
//   k_temporal_reproject   the guided estimate, once per frame: the same fetch, kept as a 16-B record
//                          (history count, per-sample moments) per pixel
//   k_temporal_error       once per iteration of a guided frame's session: the blend of the moments with the record and
//                          k_adaptive_error's block estimate on the result, one wave64 per 8x8 block
//
// Everything is float32 in the order written (the build's -ffp-contract=off; / is correctly rounded) with only
// + - * /, floorf, fmaxf, fminf and fabsf, so a numpy float32 restatement gives the same bits
// (tests/temporal_reference.py).
#include "rt_device.h"
#include "rt_internal.h"

namespace rtmi {

namespace {

constexpr int kBlock = kBlockThreads;
constexpr int kTX = 32, kTY = 8;  // pixels per thread block, as the filter's
static_assert(kTX * kTY == kBlock, "one thread per pixel of the tile");

// row r of M times (P, 1) in glm's order: (m0 x + m1 y) + (m2 z + m3 w), w = 1
__device__ __forceinline__ float row_mul(const float* M, int r, V3 P) {
    return (M[r] * P.x + M[4 + r] * P.y) + (M[8 + r] * P.z + M[12 + r]);
}

// The history of the pixel whose first hit is (P, n_p, z_p): false when it is disoccluded.
__device__ __forceinline__ bool fetch_history(const TemporalIO& io, V3 P, V3 n_p, float z_p, float& sw, float& sr,
                                              float& sg, float& sb, float& s1, float& s2, float& sn) {
    const int W = io.res_x, H = io.res_y;
    const float X = row_mul(io.M, 0, P), Y = row_mul(io.M, 1, P), Wc = row_mul(io.M, 3, P);
    if (!(Wc > 0.f)) return false;
    const float fu = X / Wc - 0.5f, fv = Y / Wc - 0.5f;
    // (a NaN fails every comparison: nothing out of range is converted to an integer)
    if (!(fu > -1.f && fu < (float)W && fv > -1.f && fv < (float)H)) return false;
    const float flx = floorf(fu), fly = floorf(fv);
    const int x0 = (int)flx, y0 = (int)fly;
    const float a = fu - flx, b = fv - fly;
    const float lim = io.plane_rel * z_p;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int xq = x0 + i, yq = y0 + j;
            if (xq < 0 || xq >= W || yq < 0 || yq >= H) continue;
            const int q = yq * W + xq;
            const float4 Fh = io.hfilm[q];
            if (Fh.w == 0.f) continue;
            const float4 Qh = io.hpos[q];
            if (Qh.w == 0.f) continue;
            const V3 Pq = v3(Qh.x / Qh.w, Qh.y / Qh.w, Qh.z / Qh.w);
            const float4 Gh = io.hfeat[q];
            const V3 nq = v3(Gh.x / io.kf, Gh.y / io.kf, Gh.z / io.kf);
            if (!(vdot(n_p, nq) >= io.normal_min)) continue;
            if (!(fabsf(vdot(n_p, vsub(Pq, P))) <= lim)) continue;
            const float w = (i ? a : 1.f - a) * (j ? b : 1.f - b);
            const float ns = Fh.w;
            const float2 Mh = io.hmom[q];
            sw = sw + w;
            sr = sr + w * (Fh.x / ns);
            sg = sg + w * (Fh.y / ns);
            sb = sb + w * (Fh.z / ns);
            s1 = s1 + w * (Mh.x / ns);
            s2 = s2 + w * (Mh.y / ns);
            sn = sn + w * ns;
        }
    return sw > 0.f;
}

__global__ void __launch_bounds__(kBlock) k_temporal_accumulate(TemporalIO io) {
    const int x = (int)blockIdx.x * kTX + (int)(threadIdx.x % kTX), y = (int)blockIdx.y * kTY + (int)(threadIdx.x / kTX);
    int cls = -1;  // (no early return: the whole wave takes part in the ballots below)
    if (x < io.res_x && y < io.res_y) {
        const int p = y * io.res_x + x;
        const float4 F = io.film[p];
        const float2 Mo = io.mom[p];
        const float n = F.w;
        float4 of = make_float4(0.f, 0.f, 0.f, 0.f);
        float2 om = make_float2(0.f, 0.f);
        if (n != 0.f) {
            of = F;
            om = Mo;
            const float4 Q = io.pos[p];
            if (Q.w == 0.f) {
                cls = T_BACKGROUND;
            } else {
                cls = T_DISOCCLUDED;
                if (io.hfilm) {
                    const float4 G = io.feat[p];
                    const V3 P = v3(Q.x / Q.w, Q.y / Q.w, Q.z / Q.w);
                    const V3 n_p = v3(G.x / io.kf, G.y / io.kf, G.z / io.kf);
                    float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, s1 = 0.f, s2 = 0.f, sn = 0.f;
                    if (fetch_history(io, P, n_p, G.w / io.kf, sw, sr, sg, sb, s1, s2, sn)) {
                        cls = T_REPROJECTED;
                        const float nh = sn / sw;
                        const float n2 = fmaxf(fminf(nh + n, io.max_history), n);
                        const float al = n / n2, be = 1.f - al;
                        of = make_float4((be * (sr / sw) + al * (F.x / n)) * n2, (be * (sg / sw) + al * (F.y / n)) * n2,
                                         (be * (sb / sw) + al * (F.z / n)) * n2, n2);
                        om = make_float2((be * (s1 / sw) + al * (Mo.x / n)) * n2, (be * (s2 / sw) + al * (Mo.y / n)) * n2);
                    }
                }
            }
        }
        io.out_film[p] = of;
        io.out_mom[p] = om;
    }
    // per wave: one ballot and one non-returning add per class into the wave's word of the spread counters
    const int wave = (int)((blockIdx.y * gridDim.x + blockIdx.x) * (kBlock >> 6) + (threadIdx.x >> 6));
    const int sub = wave & (kCtrSubs - 1);
    const bool first = (threadIdx.x & 63) == 0;
#pragma unroll
    for (int k = 0; k < T_NCLASSES; ++k) {
        const unsigned long long m = __ballot(cls == k);
        if (first && m) atomicAdd(io.ctr + ctr_word(k, sub), (unsigned long long)__popcll(m));
    }
}

// The guided estimate, first half: steps 2-6 of the stage for every pixel with a first hit, whatever
// the film holds.  rec = (nh, m1h, m2h, 0), the history's sample count and per-sample moments at the pixel; all 0
// where there is none (nh > 0 wherever there is one: every tap that counts has w ns > 0 or adds 0).
__global__ void __launch_bounds__(kBlock) k_temporal_reproject(TemporalIO io, float4* __restrict__ rec) {
    const int x = (int)blockIdx.x * kTX + (int)(threadIdx.x % kTX), y = (int)blockIdx.y * kTY + (int)(threadIdx.x / kTX);
    if (x >= io.res_x || y >= io.res_y) return;
    const int p = y * io.res_x + x;
    float4 R = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 Q = io.pos[p];
    if (Q.w != 0.f) {
        const float4 G = io.feat[p];
        const V3 P = v3(Q.x / Q.w, Q.y / Q.w, Q.z / Q.w);
        const V3 n_p = v3(G.x / io.kf, G.y / io.kf, G.z / io.kf);
        float sw = 0.f, sr = 0.f, sg = 0.f, sb = 0.f, s1 = 0.f, s2 = 0.f, sn = 0.f;
        if (fetch_history(io, P, n_p, G.w / io.kf, sw, sr, sg, sb, s1, s2, sn)) R = make_float4(sn / sw, s1 / sw, s2 / sw, 0.f);
    }
    rec[p] = R;
}

// Second half, once per iteration: one wave64 per image-aligned 8x8 block with k_adaptive_error's lane mapping.  Step 7
// of the stage on the moments alone, then k_adaptive_error's arithmetic on the result: the bits of k_temporal_accumulate
// followed by k_adaptive_error.  rec null: no history.
__global__ void __launch_bounds__(kBlock) k_temporal_error(AdaptiveIO io, const float4* __restrict__ rec,
                                                           float max_history, int nbx, int nblocks) {
    const int b = (int)blockIdx.x * (kBlock / 64) + (int)(threadIdx.x >> 6);  // wave-uniform
    if (b >= nblocks) return;
    const int by = b / nbx, bx = b - by * nbx;
    const int l = (int)(threadIdx.x & 63u);
    const int x = bx * 8 + (l & 7), y = by * 8 + (l >> 3);
    float sem = 0.f, mean = 0.f;
    if (x < io.res_x && y < io.res_y) {
        const int p = y * io.res_x + x;
        const float n = reinterpret_cast<const float*>(io.film)[4 * (size_t)p + 3];
        if (n != 0.f) {
            const float2 Mo = io.mom[p];
            float n2 = n, s = Mo.x, q = Mo.y;
            const float4 R = rec ? rec[p] : make_float4(0.f, 0.f, 0.f, 0.f);
            if (R.x != 0.f) {
                n2 = fmaxf(fminf(R.x + n, max_history), n);
                const float al = n / n2, be = 1.f - al;
                s = (be * R.y + al * (Mo.x / n)) * n2;
                q = (be * R.z + al * (Mo.y / n)) * n2;
            }
            if (n2 >= 2.f) {
                mean = s / n2;
                const float d = fmaxf(q - s * mean, 0.f);
                sem = sqrtf((d / (n2 - 1.f)) / n2);
            }
        }
    }
    float S = sem, M = mean;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        S += __shfl_xor(S, o);
        M += __shfl_xor(M, o);
    }
    if (l == 0) {
        const float E = S / (M + io.abs_floor);
        io.block_error[b] = E;
        io.converged[b] = E <= io.rel_error ? 1 : 0;
    }
}

}  // namespace

hipError_t launch_temporal_reproject(hipStream_t st, const TemporalIO& io, float4* rec) {
    const dim3 grid((io.res_x + kTX - 1) / kTX, (io.res_y + kTY - 1) / kTY);
    hipLaunchKernelGGL(k_temporal_reproject, grid, dim3(kBlock), 0, st, io, rec);
    return hipGetLastError();
}

hipError_t launch_temporal_error(hipStream_t st, const AdaptiveIO& io, const float4* rec, float max_history) {
    const int nbx = (io.res_x + 7) / 8, nblocks = nbx * ((io.res_y + 7) / 8), waves = kBlock / 64;
    hipLaunchKernelGGL(k_temporal_error, dim3((nblocks + waves - 1) / waves), dim3(kBlock), 0, st, io, rec, max_history,
                       nbx, nblocks);
    return hipGetLastError();
}

hipError_t launch_temporal_accumulate(hipStream_t st, const TemporalIO& io) {
    const dim3 grid((io.res_x + kTX - 1) / kTX, (io.res_y + kTY - 1) / kTY);
    hipLaunchKernelGGL(k_temporal_accumulate, grid, dim3(kBlock), 0, st, io);
    return hipGetLastError();
}

}  // namespace rtmi
