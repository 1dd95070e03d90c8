// Specular-chain guides: the feature and position films of the surface a pixel shows at the end of
// its chain of perfect mirrors and refractions, instead of the first surface.
//
//   k_chain_level   one launch per chain level over that level's ray queue (level 0: the camera rays and their first
//                   hits).  Per item the surface block of k_path_shade_full; then the chain stops (emitter, diffuse,
//                   chain_depth continuations traced, or a miss) and the item's result goes to res[slot], or the ray
//                   the shade kernel would spawn (mirror: the reflection; dielectric: the refraction whenever it
//                   exists, the reflection on total internal reflection) is appended to the next level's queue with a
//                   wave ballot and one atomic per wave.  The bounce rays' k_trace_closest traces that queue.
//   k_chain_film    one thread per owned pixel: adds the results of its samples in increasing index order.
//
// Chain state: the ray carries its slot, the number of reflections so far and the length D of the chain up to its
// origin in the two w components of the queue entry; the reflection normals (at most kChainMax) live per slot in
// global arrays that only a reflection writes and only the chain's end reads.  The state has to outlive a kernel
// launch per level, so it cannot stay in LDS or registers; a chain without a reflection touches none of it.
//
// k_chain_level<true> (RT_CHAIN_CURVED) replaces the chain's length D = sum of the segments by the curvature-aware
// virtual distance: a continuing item also writes one record (c_c, c_f, mu, kappa) and its segment length to per-slot
// global arrays, and the chain's end carries the image distance backwards over them (chain_curved_distance).
// k_chain_level<false> is the kernel without any of it.
//
// Everything is float32 in the order written (the build's -ffp-contract=off), so a numpy float32 restatement gives
// the same bits (tests/chain_reference.py; with the flag and on analytic shapes tests/chain_curved_reference.py).
#include "rt_device.h"
#include "rt_internal.h"

namespace rtmi {

namespace {

constexpr int kBlock = kBlockThreads;
constexpr int kSlotMask = (1 << kChainSlotBits) - 1;

RT_DEV V3 xyz(float4 a) { return v3(a.x, a.y, a.z); }

// The queue helpers of rt_kernels.hip, restated here (that file's kernels are pinned to their resource report, line
// numbers included, so nothing moves out of it).
RT_DEV int lane_id() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
// Append the `pred` lanes of a wave to a queue: one atomicAdd per wave, slots in lane order.
// Every lane of the wave must call it.
RT_DEV int wave_append(int* counter, bool pred) {
    const uint64_t mask = __ballot(pred);
    if (mask == 0) return -1;
    const int leader = __ffsll((unsigned long long)mask) - 1;
    int base = 0;
    if (lane_id() == leader) base = atomicAdd(counter, __popcll(mask));
    base = __shfl(base, leader);
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
    return pred ? base + rank : -1;
}
RT_DEV int q_len(const QueueView& q, int j) {
    if (q.len) return q.len[j * kQStride];
    const int c = q.n - j * q.S;
    return c < 0 ? 0 : (c > q.S ? q.S : c);
}

// The curvature-aware virtual distance of a chain of K continuation surfaces that ends after a segment of length tK
// (DESIGN.md §3e "curved"): the surfaces' records, last first, carry the tangential and the sagittal image distance
// back to surface 0.  Dsum: the plain sum, returned for a chain of planar reflections and when an image is not virtual.
RT_DEV float chain_curved_distance(const ChainIO& io, int slot, int K, float tK, float Dsum) {
    const float4 L = io.seg[slot];  // t_0 .. t_3
    float sT = 0.f, sS = 0.f, tn = tK;
    bool flat = true, ok = true;
    for (int k = K - 1; k >= 0; --k) {
        const float4 r = io.rec[k][slot];  // (c_c, c_f, mu, kappa)
        const float uT = tn + sT, uS = tn + sS;
        if (r.z == 0.f && r.w == 0.f) {
            sT = uT;
            sS = uS;
        } else {
            flat = false;
            float aT, aS;
            if (r.z == 0.f) {
                const float k2 = 2.0f * r.w;
                aT = 1.0f / uT + k2 / r.x;
                aS = 1.0f / uS + k2 * r.x;
            } else {
                const float gk = (r.x - r.z * r.y) * r.w;
                aT = (((r.z * r.y) * r.y) / uT + gk) / (r.x * r.x);
                aS = r.z / uS + gk;
            }
            if (!(aT > 0.f) || !(aS > 0.f)) ok = false;
            sT = 1.0f / aT;
            sS = 1.0f / aS;
        }
        tn = k == 3 ? L.w : (k == 2 ? L.z : (k == 1 ? L.y : L.x));  // t_k
    }
    if (flat || !ok) return Dsum;
    const float DT = tn + sT, DS = tn + sS;
    return ((2.0f * DT) * DS) / (DT + DS);
}

template <bool CURVED>
__global__ void __launch_bounds__(kBlock) k_chain_level(DevScene sc, ChainIO io) {
    // 64-item chunks of the shards (a shard stride is a multiple of 64), chunk c = shard c / cps: a wave's items are
    // of one shard, so its continuations take one append on that shard's length
    const int cps = io.q.S >> 6, nchunks = io.q.ns * cps;
    const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6), nwaves = (int)((gridDim.x * blockDim.x) >> 6);
    for (int c = wave; c < nchunks; c += nwaves) {
        const int j = c / cps, idx = ((c - j * cps) << 6) + lane_id();
        const int len = q_len(io.q, j);
        if (((c - j * cps) << 6) >= len) continue;  // (wave-uniform)
        const int p = j * io.q.S + idx;
        bool go = false;
        float4 nO = make_float4(0.f, 0.f, 0.f, 0.f), nD = nO;
        if (idx < len) {
            const float4 o4 = io.ray[2 * p], d4 = io.ray[2 * p + 1];
            int slot = p, m = 0;  // m: reflections so far = entries of N
            if (io.level > 0) {
                slot = __float_as_int(o4.w) & kSlotMask;
                m = __float_as_int(o4.w) >> kChainSlotBits;
            }
            const int prim = io.hitPrim[p];
            if (prim < 0) {
                io.res[slot] = make_float4(0.f, 0.f, 0.f, -1.f);
            } else {
                const float4 hb = io.hitB[p];
                const float D = io.level > 0 ? d4.w + hb.w : hb.w;
                const V3 rdw = xyz(d4), rayd = vnorm(rdw);
                // ---- surface (k_path_shade_full)
                V3 pt, nrm, nout;
                int mid;
                float kap = 0.f;  // (CURVED) the surface's signed curvature
                if (prim < sc.n_tris) {
                    const V3 p0 = xyz(sc.triWorld[3 * prim]), p1 = xyz(sc.triWorld[3 * prim + 1]),
                             p2 = xyz(sc.triWorld[3 * prim + 2]);
                    const V3 ng = vnorm(vcross(vsub(p0, p2), vsub(p1, p2)));
                    pt = vadd(vadd(vmul(p0, hb.x), vmul(p1, hb.y)), vmul(p2, hb.z));
                    nout = ng;
                    nrm = ng;
                    if (vdot(nrm, rayd) > 0) nrm = v3(-ng.x, -ng.y, -ng.z);
                    mid = sc.triMaterial[prim];
                } else {
                    const DevShape& s = sc.shapes[prim - sc.n_tris];
                    const V3 rdo = vnorm(m4_dir(s.r2o, rdw));
                    const V3 ph = xyz(hb);
                    V3 no = shape_normal_obj(s, ph);
                    const bool flip = vdot(no, rdo) > 0;
                    if (flip) no = v3(-no.x, -no.y, -no.z);
                    const V3 nw = vnorm(m3_mul(s.n2r, no));
                    pt = m4_point(s.o2r, ph);
                    nrm = nw;
                    nout = flip ? v3(-nw.x, -nw.y, -nw.z) : nw;
                    mid = s.material;
                    if constexpr (CURVED) {
                        const float km = io.kappa[prim - sc.n_tris];
                        kap = flip ? -km : km;
                    }
                }
                const DevMaterial mt = sc.materials[mid];
                // the emitter check comes first, as in the shade kernel
                if (!(mt.emit > 0) && (mt.type == 1 || mt.type == 2) && io.level < io.depth) {
                    const float off = 1e-4f * (1.0f + max3f(fabsf(pt.x), fabsf(pt.y), fabsf(pt.z)));
                    bool refl = mt.type == 1;
                    V3 po, wi;
                    float4 rec = make_float4(-vdot(rayd, nrm), 0.f, 0.f, kap);
                    if (!refl) {  // smooth dielectric: the refraction whenever it exists (no sampler draw)
                        const float eta = mt.eta != 0 ? mt.eta : io.eta_bk7;
                        V3 wt;
                        float etap;
                        if (refract_dir(v3(-rayd.x, -rayd.y, -rayd.z), nout, eta, etap, wt)) {
                            po = vsub(pt, vmul(nrm, off));
                            wi = wt;
                            if constexpr (CURVED) {
                                rec.y = -vdot(wt, nrm);
                                rec.z = etap;
                            }
                        } else {
                            refl = true;
                        }
                    }
                    if (refl) {  // N[m] = nrm (m <= level < kChainMax)
                        po = vadd(pt, vmul(nrm, off));
                        wi = reflect_dir(rayd, nrm);
                        float4* const dst = m == 0 ? io.n[0] : (m == 1 ? io.n[1] : (m == 2 ? io.n[2] : io.res));
                        dst[slot] = make_float4(nrm.x, nrm.y, nrm.z, 0.f);
                        m += 1;
                    }
                    if constexpr (CURVED) {  // surface `level` of the chain (level < depth <= kChainMax)
                        io.rec[io.level][slot] = rec;
                        reinterpret_cast<float*>(io.seg)[4 * (size_t)slot + io.level] = hb.w;
                    }
                    go = true;
                    nO = make_float4(po.x, po.y, po.z, __int_as_float(slot | (m << kChainSlotBits)));
                    nD = make_float4(wi.x, wi.y, wi.z, D);
                } else {  // the chain's end: the final normal mirrored back through N, last entry first
                    V3 v = nrm;
                    if (m > 3) v = reflect_dir(v, xyz(io.res[slot]));
                    if (m > 2) v = reflect_dir(v, xyz(io.n[2][slot]));
                    if (m > 1) v = reflect_dir(v, xyz(io.n[1][slot]));
                    if (m > 0) v = reflect_dir(v, xyz(io.n[0][slot]));
                    float Dv = D;
                    if constexpr (CURVED) {
                        if (io.level > 0) Dv = chain_curved_distance(io, slot, io.level, hb.w, D);
                    }
                    io.res[slot] = make_float4(v.x, v.y, v.z, Dv);
                }
            }
        }
        const int pn = wave_append(io.nlen + j * kQStride, go) + j * io.q.S;
        if (go) {
            io.nray[2 * pn] = nO;
            io.nray[2 * pn + 1] = nD;
        }
    }
}

template <bool POS>
__global__ void __launch_bounds__(kBlock) k_chain_film(ChainFilmIO io) {
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < io.n_pixels; j += gridDim.x * blockDim.x) {
        const int pixel = io.work_pixels[j];
        float4 f = io.feat[pixel];
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (POS) q = io.pos[pixel];
        for (int i = 0; i < io.n_index; ++i) {
            const int s = i * io.n_pixels + j;
            const float4 r = io.res[s];
            if (r.w < 0.f) continue;  // the chain ended in a miss
            f.x += r.x;
            f.y += r.y;
            f.z += r.z;
            f.w += r.w;
            if constexpr (POS) {
                const float4 o4 = io.ray[2 * (size_t)s], d4 = io.ray[2 * (size_t)s + 1];
                q.x += o4.x + r.w * d4.x;
                q.y += o4.y + r.w * d4.y;
                q.z += o4.z + r.w * d4.z;
                q.w += 1.f;
            }
        }
        io.feat[pixel] = f;
        if constexpr (POS) io.pos[pixel] = q;
    }
}

}  // namespace

hipError_t launch_chain_level(hipStream_t st, int grid, const DevScene& sc, const ChainIO& io) {
    if (io.level < 0 || io.level > io.depth || io.depth > kChainMax || (io.q.S & 63) || io.q.ns < 1)
        return hipErrorInvalidValue;
    // one wave per 64-item chunk: of the dense queue's items (level 0), of a resident grid's share otherwise (the
    // length is on the device)
    const long long chunks = io.q.len ? (long long)io.q.ns * (io.q.S >> 6) : ((long long)io.q.n + 63) / 64 + io.q.ns;
    long long gb = (chunks * 64 + kBlock - 1) / kBlock;
    if (grid > 0 && gb > grid) gb = grid;
    const dim3 g((unsigned)(gb < 1 ? 1 : gb)), blk(kBlock);
    if (io.curved) {
        if (!io.kappa || !io.seg || !io.rec[0] || !io.rec[1] || !io.rec[2] || !io.rec[3]) return hipErrorInvalidValue;
        hipLaunchKernelGGL(k_chain_level<true>, g, blk, 0, st, sc, io);
    } else {
        hipLaunchKernelGGL(k_chain_level<false>, g, blk, 0, st, sc, io);
    }
    return hipGetLastError();
}

hipError_t launch_chain_film(hipStream_t st, const ChainFilmIO& io) {
    const dim3 grid((io.n_pixels + kBlock - 1) / kBlock), block(kBlock);
    if (io.pos) hipLaunchKernelGGL(k_chain_film<true>, grid, block, 0, st, io);
    else hipLaunchKernelGGL(k_chain_film<false>, grid, block, 0, st, io);
    return hipGetLastError();
}

}  // namespace rtmi
