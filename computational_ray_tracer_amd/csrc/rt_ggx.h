// Rough reflector (RT_MAT_ROUGH): the isotropic GGX (Trowbridge-Reitz) microfacet reflector the host
// and the device share, one text for both sides (rt_ggx_eval / rt_ggx_sample on the host; k_path_shade_full<.., RGH>
// and the debug kernels of rt_rough.hip on the device).  Only + - * /, sqrtf and comparisons, float32 throughout,
// nothing fused (-ffp-contract=off on both sides), so tests/rough_reference.py restates every bit in numpy.
//
// Vectors are local to the frame (ss, tt, nrm) of the shading-side normal (ggx_frame: pbrt's CoordinateSystem, the
// frame cosine_bounce builds): v_local = (v.ss, v.tt, v.nrm), each a glm dot (x x + y y) + z z; wo = -rayd, mu_o = wo.z.
// With a = alpha, a2 = a a, in the order written:
//   D(h)      = 1 / ((pi a2) (t t)),  t = (h.x h.x + h.y h.y) / a2 + h.z h.z
//               (pbrt-v4's tan^2 form times cos^4; alpha^2 / (pi (h.z^2 (alpha^2 - 1) + 1)^2) for a unit h, without
//               that form's cancellation at alpha = 0.01, where h.z^2 (a2 - 1) + 1 loses 3 digits)
//   Lambda(w) = (sqrtf(1 + (a2 (1 - w.z w.z)) / (w.z w.z)) - 1) / 2,  G1(w) = 1 / (1 + Lambda(w))
//   G2        = 1 / ((1 + Lambda(wo)) + Lambda(wi))                      (height-correlated)
//   eval:  h = (wo + wi) (1 / sqrtf(|wo + wi|^2));  fcos = f mu_i / R = (D G2) / (4 wo.z);  pdf = (G1(wo) D) / (4 wo.z);
//          both 0 when wo.z <= 0 or wi.z <= 0
//   sample (Heitz's visible normals as pbrt-v4 TrowbridgeReitzDistribution::Sample_wm, the disk point (dx, dy) from
//          disk_concentric):  wh = normalize(a wo.x, a wo.y, wo.z);
//          T1 = wh.z < 0.99999f ? normalize(cross((0, 0, 1), wh)) : (1, 0, 0);  T2 = cross(wh, T1);
//          hh = sqrtf(1 - dx dx);  s = (1 + wh.z) / 2;  dy' = (1 - s) hh + s dy;
//          pz = sqrtf(max(0, (1 - dx dx) - dy' dy'));  nh = (T1 dx + T2 dy') + wh pz;
//          h = normalize(a nh.x, a nh.y, max(1e-6f, nh.z));  wi = (2 (wo.h)) h - wo;
//          no sample when wo.z <= 0 or wi.z <= 0; else pdf as eval's and wb = f mu_i / (R pdf) = G2 / G1(wo)
// normalize(v) = v (1 / sqrtf(v.v)), cross = glm's (a.y b.z - b.y a.z, ...), as rt_device.h vnorm / vcross.
#pragma once
#include <math.h>

#include "rt_cull.h"     // V3
#include "rt_texture.h"  // RT_HD

namespace rtmi {

static const float kGgxAlphaMin = 0.01f, kGgxAlphaMax = 1.0f;
RT_HD bool ggx_alpha_ok(float a) { return a >= kGgxAlphaMin && a <= kGgxAlphaMax; }  // (false for a NaN)

RT_HD float ggx_dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
RT_HD V3 ggx_norm(V3 v) {
    const float s = 1.0f / sqrtf(ggx_dot(v, v));
    return V3{v.x * s, v.y * s, v.z * s};
}
RT_HD V3 ggx_cross(V3 a, V3 b) { return V3{a.y * b.z - b.y * a.z, a.z * b.x - b.z * a.x, a.x * b.y - b.x * a.y}; }

// pbrt CoordinateSystem of the shading-side normal (cosine_bounce's frame, the same operations)
RT_HD void ggx_frame(V3 nrm, V3& ss, V3& tt) {
    const float sign = copysignf(1.0f, nrm.z);
    const float a = -1 / (sign + nrm.z);
    const float b = nrm.x * nrm.y * a;
    ss = V3{1 + sign * (nrm.x * nrm.x) * a, sign * b, -sign * nrm.x};
    tt = V3{b, sign + (nrm.y * nrm.y) * a, -nrm.y};
}
RT_HD V3 ggx_to_local(V3 v, V3 ss, V3 tt, V3 nrm) { return V3{ggx_dot(v, ss), ggx_dot(v, tt), ggx_dot(v, nrm)}; }
RT_HD V3 ggx_to_world(V3 l, V3 ss, V3 tt, V3 nrm) {
    return V3{(ss.x * l.x + tt.x * l.y) + nrm.x * l.z, (ss.y * l.x + tt.y * l.y) + nrm.y * l.z,
              (ss.z * l.x + tt.z * l.y) + nrm.z * l.z};
}

RT_HD float ggx_D(float a2, V3 h) {
    const float t = (h.x * h.x + h.y * h.y) / a2 + h.z * h.z;
    return 1.0f / ((3.14159265358979323846f * a2) * (t * t));
}
RT_HD float ggx_lambda(float a2, V3 w) {
    const float z2 = w.z * w.z;
    return (sqrtf(1.0f + (a2 * (1.0f - z2)) / z2) - 1.0f) / 2.0f;
}

// fcos = f mu_i / R(lambda) and the pdf of sampling wi from wo
RT_HD void ggx_eval(float alpha, V3 wo, V3 wi, float& fcos, float& pdf) {
    fcos = 0.f;
    pdf = 0.f;
    if (!(wo.z > 0.f) || !(wi.z > 0.f)) return;
    const float a2 = alpha * alpha;
    const V3 h = ggx_norm(V3{wo.x + wi.x, wo.y + wi.y, wo.z + wi.z});
    const float D = ggx_D(a2, h);
    const float lo = 1.0f + ggx_lambda(a2, wo);
    const float G2 = 1.0f / (lo + ggx_lambda(a2, wi)), G1 = 1.0f / lo;
    const float d4 = 4.0f * wo.z;
    fcos = (D * G2) / d4;
    pdf = (G1 * D) / d4;
}

// the visible normal h of wo (wo.z > 0) from a disk point: the half vector ggx_sample_disk reflects about and
// rt_roughglass.h reflects or refracts through
RT_HD V3 ggx_sample_h(float alpha, V3 wo, float dx, float dy) {
    const V3 wh = ggx_norm(V3{alpha * wo.x, alpha * wo.y, wo.z});
    V3 T1 = V3{1.f, 0.f, 0.f};
    if (wh.z < 0.99999f) T1 = ggx_norm(ggx_cross(V3{0.f, 0.f, 1.f}, wh));
    const V3 T2 = ggx_cross(wh, T1);
    const float c2 = 1.0f - dx * dx;
    const float hh = sqrtf(c2);
    const float s = (1.0f + wh.z) / 2.0f;
    dy = (1.0f - s) * hh + s * dy;
    float pz = c2 - dy * dy;
    pz = sqrtf(pz > 0.f ? pz : 0.f);
    const V3 nh = V3{(T1.x * dx + T2.x * dy) + wh.x * pz, (T1.y * dx + T2.y * dy) + wh.y * pz,
                     (T1.z * dx + T2.z * dy) + wh.z * pz};
    return ggx_norm(V3{alpha * nh.x, alpha * nh.y, nh.z > 1e-6f ? nh.z : 1e-6f});
}

// the bounce from a disk point: false = no bounce (wo or wi below the horizon; wi, wb, pdf are then 0)
RT_HD bool ggx_sample_disk(float alpha, V3 wo, float dx, float dy, V3& wi, float& wb, float& pdf) {
    wi = V3{0.f, 0.f, 0.f};
    wb = 0.f;
    pdf = 0.f;
    if (!(wo.z > 0.f)) return false;
    const float a2 = alpha * alpha;
    const V3 h = ggx_sample_h(alpha, wo, dx, dy);
    const float d2 = 2.0f * ggx_dot(wo, h);
    const V3 w = V3{d2 * h.x - wo.x, d2 * h.y - wo.y, d2 * h.z - wo.z};
    if (!(w.z > 0.f)) return false;
    const float D = ggx_D(a2, h);
    const float lo = 1.0f + ggx_lambda(a2, wo);
    const float G2 = 1.0f / (lo + ggx_lambda(a2, w)), G1 = 1.0f / lo;
    wi = w;
    pdf = (G1 * D) / (4.0f * wo.z);
    wb = G2 / G1;
    return true;
}

// ---- the variants a conductor vertex uses (RT_MAT_CONDUCTOR): the same fcos / pdf / wi / wb bits, and
// ch = the clamped cosine between wo and the half vector of (wo, wi), the argument of rt_fresnel.h fresnel_conductor.
// One definition for a light's wi and for the bounce's: h = normalize(wo + wi), ch = fminf(fmaxf(wo.h, 0), 1), so a
// direction has the same F whether NEE or the bounce found it (the two branches of an MIS pair).
RT_HD float ggx_cos_h(V3 wo, V3 wi) {
    const V3 h = ggx_norm(V3{wo.x + wi.x, wo.y + wi.y, wo.z + wi.z});
    return fminf(fmaxf(ggx_dot(wo, h), 0.f), 1.f);
}
RT_HD void ggx_eval_h(float alpha, V3 wo, V3 wi, float& fcos, float& pdf, float& ch) {
    ggx_eval(alpha, wo, wi, fcos, pdf);
    ch = ggx_cos_h(wo, wi);
}
RT_HD bool ggx_sample_disk_h(float alpha, V3 wo, float dx, float dy, V3& wi, float& wb, float& pdf, float& ch) {
    const bool ok = ggx_sample_disk(alpha, wo, dx, dy, wi, wb, pdf);
    ch = ok ? ggx_cos_h(wo, wi) : 0.f;
    return ok;
}

}  // namespace rtmi
