// Rough glass (RT_MAT_ROUGH_DIELECTRIC): the non-absorbing rough dielectric interface of Walter et al.
// 2007 with §3k's isotropic GGX, one text for the host and the device (rt_roughglass_eval / rt_roughglass_sample on the
// host; k_path_shade_full<.., RGH = 3> and the debug kernels of rt_roughglass.hip on the device).  Only + - * /, sqrtf
// and comparisons, float32 in the order written, nothing fused (-ffp-contract=off on both sides), so
// tests/roughglass_reference.py restates every bit in numpy.
//
// Vectors are local to ggx_frame of the shading-side normal, so wo.z > 0.  er is the relative index seen from the
// shading side: er = front ? eta : 1 / eta.  D, Lambda, G1, G2, the visible normal h and ggx_cos_h are rt_ggx.h's.
//   F(c, er):  fr_dielectric's operations (rt_fresnel.h fr_dielectric_pos) at c = fminf(fmaxf(c, 0), 1):
//              s2i = 1 - c c;  s2t = s2i / (er er);  1 when s2t >= 1 (total internal reflection);
//              ct = sqrtf(max(1 - s2t, 0));
//              rp = (er c - ct) / (er c + ct);  rs = (c - er ct) / (c + er ct);  F = (rp rp + rs rs) / 2
//   eval (the reflection side; a light below the shading side is never sampled):  with ggx_eval's fcos and pdf,
//              ch = ggx_cos_h(wo, wi):  fcosF = F(ch, er) fcos;  pdfF = F(ch, er) pdf;  both 0 when wi.z <= 0
//   sample (disk point (dx, dy), one more uniform u):  h = ggx_sample_h;  c = wo.h;  F = F(c, er);
//     u < F:  wi = (2 c) h - wo;  none when wi.z <= 0;  w = G2(wo, wi) / G1(wo);  prevPdf = F ((G1 D) / (4 wo.z))
//     else:   refract_dir's operations through h:  s2t = max(1 - c c, 0) / (er er) (none when >= 1);
//             ct = sqrtf(max(1 - s2t, 0));  wt = -wo / er + (c / er - ct) h;  none unless wt.z < 0;
//             w = (G2(wo, wt) / G1(wo)) / (er er), Lambda(wt) from wt.z^2;  prevPdf = 0
// Both weights are f |mu_i| / pdf of the whole BSDF under "visible normal, then Fresnel choice"; F cancels in each; the
// 1 / er^2 is the radiance scaling the smooth glass applies as beta /= etap^2.
#pragma once
#include <math.h>

#include "rt_fresnel.h"  // fr_dielectric_pos
#include "rt_ggx.h"

namespace rtmi {

// the index of a rough-glass material: finite and above 1 (false for a NaN, an infinity, 0 = dispersive BK7)
RT_HD bool roughglass_eta_ok(float eta) { return eta > 1.0f && eta < 3.0e38f; }

RT_HD float roughglass_F(float c, float er) { return fr_dielectric_pos(fminf(fmaxf(c, 0.f), 1.f), er); }

RT_HD void roughglass_eval(float alpha, float er, V3 wo, V3 wi, float& fcosF, float& pdfF) {
    fcosF = 0.f;
    pdfF = 0.f;
    if (!(wo.z > 0.f) || !(wi.z > 0.f)) return;
    float fc, pdf;
    ggx_eval(alpha, wo, wi, fc, pdf);
    const float F = roughglass_F(ggx_cos_h(wo, wi), er);
    fcosF = F * fc;
    pdfF = F * pdf;
}

// the bounce: 0 = none (wi, w, pdf are then 0), 1 = reflected, 2 = transmitted (wi.z < 0, pdf = 0)
RT_HD int roughglass_sample(float alpha, float er, V3 wo, float dx, float dy, float u, V3& wi, float& w, float& pdf) {
    wi = V3{0.f, 0.f, 0.f};
    w = 0.f;
    pdf = 0.f;
    if (!(wo.z > 0.f)) return 0;
    const float a2 = alpha * alpha;
    const V3 h = ggx_sample_h(alpha, wo, dx, dy);
    const float c = ggx_dot(wo, h);
    const float F = roughglass_F(c, er);
    const float lo = 1.0f + ggx_lambda(a2, wo);
    const float G1 = 1.0f / lo;
    if (u < F) {
        const float d2 = 2.0f * c;
        const V3 wr = V3{d2 * h.x - wo.x, d2 * h.y - wo.y, d2 * h.z - wo.z};
        if (!(wr.z > 0.f)) return 0;
        const float D = ggx_D(a2, h);
        const float G2 = 1.0f / (lo + ggx_lambda(a2, wr));
        wi = wr;
        w = G2 / G1;
        pdf = F * ((G1 * D) / (4.0f * wo.z));
        return 1;
    }
    const float x = 1 - c * c;
    const float sin2i = x > 0.f ? x : 0.f;
    const float sin2t = sin2i / (er * er);
    if (sin2t >= 1) return 0;
    const float y = 1 - sin2t;
    const float cost = sqrtf(y > 0.f ? y : 0.f);
    const float k = c / er - cost;
    const V3 wt = V3{-wo.x / er + h.x * k, -wo.y / er + h.y * k, -wo.z / er + h.z * k};
    if (!(wt.z < 0.f)) return 0;
    const float G2 = 1.0f / (lo + ggx_lambda(a2, wt));
    wi = wt;
    w = (G2 / G1) / (er * er);
    return 2;
}

}  // namespace rtmi
