// Metal (RT_MAT_CONDUCTOR): the conductor Fresnel term and the dense table of measured optical constants
// the host and the device share, one text for both sides (rt_fresnel_conductor / rt_metal_nk on the host;
// k_path_shade_full<.., RGH = 2>, k_path_nee<.., RGH = 2> and the debug kernel of rt_conductor.hip on the device).  Only
// + - * /, sqrtf and comparisons, float32 in the order written, nothing fused (-ffp-contract=off on both sides), so
// tests/metal_reference.py restates every bit in numpy.
//
// Fresnel: unpolarised, exact, in real arithmetic, for a complex index n + i k seen from vacuum at the clamped cosine
// c = fminf(fmaxf(wo.h, 0), 1) of the angle between wo and the microfacet normal h:
//   c2 = c c;  s2 = 1 - c2;  t0 = (n n - k k) - s2;  ab = sqrtf(t0 t0 + (4 (n n)) (k k));  t1 = ab + c2
//   a  = sqrtf(fmaxf(0.5f (ab + t0), 0));  t2 = (2 a) c;  Rs = (t1 - t2) / (t1 + t2)
//   t3 = c2 ab + s2 s2;  t4 = t2 s2;  Rp = (Rs (t3 - t4)) / (t3 + t4);  F = 0.5f (Rp + Rs)
// (ab = a^2 + b^2 of the complex sqrt(eta^2 - sin^2) = a + i b; equal to 1/2 (|r_s|^2 + |r_p|^2) to 1e-14 in float64).
//
// Optical constants: NK[4][471] (n, k) pairs, entry j of metal m the piecewise-linear value of the metal's two measured
// tables (data/spectra_data.h metal_{ag,al,au,cu}_{eta,k}, 56 interleaved (lambda, value) pairs, 298.76-885.60 nm) at
// lambda = 360 + j, with the operations of piecewise_query (rt_device.h): the same interval search,
// t = (lambda - l[o]) / (l[o + 1] - l[o]), lerpf_ = (1 - t) v[o] + t v[o + 1].  Read at dense_query's index,
// (long)roundf(lambda) - 360, as D65 and the sensor bars are; (0, 0) outside 360-830.
#pragma once
#include <math.h>

#include "rt_texture.h"  // RT_HD

namespace rtmi {

static const int kMetals = 4;       // RT_METAL_AG, AL, AU, CU
static const int kMetalSpecN = 471;  // 360..830 nm (kSpecN)

// the metal id a conductor carries in sigmoid[0]: an integer 0..3 as a float (false for a NaN)
RT_HD bool metal_id_ok(float m) { return m == 0.f || m == 1.f || m == 2.f || m == 3.f; }

RT_HD float fresnel_conductor(float c, float n, float k) {
    c = fminf(fmaxf(c, 0.f), 1.f);
    const float c2 = c * c;
    const float s2 = 1.0f - c2;
    const float n2 = n * n, k2 = k * k;
    const float t0 = (n2 - k2) - s2;
    const float ab = sqrtf(t0 * t0 + (4.0f * n2) * k2);
    const float t1 = ab + c2;
    const float a = sqrtf(fmaxf(0.5f * (ab + t0), 0.f));
    const float t2 = (2.0f * a) * c;
    const float Rs = (t1 - t2) / (t1 + t2);
    const float t3 = c2 * ab + s2 * s2;
    const float t4 = t2 * s2;
    const float Rp = (Rs * (t3 - t4)) / (t3 + t4);
    return 0.5f * (Rp + Rs);
}

// The unpolarised dielectric Fresnel reflectance for a cosine already in [0, 1] and the relative index of that side: the
// one text of rt_device.h's fr_dielectric (smooth glass) and rt_roughglass.h's roughglass_F (rough glass)
RT_HD float fr_dielectric_pos(float cosi, float eta) {
    const float sin2i = 1 - cosi * cosi;
    const float sin2t = sin2i / (eta * eta);
    if (sin2t >= 1) return 1.f;
    const float x = 1 - sin2t;
    const float cost = sqrtf(x > 0.f ? x : 0.f);
    const float r_parl = (eta * cosi - cost) / (eta * cosi + cost);
    const float r_perp = (cosi - eta * cost) / (cosi + eta * cost);
    return (r_parl * r_parl + r_perp * r_perp) / 2;
}

// dense_query's index (rt_device.h): roundf is half away from zero, as std::lround
RT_HD long metal_index(float lambda) { return (long)roundf(lambda) - 360; }

// piecewise_query over one interleaved table s of n floats (n / 2 (lambda, value) pairs)
inline float metal_table_query(const float* s, int n, float lambda) {
    const long m = n / 2;
    if (m == 0 || lambda < s[0] || lambda > s[2 * (m - 1)]) return 0;
    long size = m - 2, first = 1;  // FindInterval
    while (size > 0) {
        const long half = size >> 1, middle = first + half;
        const bool r = s[2 * middle] <= lambda;
        first = r ? middle + 1 : first;
        size = r ? size - (half + 1) : half;
    }
    long o = first - 1;
    o = o < 0 ? 0 : (o > m - 2 ? m - 2 : o);
    const float t = (lambda - s[2 * o]) / (s[2 * (o + 1)] - s[2 * o]);
    return (1 - t) * s[2 * o + 1] + t * s[2 * (o + 1) + 1];
}

// one metal's dense table: nk[2 j] = n(360 + j), nk[2 j + 1] = k(360 + j), j < kMetalSpecN
inline void metal_nk_build(const float* eta, int eta_n, const float* kk, int k_n, float* nk) {
    for (int j = 0; j < kMetalSpecN; ++j) {
        nk[2 * j] = metal_table_query(eta, eta_n, (float)(360 + j));
        nk[2 * j + 1] = metal_table_query(kk, k_n, (float)(360 + j));
    }
}

}  // namespace rtmi
