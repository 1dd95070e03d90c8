// Image environment light: the direction <-> texel mapping the host and the device share, one text for
// both sides (rt_env_texel on the host; env_sample / env_eval of rt_device.h and k_env_bake on the device).
// The map lies over the unit square (s, t) by the plain octahedral mapping: only + - * /, fabsf, copysignf and one
// sqrtf, float32 throughout, nothing fused (-ffp-contract=off on both sides), so tests/envlight_reference.py restates
// every bit in numpy.  M = world_to_env, 3x3 column-major, glm operation order: M v = (m0 x + m1 y) + m2 z.
#pragma once
#include <math.h>

#include "rt_texture.h"  // RT_HD

namespace rtmi {

// the fold of the lower hemisphere (e.z < 0) over the square's corners; the old values on the right-hand side
RT_HD void env_fold(float& px, float& py) {
    const float ox = px, oy = py;
    px = (1.f - fabsf(oy)) * copysignf(1.f, ox);
    py = (1.f - fabsf(ox)) * copysignf(1.f, oy);
}

// A texel coordinate: min((int)(s n), n - 1); a NaN coordinate counts as 0 (as rt_texture.h texel_wrap).  s is in
// [0, 1] for every finite direction; the lower clamp only keeps a hostile input inside the table.
RT_HD int env_coord(float s, int n) {
    if (s != s) return 0;
    const float f = s * (float)n;
    const int i = f < (float)n ? (int)f : n - 1;
    return i < 0 ? 0 : i;
}

// direction d -> texel (x, y) of a W x H map; l2 = |p|^2 of the octahedron point p = e / |e|_1, e = M d
RT_HD void env_dir_to_texel(int W, int H, const float* M, const float* d, int& x, int& y, float& l2) {
    const float ex = (M[0] * d[0] + M[3] * d[1]) + M[6] * d[2];
    const float ey = (M[1] * d[0] + M[4] * d[1]) + M[7] * d[2];
    const float ez = (M[2] * d[0] + M[5] * d[1]) + M[8] * d[2];
    const float a = (fabsf(ex) + fabsf(ey)) + fabsf(ez);
    float px = ex / a, py = ey / a;
    const float pz = ez / a;
    l2 = (px * px + py * py) + pz * pz;
    if (ez < 0.f) env_fold(px, py);
    const float s = px * 0.5f + 0.5f, t = py * 0.5f + 0.5f;
    x = env_coord(s, W);
    y = env_coord(t, H);
}

// (s, t) -> the octahedron point p (|p|_1 = 1)
RT_HD void env_st_to_point(float s, float t, float p[3]) {
    float px = 2.f * s - 1.f, py = 2.f * t - 1.f;
    const float z = (1.f - fabsf(px)) - fabsf(py);
    if (z < 0.f) env_fold(px, py);
    p[0] = px; p[1] = py; p[2] = z;
}

// d omega = 4 ds dt / |p|^3, so pdf_omega = pdf_st (l2 sqrtf(l2)) / 4 with l2 = p . p
RT_HD float env_pdf_omega(float pdf_st, float l2) { return (pdf_st * (l2 * sqrtf(l2))) / 4.f; }

}  // namespace rtmi
