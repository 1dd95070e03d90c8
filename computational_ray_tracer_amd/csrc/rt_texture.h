// Albedo textures: the arithmetic the host and the device share, one text for both sides.
//   rgb_to_sigmoid  RGBToSpectrumTable::operator() (color.cpp:26-72): rt_rgb_to_sigmoid on the host, k_texture_bake on
//                   the device;
//   texel_index     the nearest-texel rule of the reference's Li (RayTracerTestApp.h:229-242) on the uv of
//                   Triangle::CalculateLocalSurface (Shapes.h:1036-1046): rt_texel_index on the host, the shade
//                   kernels' fetch on the device.
// float32 throughout, nothing fused (the build compiles both sides with -ffp-contract=off).
#pragma once
#include <math.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define RT_HD __host__ __device__ inline
#else
#define RT_HD inline
#endif

namespace rtmi {

static const int kRgbRes = 64;  // the coefficient table's resolution (RGBToSpectrumTable::res)
static const size_t kRgbTableFloats = (size_t)3 * kRgbRes * kRgbRes * kRgbRes * 3;

RT_HD float rgb_lerp(float x, float a, float b) { return (1 - x) * a + x * b; }  // helpers.h:154-157

// color.cpp:26-72 RGBToSpectrumTable::operator() (non-uniform branch): the largest component's table, (x, y) = the other
// two scaled by (res - 1) / z, z's interval by FindInterval over the z-nodes (helpers.h:159-172), float trilinear Lerps.
// zn: res z-nodes; co: [3][res][res][res][3] coefficients.
RT_HD void rgb_table_lookup(const float* zn, const float* co, const float* rgb, float* c) {
    const int res = kRgbRes;
    const int maxc = (rgb[0] > rgb[1]) ? ((rgb[0] > rgb[2]) ? 0 : 2) : ((rgb[1] > rgb[2]) ? 1 : 2);
    const float z = rgb[maxc];
    const float x = rgb[(maxc + 1) % 3] * (res - 1) / z;
    const float y = rgb[(maxc + 2) % 3] * (res - 1) / z;
    const int xi = (int)x < res - 2 ? (int)x : res - 2, yi = (int)y < res - 2 ? (int)y : res - 2;
    long size = (long)res - 2, first = 1;  // FindInterval(res, zNodes[i] < z)
    while (size > 0) {
        const long half = size >> 1, middle = first + half;
        const bool r = zn[middle] < z;
        first = r ? middle + 1 : first;
        size = r ? size - (half + 1) : half;
    }
    long zl = first - 1 > 0 ? first - 1 : 0;
    const int zi = (int)(zl < (long)res - 2 ? zl : (long)res - 2);
    const float dx = x - xi, dy = y - yi, dz = (z - zn[zi]) / (zn[zi + 1] - zn[zi]);
    for (int i = 0; i < 3; ++i) {
        const float* q = co + ((size_t)maxc * 64 * 64 * 64 * 3 + (size_t)zi * 64 * 64 * 3 + (size_t)yi * 64 * 3 +
                               (size_t)xi * 3 + i);
        const size_t ox = 3, oy = 64 * 3, oz = 64 * 64 * 3;
        c[i] = rgb_lerp(dz, rgb_lerp(dy, rgb_lerp(dx, q[0], q[ox]), rgb_lerp(dx, q[oy], q[ox + oy])),
                        rgb_lerp(dy, rgb_lerp(dx, q[oz], q[ox + oz]), rgb_lerp(dx, q[oy + oz], q[ox + oy + oz])));
    }
}

// RGBToSpectrumTable::operator() for rgb in [0,1]^3: the uniform-RGB closed form (color.cpp:35-37), else the table
RT_HD void rgb_to_sigmoid(const float* zn, const float* co, const float* rgb, float* c) {
    if (rgb[0] == rgb[1] && rgb[1] == rgb[2]) {
        const float g = rgb[0];
        c[0] = 0;
        c[1] = 0;
        c[2] = (g - .5f) / sqrtf(g * (1 - g));  // +-inf at 0 and 1: s(+-inf) = 1, 0
        return;
    }
    rgb_table_lookup(zn, co, rgb, c);
}

// One coordinate of the texel rule: CLAMP min(max(u, 0), 1) (Shapes.h:1045-1046), REPEAT u - floor(u) (0 when that is
// not < 1: -1e-9 rounds to 1, +-inf gives NaN); a NaN coordinate counts as 0 (build-defined).
RT_HD float texel_wrap(int wrap, float u) {
    if (u != u) return 0.f;
    if (wrap == 1) {
        const float f = u - floorf(u);
        return f < 1.f ? f : 0.f;
    }
    return u < 0.f ? 0.f : (u > 1.f ? 1.f : u);
}
// index = y W + x with x = (int)floor(u' W) % W (u' = 1 wraps to column 0, RayTracerTestApp.h:234) and
// y = min((int)floor(v' H), H - 1) (the reference reads past the image at v = 1; the clamp is build-defined)
RT_HD int texel_index(int W, int H, int wrap, float u, float v) {
    const float uw = texel_wrap(wrap, u), vw = texel_wrap(wrap, v);
    const int x = (int)floorf(uw * (float)W) % W;
    const int yf = (int)floorf(vw * (float)H);
    const int y = yf < H - 1 ? yf : H - 1;
    return y * W + x;
}

}  // namespace rtmi
