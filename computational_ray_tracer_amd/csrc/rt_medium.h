// Absorbing media inside glass: the spectral Beer-Lambert transmittance of one path segment, one text
// for the host and the device (rt_medium_transmittance on the host; k_medium_eval and the per-depth stage k_medium_absorb
// of rt_medium.hip on the device).
//
// A medium belongs to a material (rt_medium, rt_scene_set_media): sigma_a(lambda) = sigma S(lambda), S the
// RGBSigmoidPolynomial of three coefficients exactly as sigmoid_eval (rt_device.h, color.h:373-399) evaluates it, its
// two fmaf included; sigma >= 0 per render-space unit length.  For a segment of length len, per hero wavelength:
//     x = (sigma S(lambda)) len;   a = x >= 87 ? 0 : (float)exp(-(double)x)
// float32 in the order written, nothing else fused (-ffp-contract=off on both sides).  The cut at 87 keeps every result a
// normal float (exp(-87) = 1.6e-38 > FLT_MIN), so the rounding argument below never meets a subnormal.
//
// The exponential takes the wavelength warps' route (rt_mathf.h): rtm::exp_tab in double, rounded to float, and the
// library exp only when near_midpoint cannot vouch for that rounding.  The returned float therefore equals the float
// rounding of any double evaluation accurate to better than 2^-46: glibc's on the host, ocml's on the device, numpy's in
// tests/medium_reference.py.  exp_tab's own comment covers |x| <= 2.3 only; its Cody-Waite reduction stays exact up to
// 87 (kd < 2^13 times the 32-bit ln2_hi / 64 is exact in double), and tools/verify_absorb.cpp runs every float of
// [0, 87) against glibc (DESIGN.md §3n records its line).  A negative or NaN x, which no render produces (sigma, S and
// len are >= 0), goes to the library call.
//
// The exp2 rows (64 x 16 B) are read from the constant arrays (rtm::TabConst), not staged in LDS as the camera kernels'
// WarpTabLds does: only the back-face hits of media-bearing materials reach the exponential, a small share of a queue,
// so a per-block copy of the table would cost every block of the stage for the few waves that use it, while the 1 KiB
// of rows stays resident in the scalar / L2 caches for those that do.
#pragma once
#include <math.h>

#include "rt_mathf.h"
#include "rt_texture.h"  // RT_HD

namespace rtmi {

static const float kMediumCut = 87.f;  // x >= kMediumCut: a = 0

// sigmoid_eval's operations (rt_device.h), host and device
RT_HD float medium_sigmoid(float c0, float c1, float c2, float lambda) {
    const float x = __builtin_fmaf(lambda, __builtin_fmaf(lambda, c0, c1), c2);
    if (__builtin_isinf(x)) return x > 0 ? 1.f : 0.f;
    return .5f + x / (2 * sqrtf(1 + (x * x)));
}

// (float)exp(-(double)x) for x in [0, kMediumCut); *fallback (may be NULL) = the library call was taken
RT_HD float medium_exp_neg(float x, int* fallback = nullptr) {
    const double xd = -(double)x;
    if (!(x >= 0.f && x < kMediumCut)) {  // outside the verified range (never from a render)
        if (fallback) *fallback = 1;
        return (float)exp(xd);
    }
    const double r = rtm::exp_tab<rtm::TabConst>(xd);
    float f = (float)r;
    const bool near = rtm::near_midpoint(r, f);
    if (near) f = (float)exp(xd);
    if (fallback) *fallback = near ? 1 : 0;
    return f;
}

// the transmittance of a segment of length len at one wavelength; m = (c0, c1, c2, sigma)
RT_HD float medium_transmittance(float c0, float c1, float c2, float sigma, float lambda, float len) {
    const float x = (sigma * medium_sigmoid(c0, c1, c2, lambda)) * len;
    return x >= kMediumCut ? 0.f : medium_exp_neg(x);
}

}  // namespace rtmi
