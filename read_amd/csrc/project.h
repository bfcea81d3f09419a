// The pinhole projection of one point, shared by every translation unit that must land a point in the same pixel as the
// rasteriser does (splat.hip, select.hip).  Bit-exact fp32: include it only from files compiled with -ffp-contract=off.
#pragma once
#include "common.h"

namespace readhip {

// The three IEEE divisions of point_render.cu:119 (c0 / c3, c1 / c3, c2 / c3) with ONE reciprocal.
// hipcc expands a correctly rounded fp32 a / b into  sb = v_div_scale(b), sa = v_div_scale(a), r = v_rcp(sb), e = fma(-sb, r, 1),
// r = fma(e, r, r), q = sa r, t = fma(-sb, q, sa), q = fma(t, r, q), t = fma(-sb, q, sa), v_div_fmas(t, r, q), v_div_fixup — 11
// instructions, 33 for a point (a quarter of pass A's vector instructions, and pass A is issue-bound).  v_div_scale only scales
// when an exponent is extreme: for 2^-40 <= |b| <= 2^40 it returns b itself, and it returns a itself unless |a| < 2^-103 (then
// |a / b| < 2^-63: n + 1 rounds to 1 whichever way the quotient was rounded — pixel and depth come out the same) or
// |a| >= 2^56 |b| (then |a / b| > 1 on both paths, or inf / NaN: the point is rejected either way).  With nothing scaled
// v_div_fmas is a plain fma and v_div_fixup returns its input, so the reciprocal and its Newton step (they depend on b alone)
// can be shared and each quotient is the same five instructions on the same operands as in the compiler's expansion — the
// same bits.  Outside the window the whole wave takes the compiler's divisions.  18 instead of 33 instructions per point;
// tests/test_gpu_splat.py::test_shared_reciprocal_projection_is_ieee_division compares > 10^8 device points with the host's
// IEEE divisions (random, window-edge, tiny, huge, zero and non-finite operands).
__device__ __forceinline__ void div3_ieee(float a0, float a1, float a2, float b, float &q0, float &q1, float &q2)
{
    const float ab = fabsf(b);
    const bool window = (ab >= 0x1p-40f) & (ab <= 0x1p40f);
    if (__builtin_expect(__ballot(!window) == 0ull, 1)) {
        float r = __builtin_amdgcn_rcpf(b);
        const float e = __builtin_fmaf(-b, r, 1.0f);
        r = __builtin_fmaf(e, r, r);
        float t;
        q0 = a0 * r;
        q1 = a1 * r;
        q2 = a2 * r;
        t = __builtin_fmaf(-b, q0, a0);
        q0 = __builtin_fmaf(t, r, q0);
        t = __builtin_fmaf(-b, q1, a1);
        q1 = __builtin_fmaf(t, r, q1);
        t = __builtin_fmaf(-b, q2, a2);
        q2 = __builtin_fmaf(t, r, q2);
        t = __builtin_fmaf(-b, q0, a0);
        q0 = __builtin_fmaf(t, r, q0);
        t = __builtin_fmaf(-b, q1, a1);
        q1 = __builtin_fmaf(t, r, q1);
        t = __builtin_fmaf(-b, q2, a2);
        q2 = __builtin_fmaf(t, r, q2);
    } else {
        q0 = a0 / b;
        q1 = a1 / b;
        q2 = a2 / b;
    }
}

// point_render.cu:135-147 for one point and one camera; returns the pixel or -1.
__device__ __forceinline__ int project_one(float x, float y, float z, const float *M, int W, int H,
                                           float &depth, int &xx_out, int &yy_out)
{
    const float c0 = M[0] * x + M[1] * y + M[2] * z + M[3] * 1.0f;
    const float c1 = M[4] * x + M[5] * y + M[6] * z + M[7] * 1.0f;
    const float c2 = M[8] * x + M[9] * y + M[10] * z + M[11] * 1.0f;
    const float c3 = M[12] * x + M[13] * y + M[14] * z + M[15] * 1.0f;
    float nx, ny, nz;
    div3_ieee(c0, c1, c2, c3, nx, ny, nz);
    // NaN compares false everywhere: written so that NaN is rejected (canonical semantics).
    const bool inside = (nx >= -1.0f) & (nx <= 1.0f) & (ny >= -1.0f) & (ny <= 1.0f) &
                        (nz >= -1.0f) & (nz <= 1.0f);
    const float u = ((float)W * (nx + 1.0f)) * 0.5f;
    const float v = ((float)H * (1.0f - ny)) * 0.5f;
    depth = (nz + 1.0f) * 0.5f;
    const int xx = (int)u, yy = (int)v;
    const bool ok = inside & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H);
    xx_out = xx;
    yy_out = yy;
    return ok ? yy * W + xx : -1;
}

// The arctangent of the panorama, lens and LiDAR cameras (splat.hip, lidar.hip); tests/pano_model.py::atan2_model is the definition.
// atan2 of the model: t = small / large of (|a|, |b|) by compare-and-select (NaN takes the 'false' side, as NumPy's where),
// Abramowitz & Stegun 4.4.49 by Horner in t^2, then the octant fix-ups.  The literals are the model's ATAN_COEFFS, bit for bit.
__device__ __forceinline__ float pano_atan2(float a, float b)
{
    const float ax = fabsf(a), az = fabsf(b);
    const bool swap = ax > az;
    const float large = swap ? ax : az, small = swap ? az : ax;
    const float t = large == 0.0f ? 0.0f : small / large;
    const float s = t * t;
    float p = 0.0028662257f;
    p = p * s + -0.0161657367f;
    p = p * s + 0.0429096138f;
    p = p * s + -0.0752896400f;
    p = p * s + 0.1065626393f;
    p = p * s + -0.1420889944f;
    p = p * s + 0.1999355085f;
    p = p * s + -0.3333314528f;
    p = p * s + 1.0f;
    float r = p * t;
    if (swap) r = 1.57079632679489661923f - r;
    if (b < 0.0f) r = 3.14159265358979323846f - r;
    return copysignf(r, a);
}

}  // namespace readhip
