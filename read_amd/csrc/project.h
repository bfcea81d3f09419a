// The projection of one point under every camera model, shared by every translation unit that must land a point in the same pixel
// as the rasteriser does (splat.hip, select.hip, annotate.hip, flow.hip, lidar.hip), and the camera types the rasteriser's range kernels are
// written over.  Bit-exact fp32: include it only from files compiled with -ffp-contract=off.
#pragma once
#include <cmath>

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

// point_render.cu:141-147: normalised device coordinates to the pixel (or -1), the depth and the integer column and row.  `keep` is
// what the camera itself asks of the point (a lens's limit; true where it asks nothing).
__device__ __forceinline__ int ndc_pixel(float nx, float ny, float nz, bool keep, int W, int H, float &depth, int &xx_out, int &yy_out)
{
    // NaN compares false everywhere: written so that NaN is rejected (canonical semantics).
    const bool inside = (nx >= -1.0f) & (nx <= 1.0f) & (ny >= -1.0f) & (ny <= 1.0f) &
                        (nz >= -1.0f) & (nz <= 1.0f);
    const float u = ((float)W * (nx + 1.0f)) * 0.5f;
    const float v = ((float)H * (1.0f - ny)) * 0.5f;
    depth = (nz + 1.0f) * 0.5f;
    const int xx = (int)u, yy = (int)v;
    const bool ok = keep & inside & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H);
    xx_out = xx;
    yy_out = yy;
    return ok ? yy * W + xx : -1;
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
    return ndc_pixel(nx, ny, nz, true, W, H, depth, xx_out, yy_out);
}

// project_one with what ndc_pixel rounds away kept (flow.hip; tests/flow_model.py is the definition): the continuous pixel
// coordinates u, v that the pixel is the integer part of, and the normalised device coordinates, which tell a point beside the image
// (nz in [-1, 1], nx and ny finite) from one cut by a plane.  The same operations on the same operands as project_one / ndc_pixel, so
// pixel and depth are theirs bit for bit.  M is anything indexed 0..15: a table row, or a matrix in the kernel arguments.
struct SubPixel {
    float u, v, depth, nx, ny, nz;
    int pix;                                    // the pixel, or -1
};

template <class Mat>
__device__ __forceinline__ SubPixel project_one_subpixel(float x, float y, float z, const Mat &M, int W, int H)
{
    const float c0 = M[0] * x + M[1] * y + M[2] * z + M[3] * 1.0f;
    const float c1 = M[4] * x + M[5] * y + M[6] * z + M[7] * 1.0f;
    const float c2 = M[8] * x + M[9] * y + M[10] * z + M[11] * 1.0f;
    const float c3 = M[12] * x + M[13] * y + M[14] * z + M[15] * 1.0f;
    SubPixel s;
    div3_ieee(c0, c1, c2, c3, s.nx, s.ny, s.nz);
    const bool inside = (s.nx >= -1.0f) & (s.nx <= 1.0f) & (s.ny >= -1.0f) & (s.ny <= 1.0f) & (s.nz >= -1.0f) & (s.nz <= 1.0f);
    s.u = ((float)W * (s.nx + 1.0f)) * 0.5f;
    s.v = ((float)H * (1.0f - s.ny)) * 0.5f;
    s.depth = (s.nz + 1.0f) * 0.5f;
    const int xx = (int)s.u, yy = (int)s.v;
    const bool ok = inside & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H);
    s.pix = ok ? yy * W + xx : -1;
    return s;
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

// ---- panorama camera: cylindrical projection --------------------------------------------------------------------------------
// Only the per-point projection differs from the pinhole; keys, z-test, resolve, gather and UNet are the frame's as ever.  The
// camera is 16 floats formed on the host (camera.pano_camera): c[0..11] three rows applied to (x, y, z, 1) — c0 = x_c,
// c1 = P[1,1] y_c, c3 = -z_c —, c[12] = kx = 2 / hfov_rad, c[13] = ky = P[1,2], c[14] = za = P[2,2], c[15] = zb = P[2,3].
// tests/pano_model.py is the definition; this restates it: fp32, no contraction, sums left to right, IEEE division, correctly
// rounded square root.  No chunk culling here: a cylinder does not map a box to the hull of its corners.
// One point under one panorama camera; returns the pixel or -1.  rho = 0, NaN and Inf fall out through `inside`.
__device__ __forceinline__ int project_pano_one(float x, float y, float z, const float *c, int W, int H,
                                                float &depth, int &xx_out, int &yy_out)
{
    const float c0 = c[0] * x + c[1] * y + c[2] * z + c[3] * 1.0f;
    const float c1 = c[4] * x + c[5] * y + c[6] * z + c[7] * 1.0f;
    const float c3 = c[8] * x + c[9] * y + c[10] * z + c[11] * 1.0f;
    const float rho = __builtin_sqrtf(c0 * c0 + c3 * c3);
    const float theta = pano_atan2(c0, c3);
    const float nx = theta * c[12];
    const float ny = c1 / rho - c[13];
    const float nz = (c[15] - c[14] * rho) / rho;
    return ndc_pixel(nx, ny, nz, true, W, H, depth, xx_out, yy_out);
}

// ---- lens cameras: distorted pinhole and fisheye ------------------------------------------------------------------------------
// Again only the per-point projection differs.  The camera is 32 floats formed on the host (camera.lens_camera): c[0..11] three
// UNSCALED rows applied to (x, y, z, 1) — c0 = x_c, c1 = y_c, c3 = -z_c — and twenty scalars, the same for every range of a frame,
// which travel once per launch as LensScalars: sx, ox, sy, oy = P[0,0], P[0,2], P[1,1], P[1,2]; za, zb = P[2,2], P[2,3]; the
// limit; the model (0 = Brown-Conrady pinhole, 1 = Kannala-Brandt fisheye); k[5] in OpenCV's order; seven zeros.
// tests/lens_model.py is the definition; this restates it: fp32, no contraction, sums left to right, IEEE division, correctly
// rounded square root, Horner with separate multiply and add.  The model is uniform over a launch, so the branch is scalar.
struct LensScalars {
    float s[20];
};

// One point under one lens camera (rows r[12], scalars ls); returns the pixel or -1.  A point past the limit, NaN and Inf fall out
// through `keep` and `inside`; the fisheye's axis point (rho = 0) is kept and lands on the principal point.
__device__ __forceinline__ int project_lens_one(float x, float y, float z, const float *r, const LensScalars &ls, int W, int H,
                                                float &depth, int &xx_out, int &yy_out)
{
    const float c0 = r[0] * x + r[1] * y + r[2] * z + r[3] * 1.0f;
    const float c1 = r[4] * x + r[5] * y + r[6] * z + r[7] * 1.0f;
    const float c3 = r[8] * x + r[9] * y + r[10] * z + r[11] * 1.0f;
    const float sx = ls.s[0], ox = ls.s[1], sy = ls.s[2], oy = ls.s[3], za = ls.s[4], zb = ls.s[5], limit = ls.s[6];
    float a2, b2, d;
    bool keep;
    if (ls.s[7] == 0.0f) {
        const float k1 = ls.s[8], k2 = ls.s[9], p1 = ls.s[10], p2 = ls.s[11], k3 = ls.s[12];
        const float a = c0 / c3, b = c1 / c3;
        const float r2 = a * a + b * b;
        keep = (c3 > 0.0f) & (r2 <= limit);
        const float rad = ((k3 * r2 + k2) * r2 + k1) * r2 + 1.0f;
        const float xo = a, yo = -b;                             // OpenCV's axes: its y points down
        const float xy2 = 2.0f * (xo * yo);
        const float tx = p1 * xy2 + p2 * (r2 + 2.0f * (xo * xo));
        const float ty = p1 * (r2 + 2.0f * (yo * yo)) + p2 * xy2;
        a2 = xo * rad + tx;
        b2 = -(yo * rad + ty);
        d = c3;
    } else {
        const float k1 = ls.s[8], k2 = ls.s[9], k3 = ls.s[10], k4 = ls.s[11];
        const float rho = __builtin_sqrtf(c0 * c0 + c1 * c1);
        const float theta = pano_atan2(rho, c3);
        keep = theta <= limit;
        const float t2 = theta * theta;
        const float theta_d = theta * ((((k4 * t2 + k3) * t2 + k2) * t2 + k1) * t2 + 1.0f);
        const float q = rho == 0.0f ? 0.0f : theta_d / rho;
        a2 = q * c0;
        b2 = q * c1;
        d = __builtin_sqrtf(c0 * c0 + c1 * c1 + c3 * c3);
    }
    const float nx = sx * a2 - ox;
    const float ny = sy * b2 - oy;
    const float nz = (zb - za * d) / d;
    return ndc_pixel(nx, ny, nz, keep, W, H, depth, xx_out, yy_out);
}

// ---- the camera seam ----------------------------------------------------------------------------------------------------------
// One type per camera model; everything above the per-point projection (range kernel, seed kernel, project-points kernel, the
// host's checks and frames) is written once over it.  A camera carries what is uniform over a launch and says, for the host,
//   whole_cloud   it reads the cloud itself: no cell blob, and ids may be NULL (a point's id is its index)
//   host_name     what the C ABI calls its 16 or 32 host floats
//   from_host     the launch's camera from those floats
//   frame_fault   what is wrong with the frame's camera floats, or NULL;  range_fault: the same for one range's 16 floats
struct PinholeCam {
    static constexpr bool whole_cloud = false;
    static constexpr const char *host_name = "M_host";
    static PinholeCam from_host(const float *) { return {}; }
    static const char *frame_fault(const float *) { return nullptr; }
    __device__ __forceinline__ int project(float x, float y, float z, const float *M, int W, int H, float &depth, int &xx, int &yy) const
    {
        return project_one(x, y, z, M, W, H, depth, xx, yy);
    }
};

struct PanoCam {
    static constexpr bool whole_cloud = true;
    static constexpr const char *host_name = "cam_host";
    static PanoCam from_host(const float *) { return {}; }
    // 16 finite floats, kx = 2 / hfov_rad with hfov in (0, 2 pi]
    static const char *frame_fault(const float *c)
    {
        for (int i = 0; i < 16; ++i)
            if (!std::isfinite(c[i])) return "a camera entry is not finite";
        if (!(c[12] >= (float)(1.0 / 3.14159265358979323846))) return "kx = 2 / hfov_rad must be >= 1 / pi (a field of at most 360 degrees)";
        return nullptr;
    }
    static const char *range_fault(const float *c) { return frame_fault(c); }
    __device__ __forceinline__ int project(float x, float y, float z, const float *c, int W, int H, float &depth, int &xx, int &yy) const
    {
        return project_pano_one(x, y, z, c, W, H, depth, xx, yy);
    }
};

struct LensCam {
    LensScalars ls;
    static constexpr bool whole_cloud = true;
    static constexpr const char *host_name = "cam_host";
    // cam_host is 32 floats: its first 16 are a range's entry (12 rows, 4 ignored), its last 20 the frame's scalars
    static LensCam from_host(const float *c)
    {
        LensCam cam;
        memcpy(cam.ls.s, c + 12, sizeof(cam.ls.s));
        return cam;
    }
    // every entry but the limit finite, the model 0 or 1, the limit not NaN, not negative and, for the fisheye, not above the fp32
    // pi its arctangent ends at (model 0 may carry +inf)
    static const char *frame_fault(const float *c)
    {
        for (int i = 0; i < 32; ++i)
            if (i != 18 && !std::isfinite(c[i])) return "a camera entry is not finite";
        if (c[19] != 0.0f && c[19] != 1.0f) return "the model must be 0 (distorted pinhole) or 1 (fisheye)";
        if (!(c[18] >= 0.0f)) return "the limit is negative or NaN";
        if (c[19] == 1.0f && c[18] > 3.14159265358979323846f) return "the limit of a fisheye must not exceed pi";
        return nullptr;
    }
    // the 12 rows of a range (the 4 floats after them are ignored)
    static const char *range_fault(const float *m)
    {
        for (int i = 0; i < 12; ++i)
            if (!std::isfinite(m[i])) return "a camera row entry is not finite";
        return nullptr;
    }
    __device__ __forceinline__ int project(float x, float y, float z, const float *r, int W, int H, float &depth, int &xx, int &yy) const
    {
        return project_lens_one(x, y, z, r, ls, W, H, depth, xx, yy);
    }
};

}  // namespace readhip
