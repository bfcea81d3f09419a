// Host weight packers of the gated-convolution kernels (conv.hip): every read_conv_pack_*_host of read_hip.h, the sizes of what
// they write and read_conv_unpack_weights_host.  No HIP call is made here.
//
// The split-operand orders (w4h, f4x1, dkh) are one row-wise driver, pack_split_rows, around a filter transform and an index map;
// the steps they share — the Winograd G tables, the power-of-two row scale, the hi / lo cut — exist once.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "internal.h"

using namespace readhip;

namespace {

// F(2x2,3x3) and F(4x4,3x3) filter transforms U = G g G^T
const float G4[4][3] = {{1.f, 0.f, 0.f}, {.5f, .5f, .5f}, {.5f, -.5f, .5f}, {0.f, 0.f, 1.f}};
const double G6[6][3] = {{0.25, 0.0, 0.0}, {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                         {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0.0, 0.0, 1.0}};

// The sums below are rounded once (fp32 sums as they always were): the order of their terms is part of the packed format.
float f2x2_filter(const float *k, int i, int j)                // U[i][j] of one 3x3 filter, fp32
{
    float u = 0.0f;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) u += G4[i][a] * k[a * 3 + b] * G4[j][b];
    return u;
}
double f4x4_filter(const float *k, int fq)                     // U[fq / 6][fq % 6] of one 3x3 filter, in double
{
    double u = 0.0;
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) u += G6[fq / 6][a] * (double)k[a * 3 + b] * G6[fq % 6][b];
    return u;
}
double f4x1_filter(const float *k, int t)                      // (G w[ky][:])[f], t = 6 ky + f: the transform along x only
{
    double u = 0.0;
    for (int b = 0; b < 3; ++b) u += G6[t % 6][b] * (double)k[(t / 6) * 3 + b];
    return u;
}

// double -> IEEE binary16, round to nearest even, subnormals kept (the values are far inside the range: |x| < 2^15)
unsigned short f16_bits_rtn(double x)
{
    const unsigned short sign = std::signbit(x) ? 0x8000u : 0u;
    double ax = std::fabs(x);
    if (ax == 0.0) return sign;
    if (ax >= 65520.0) return (unsigned short)(sign | 0x7c00u);
    int e;
    (void)std::frexp(ax, &e);                                  // ax = f 2^e, f in [0.5, 1)
    int ex = e - 1;                                            // ax = 1.m x 2^ex
    if (ex < -14) ex = -14;                                    // subnormal: fixed quantum 2^-24
    const double q = std::ldexp(1.0, ex - 10);                 // quantum of the 11-bit significand
    const double r = std::nearbyint(ax / q);                   // ties to even (default rounding mode)
    const double v = r * q;                                    // may have carried into the next binade: recompute the fields
    if (v >= 65520.0) return (unsigned short)(sign | 0x7c00u);
    if (v < std::ldexp(1.0, -14)) return (unsigned short)(sign | (unsigned short)std::lrint(v / std::ldexp(1.0, -24)));
    int e2;
    (void)std::frexp(v, &e2);
    const int ex2 = e2 - 1;
    const unsigned mant = (unsigned)std::lrint(v / std::ldexp(1.0, ex2 - 10)) - 1024u;
    return (unsigned short)(sign | (unsigned)((ex2 + 15) << 10) | mant);
}
double f16_value(unsigned short h)
{
    const int e = (h >> 10) & 31, m = h & 1023;
    const double v = e == 0 ? std::ldexp((double)m, -24) : std::ldexp((double)(1024 + m), e - 25);
    return (h & 0x8000u) ? -v : v;
}

// The exponent ex of a row's scale s = 2^ex: max |U| s in [2^14, 2^15).  An all-zero (or non-finite) row: 0.
int row_scale_exponent(double max_abs)
{
    int ex = 0;
    if (max_abs > 0.0 && std::isfinite(max_abs)) {
        int e;
        (void)std::frexp(max_abs, &e);                         // max_abs in [2^(e-1), 2^e)
        ex = 15 - e;
        if (ex > 60) ex = 60;                                  // a row of denormal weights: keep 1 / s an fp32 normal
        if (ex < -60) ex = -60;
    }
    return ex;
}

// The scaled value us as hi = f16(us) and lo = f16(us - hi) (round to nearest even, both) at `at` (halfs) of a fragment's hi piece
// and of its lo piece, 512 halfs on
void store_split(unsigned short *h, size_t at, double us)
{
    const unsigned short hi = f16_bits_rtn(us), lo = f16_bits_rtn(us - f16_value(hi));
    h[at] = hi;
    h[at + 512] = lo;
}

// A split-operand order, row by row (row = [conv_f | conv_m] x padded output channel): transform(k, U) fills U[t Cin + ci], t < T,
// from the row's filters k = w[co] (Cin filters); a padded row is all zero.  The row is scaled by the power of two s that puts its
// largest |U s| in [2^14, 2^15) and cut into f16 pieces; index(fm, co, t, ci) is where the hi piece of an element goes (halfs; each
// 1024-half fragment is [hi 512 | lo 512]).  Behind the Cin T 2 CoutPad floats of halfs: 2 CoutPad floats 1 / s ([f rows | m rows]).
template <typename Transform, typename Index>
void pack_split_rows(int Cin, int Cout, int T, int taps, const float *wf, const float *wm, void *out, Transform transform, Index index)
{
    const int CoutPad = pad32(Cout);
    unsigned short *h = static_cast<unsigned short *>(out);
    float *inv = reinterpret_cast<float *>(out) + (size_t)Cin * T * 2 * CoutPad;
    std::vector<double> U((size_t)T * Cin);
    for (int row = 0; row < 2 * CoutPad; ++row) {
        const int fm = row / CoutPad, co = row % CoutPad;
        if (co < Cout) transform((fm ? wm : wf) + (size_t)co * Cin * taps, U.data());
        else std::fill(U.begin(), U.end(), 0.0);
        double mx = 0.0;
        for (const double u : U) mx = std::fmax(mx, std::fabs(u));
        const int ex = row_scale_exponent(mx);
        inv[row] = (float)std::ldexp(1.0, -ex);
        for (int t = 0; t < T; ++t)
            for (int ci = 0; ci < Cin; ++ci) store_split(h, index(fm, co, t, ci), std::ldexp(U[(size_t)t * Cin + ci], ex));
    }
}

// [group][wave 4][chunk of 32 cin][t < T][piece][lane][8 halfs], lane (i = lane & 15, kq = lane >> 4): row i of the wave (i < 8: conv_f
// of channel 32 group + 8 wave + i, else conv_m of channel ... + i - 8), cin = 32 chunk + 8 kq + e
struct WaveRowsIndex {
    int Cin, T;
    size_t operator()(int fm, int co, int t, int ci) const
    {
        const int g = co / 32, w = (co % 32) / 8, i = (co % 8) + 8 * fm, c = ci / 32, kq = (ci % 32) / 8, e = ci % 8;
        const size_t frag = ((((size_t)(g * 4 + w) * (Cin / 32) + c) * T + t) * 2) * 512;
        return frag + (size_t)(i + 16 * kq) * 8 + e;
    }
};

}  // namespace

extern "C" size_t read_conv_packed_floats(int Cin, int Cout, int ksize)
{
    if (Cin < 8 || Cin % 8 || Cout < 1 || (ksize != 1 && ksize != 3 && ksize != 4)) return 0;
    return (size_t)Cin * ksize * ksize * 2 * pad32(Cout);
}
extern "C" size_t read_conv_param_floats(int Cout) { return Cout < 1 ? 0 : (size_t)4 * pad32(Cout); }

extern "C" int read_conv_pack_weights_host(int Cin, int Cout, int ksize, int kc, const float *wf, const float *wm,
                                           float *wpacked_host)
{
    READ_CHECK_ARG(wf && wm && wpacked_host, "read_conv_pack_weights_host: null pointer");
    READ_CHECK_ARG(ksize == 1 || ksize == 3 || ksize == 4, "read_conv_pack_weights_host: ksize must be 1, 3 or 4");
    // (for 1x1 layers the fragment order does not depend on kc: k8 steps are simply consecutive, so 16- and 32-channel
    //  chunk kernels read the same blob)
    READ_CHECK_ARG((kc == 8 || kc == 16 || (kc == 32 && ksize == 1)) && Cin >= kc && Cin % kc == 0,
                   "read_conv_pack_weights_host: Cin=%d is not a multiple of kc=%d", Cin, kc);
    READ_CHECK_ARG(Cout >= 1, "read_conv_pack_weights_host: Cout < 1");
    const int CoutPad = pad32(Cout), NT = CoutPad / 16, KK = kc / 8, taps = ksize * ksize;
    const int nchunks = Cin / kc;
    size_t o = 0;
    for (int chunk = 0; chunk < nchunks; ++chunk)
        for (int tap = 0; tap < taps; ++tap)
            for (int kk = 0; kk < KK; ++kk)
                for (int nt = 0; nt < NT; ++nt) {
                    const float *w = (nt & 1) ? wm : wf;
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 4; ++j, ++o) {
                            const int cout = (nt >> 1) * 32 + (lane & 31);
                            const int cin = chunk * kc + kk * 8 + 4 * (lane >> 5) + j;
                            wpacked_host[o] = cout < Cout ? w[((size_t)cout * Cin + cin) * taps + tap] : 0.0f;
                        }
                }
    return READ_OK;
}

// The inverse of read_conv_pack_weights_host: the layer's weights (Cout, Cin, k, k), exact, out of its direct fragment order.
extern "C" int read_conv_unpack_weights_host(int Cin, int Cout, int ksize, int kc, const float *wpacked_host, float *wf, float *wm)
{
    READ_CHECK_ARG(wf && wm && wpacked_host, "read_conv_unpack_weights_host: null pointer");
    READ_CHECK_ARG((ksize == 1 || ksize == 3 || ksize == 4) && (kc == 8 || kc == 16 || (kc == 32 && ksize == 1)) && Cin >= kc && Cin % kc == 0 && Cout >= 1,
                   "read_conv_unpack_weights_host: bad shape (Cin=%d kc=%d ksize=%d)", Cin, kc, ksize);
    const int CoutPad = pad32(Cout), NT = CoutPad / 16, KK = kc / 8, taps = ksize * ksize;
    const int nchunks = Cin / kc;
    size_t o = 0;
    for (int chunk = 0; chunk < nchunks; ++chunk)
        for (int tap = 0; tap < taps; ++tap)
            for (int kk = 0; kk < KK; ++kk)
                for (int nt = 0; nt < NT; ++nt) {
                    float *w = (nt & 1) ? wm : wf;
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 4; ++j, ++o) {
                            const int cout = (nt >> 1) * 32 + (lane & 31);
                            const int cin = chunk * kc + kk * 8 + 4 * (lane >> 5) + j;
                            if (cout < Cout) w[((size_t)cout * Cin + cin) * taps + tap] = wpacked_host[o];
                        }
                }
    return READ_OK;
}

extern "C" size_t read_conv_wino_floats(int Cin, int Cout)
{
    if (Cin < 16 || Cin % 16 || Cout < 1) return 0;
    return (size_t)Cin * 16 * 2 * pad32(Cout);
}

// U = G g G^T per (cout, cin) pair, packed [group][k8 step][row i][j][f|m][lane][4] (tests/wino_ref.py).
extern "C" int read_conv_pack_wino_host(int Cin, int Cout, const float *wf, const float *wm, float *out)
{
    READ_CHECK_ARG(wf && wm && out, "read_conv_pack_wino_host: null pointer");
    READ_CHECK_ARG(Cin >= 16 && Cin % 16 == 0 && Cout >= 1, "read_conv_pack_wino_host: needs Cin %% 16 == 0 (got %d)", Cin);
    const int CoutPad = pad32(Cout), groups = CoutPad / 32, nsteps = Cin / 8;
    size_t o = 0;
    for (int g = 0; g < groups; ++g)
        for (int s = 0; s < nsteps; ++s)
            for (int i = 0; i < 4; ++i)
                for (int j = 0; j < 4; ++j)
                    for (int fm = 0; fm < 2; ++fm) {
                        const float *w = fm ? wm : wf;
                        for (int lane = 0; lane < 64; ++lane)
                            for (int e = 0; e < 4; ++e, ++o) {
                                const int co = g * 32 + (lane & 31), ci = 8 * s + 4 * (lane >> 5) + e;
                                const float u = co < Cout ? f2x2_filter(w + ((size_t)co * Cin + ci) * 9, i, j) : 0.0f;
                                out[o] = i == 2 ? -u : u;      // the kernel builds row 2 of B^T d negated
                            }
                    }
    return READ_OK;
}

// The wave-autonomous Winograd kernel's order (tests/wino16_ref.py): [group][wave 4][chunk of 16 cin][a][j][lane][e]; lane
// (i = lane & 15, kl = lane >> 4) holds U_{i < 8 ? f : m}[a][j][cin = 16 chunk + 4 kl + e][cout = 32 group + 8 wave + (i & 7)].
extern "C" int read_conv_pack_w16_host(int Cin, int Cout, const float *wf, const float *wm, float *out)
{
    READ_CHECK_ARG(wf && wm && out, "read_conv_pack_w16_host: null pointer");
    READ_CHECK_ARG(Cin >= 16 && Cin % 16 == 0 && Cout >= 1, "read_conv_pack_w16_host: needs Cin %% 16 == 0 (got %d)", Cin);
    const int CoutPad = pad32(Cout), groups = CoutPad / 32, nchunks = Cin / 16;
    size_t o = 0;
    for (int g = 0; g < groups; ++g)
        for (int w = 0; w < 4; ++w)
            for (int c = 0; c < nchunks; ++c)
                for (int i = 0; i < 4; ++i)
                    for (int j = 0; j < 4; ++j)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int e = 0; e < 4; ++e, ++o) {
                                const int slot = lane & 15, co = g * 32 + w * 8 + (slot & 7), ci = 16 * c + 4 * (lane >> 4) + e;
                                out[o] = co < Cout ? f2x2_filter(((slot >> 3) ? wm : wf) + ((size_t)co * Cin + ci) * 9, i, j) : 0.0f;
                            }
    return READ_OK;
}

extern "C" size_t read_conv_w4_floats(int Cin, int Cout)
{
    if (Cin < 16 || Cin % 16 || Cout < 1) return 0;
    return (size_t)Cin * 36 * 2 * pad32(Cout);
}

// F(4x4,3x3): U = G g G^T (6 x 6) per (cout, cin) pair, G = [1/4 0 0; -1/6 -1/6 -1/6; -1/6 1/6 -1/6; 1/24 1/12 1/6; 1/24 -1/12 1/6; 0 0 1],
// evaluated in double and rounded once; order [group][wave 4][chunk of 16 cin][frequency 6 xi + nu][lane][e] with lane
// (i = lane & 15, kl = lane >> 4) = U_{i < 8 ? f : m}[xi][nu][cin = 16 chunk + 4 kl + e][cout = 32 group + 8 wave + (i & 7)]   (tests/wino4_ref.py)
extern "C" int read_conv_pack_w4_host(int Cin, int Cout, const float *wf, const float *wm, float *out)
{
    READ_CHECK_ARG(wf && wm && out, "read_conv_pack_w4_host: null pointer");
    READ_CHECK_ARG(Cin >= 16 && Cin % 16 == 0 && Cout >= 1, "read_conv_pack_w4_host: needs Cin %% 16 == 0 (got %d)", Cin);
    const int CoutPad = pad32(Cout), groups = CoutPad / 32, nchunks = Cin / 16;
    size_t o = 0;
    for (int g = 0; g < groups; ++g)
        for (int w = 0; w < 4; ++w)
            for (int c = 0; c < nchunks; ++c)
                for (int fq = 0; fq < 36; ++fq)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int e = 0; e < 4; ++e, ++o) {
                            const int slot = lane & 15, co = g * 32 + w * 8 + (slot & 7), ci = 16 * c + 4 * (lane >> 4) + e;
                            out[o] = co < Cout ? (float)f4x4_filter(((slot >> 3) ? wm : wf) + ((size_t)co * Cin + ci) * 9, fq) : 0.0f;
                        }
    return READ_OK;
}

// F(4x4,3x3) operand of the split-operand kernel (gated_conv_wino4h_kernel): U = G g G^T in double, scaled per output ROW by the
// power of two s that puts max |U s| of the row in [2^14, 2^15), cut into Uh = f16(U s) and Ul = f16(U s - Uh) (round to nearest
// even, both); order [group][wave 4][chunk of 32 cin][frequency 36][piece Uh | Ul][lane][8 halfs], lane (i = lane & 15, kq = lane >> 4)
// = rows as in read_conv_pack_w4_host, cin = 32 chunk + 8 kq + e; then 2 * CoutPad floats 1 / s ([conv_f rows | conv_m rows]).
// Sized in floats like every block of a packed blob: Cin * 36 * 2 * CoutPad (the halfs) + 2 * CoutPad.   (tests/wino4h_ref.py)
extern "C" size_t read_conv_w4h_floats(int Cin, int Cout)
{
    if (Cin < 32 || Cin % 32 || Cout < 1) return 0;
    return (size_t)Cin * 36 * 2 * pad32(Cout) + 2 * (size_t)pad32(Cout);
}

extern "C" int read_conv_pack_w4h_host(int Cin, int Cout, const float *wf, const float *wm, void *out)
{
    READ_CHECK_ARG(wf && wm && out, "read_conv_pack_w4h_host: null pointer");
    READ_CHECK_ARG(Cin >= 32 && Cin % 32 == 0 && Cout >= 1, "read_conv_pack_w4h_host: needs Cin %% 32 == 0 (got %d)", Cin);
    pack_split_rows(Cin, Cout, 36, 9, wf, wm, out,
                    [Cin](const float *k, double *U) {
                        for (int ci = 0; ci < Cin; ++ci)
                            for (int fq = 0; fq < 36; ++fq) U[(size_t)fq * Cin + ci] = f4x4_filter(k + (size_t)ci * 9, fq);
                    },
                    WaveRowsIndex{Cin, 36});
    return READ_OK;
}

// F(4,3)-by-rows operand of gated_conv_f4x1h_kernel: U[ky] = G w[ky][:] in double (the filter transform along x only), scaled per
// output ROW by the power of two s that puts max |U s| of the row in [2^14, 2^15), cut into Uh = f16(U s) and Ul = f16(U s - Uh);
// order [group][wave 4][chunk of 32 cin][ky 3][frequency 6][piece Uh | Ul][lane][8 halfs], lanes as in read_conv_pack_w4h_host; then
// 2 * CoutPad floats 1 / s ([conv_f rows | conv_m rows]).  Half the bytes of the F(4x4) order: Cin * 18 * pad32(Cout) * 2 halfs.
extern "C" size_t read_conv_f4x1_floats(int Cin, int Cout)
{
    if (Cin < 32 || Cin % 32 || Cout < 1) return 0;
    return (size_t)Cin * 18 * 2 * pad32(Cout) + 2 * (size_t)pad32(Cout);
}

extern "C" int read_conv_pack_f4x1_host(int Cin, int Cout, const float *wf, const float *wm, void *out)
{
    READ_CHECK_ARG(wf && wm && out, "read_conv_pack_f4x1_host: null pointer");
    READ_CHECK_ARG(Cin >= 32 && Cin % 32 == 0 && Cout >= 1, "read_conv_pack_f4x1_host: needs Cin %% 32 == 0 (got %d)", Cin);
    pack_split_rows(Cin, Cout, 18, 9, wf, wm, out,
                    [Cin](const float *k, double *U) {
                        for (int ci = 0; ci < Cin; ++ci)
                            for (int t = 0; t < 18; ++t) U[(size_t)t * Cin + ci] = f4x1_filter(k + (size_t)ci * 9, t);
                    },
                    WaveRowsIndex{Cin, 18});
    return READ_OK;
}

// Operand of the direct split-operand kernel (gated_conv_d3h_kernel): the 3x3 weights themselves, scaled per output ROW by the power
// of two s that puts the row's largest |w s| in [2^14, 2^15), cut into wh = f16(w s) and wl = f16(w s - wh); order
// [group][row half rh 2][chunk of 32 cin][tap 9 = 3 ky + kx][row block rb 2][piece wh | wl][lane][8 halfs], lane (i = lane & 15,
// kq = lane >> 4) = row i of the block (i < 8: conv_f of channel 32 g + 16 rh + 8 rb + i, else conv_m of channel ... + i - 8), cin = 32
// chunk + 8 kq + e; then 2 * CoutPad floats 1 / s ([conv_f rows | conv_m rows]).   (tests/d3h_ref.py)
extern "C" size_t read_conv_dkh_floats(int Cin, int Cout, int ksize)
{
    if (ksize == 1) return (Cin < 16 || Cin % 16 || Cout < 1) ? 0 : (size_t)Cin * 2 * pad32(Cout) + 2 * (size_t)pad32(Cout);
    if (Cin < 32 || Cin % 32 || Cout < 1 || (ksize != 3 && ksize != 4)) return 0;
    return (size_t)Cin * 2 * ksize * ksize * pad32(Cout) + 2 * (size_t)pad32(Cout);
}
extern "C" size_t read_conv_d3h_floats(int Cin, int Cout) { return read_conv_dkh_floats(Cin, Cout, 3); }
extern "C" int read_conv_pack_dkh_host(int Cin, int Cout, int ksize, const float *wf, const float *wm, void *out);
extern "C" int read_conv_pack_d3h_host(int Cin, int Cout, const float *wf, const float *wm, void *out)
{
    return read_conv_pack_dkh_host(Cin, Cout, 3, wf, wm, out);
}

// ... the same for a k x k kernel, k = 3 or 4 (tap = k ky + kx): the 4 x 4 / stride-2 layers run on the stride-2 kernel too
extern "C" int read_conv_pack_dkh_host(int Cin, int Cout, int ksize, const float *wf, const float *wm, void *out)
{
    READ_CHECK_ARG(wf && wm && out, "read_conv_pack_dkh_host: null pointer");
    const int NT = ksize * ksize;
    const auto taps_of_row = [Cin, NT](const float *k, double *U) {       // no transform: U[tap][cin] = w[cin][tap]
        for (int ci = 0; ci < Cin; ++ci)
            for (int tap = 0; tap < NT; ++tap) U[(size_t)tap * Cin + ci] = (double)k[(size_t)ci * NT + tap];
    };
    if (ksize == 1) {
        // 1x1 layers (gated_conv_pxh_kernel, v_mfma_f32_32x32x16_f16 with the weights as the A operand): the same rows, scales and
        // pieces in the order [k16 step][tile t = 2 group + (f | m)][wh | wl][lane][8 halfs], lane (i = lane & 31, h = lane >> 5) =
        // row i of the tile (conv_f / conv_m of channel 32 group + i), cin = 16 step + 8 h + e; then the 2 * CoutPad floats 1 / s.
        READ_CHECK_ARG(Cin >= 16 && Cin % 16 == 0 && Cout >= 1, "read_conv_pack_dkh_host: a 1x1 layer needs Cin %% 16 == 0 (got %d)", Cin);
        const int NTL = pad32(Cout) / 16;
        pack_split_rows(Cin, Cout, 1, 1, wf, wm, out, taps_of_row, [NTL](int fm, int co, int, int ci) {
            const int t = 2 * (co / 32) + fm, i = co % 32, st = ci / 16, hh = (ci % 16) / 8, e = ci % 8;
            return (((size_t)st * NTL + t) * 2) * 512 + (size_t)(i + 32 * hh) * 8 + e;
        });
        return READ_OK;
    }
    READ_CHECK_ARG(ksize == 3 || ksize == 4, "read_conv_pack_dkh_host: ksize must be 1, 3 or 4");
    READ_CHECK_ARG(Cin >= 32 && Cin % 32 == 0 && Cout >= 1, "read_conv_pack_dkh_host: needs Cin %% 32 == 0 (got %d)", Cin);
    const int nchunks = Cin / 32;
    pack_split_rows(Cin, Cout, NT, NT, wf, wm, out, taps_of_row, [nchunks, NT](int fm, int co, int tap, int ci) {
        const int g = co / 32, rh = (co % 32) / 16, rb = (co % 16) / 8, i = (co % 8) + 8 * fm, c = ci / 32, kq = (ci % 32) / 8, e = ci % 8;
        return (((((size_t)(g * 2 + rh) * nchunks + c) * NT + tap) * 2 + rb) * 2) * 512 + (size_t)(i + 16 * kq) * 8 + e;
    });
    return READ_OK;
}

// 3x3 weights of a layer with 8, 16 or 32 input channels as the implicit-GEMM operand of the split-operand pixel-lane kernel: the matrix
// W'[cout][k = tap Cin + ci] (tap = 3 ky + kx), k padded with zeros to whole k16 steps, in the 1x1 operand's order (read_conv_pack_dkh_host, ksize 1)
extern "C" size_t read_conv_t3h_floats(int Cin, int Cout)
{
    return (Cin == 8 || Cin == 16 || Cin == 32) && Cout >= 1 ? read_conv_dkh_floats((9 * Cin + 15) / 16 * 16, Cout, 1) : 0;
}

extern "C" int read_conv_pack_t3h_host(int Cin, int Cout, const float *wf, const float *wm, void *out)
{
    READ_CHECK_ARG(wf && wm && out, "read_conv_pack_t3h_host: null pointer");
    READ_CHECK_ARG(read_conv_t3h_floats(Cin, Cout) > 0, "read_conv_pack_t3h_host: needs Cin = 8, 16 or 32 (got %d)", Cin);
    const int K = (9 * Cin + 15) / 16 * 16;
    std::vector<float> f((size_t)Cout * K, 0.0f), m((size_t)Cout * K, 0.0f);
    for (int co = 0; co < Cout; ++co)
        for (int ci = 0; ci < Cin; ++ci)
            for (int tap = 0; tap < 9; ++tap) {
                f[(size_t)co * K + tap * Cin + ci] = wf[((size_t)co * Cin + ci) * 9 + tap];
                m[(size_t)co * K + tap * Cin + ci] = wm[((size_t)co * Cin + ci) * 9 + tap];
            }
    return read_conv_pack_dkh_host(K, Cout, 1, f.data(), m.data(), out);
}

// Small-Cout order (gated_conv_smallc_kernel): [tap][cin][f0 f1 f2 f3 | m0 m1 m2 m3], channels >= Cout zero.
extern "C" size_t read_conv_sc_floats(int Cin, int Cout)
{
    return (Cin == 32 && Cout >= 1 && Cout <= 4) ? (size_t)9 * Cin * 8 : 0;      // the kernel is instantiated for 32 input channels
}

extern "C" int read_conv_pack_sc_host(int Cin, int Cout, const float *wf, const float *wm, float *out)
{
    READ_CHECK_ARG(wf && wm && out, "read_conv_pack_sc_host: null pointer");
    READ_CHECK_ARG(read_conv_sc_floats(Cin, Cout) > 0, "read_conv_pack_sc_host: needs Cin == 32 and 1 <= Cout <= 4 (got %d, %d)", Cin, Cout);
    for (int tap = 0; tap < 9; ++tap)
        for (int ci = 0; ci < Cin; ++ci)
            for (int j = 0; j < 8; ++j) {
                const int co = j & 3;
                out[((size_t)tap * Cin + ci) * 8 + j] = co < Cout ? ((j >> 2) ? wm : wf)[((size_t)co * Cin + ci) * 9 + tap] : 0.0f;
            }
    return READ_OK;
}

extern "C" int read_conv_pack_params_host(int Cout, const float *bf, const float *bm, const float *gamma,
                                          const float *beta, const float *mean, const float *var, float eps,
                                          float *params_host)
{
    READ_CHECK_ARG(bf && bm && gamma && beta && mean && var && params_host, "read_conv_pack_params_host: null pointer");
    READ_CHECK_ARG(Cout >= 1, "read_conv_pack_params_host: Cout < 1");
    const int CoutPad = pad32(Cout);
    for (int c = 0; c < CoutPad; ++c) {
        const bool ok = c < Cout;
        // eval-mode BatchNorm folded to y = x*scale + shift (applied AFTER the gate product)
        const float scale = ok ? gamma[c] / sqrtf(var[c] + eps) : 0.0f;
        params_host[c] = ok ? bf[c] : 0.0f;
        params_host[CoutPad + c] = ok ? bm[c] : 0.0f;
        params_host[2 * CoutPad + c] = scale;
        params_host[3 * CoutPad + c] = ok ? beta[c] - mean[c] * scale : 0.0f;
    }
    return READ_OK;
}
