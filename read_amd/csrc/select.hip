// Object selection for gfx950: per-point labels from oriented 3-D boxes and from 2-D label images lifted over posed views
// (the contract is tests/select_model.py, held bit for bit).
//
//   select_boxes_kernel   point i gets label_of[k] of the first box k that contains it: 12 B read + 4 B written per point, the K
//                         matrices staged once per workgroup in LDS and read wave-uniformly (broadcast, no bank conflicts)
//   select_near_kernel    per pixel of a level-0 frame: the clip w of its winning point (+inf where the pixel is empty)
//   select_vote_kernel    per point and view: project as the rasteriser does, test against near, count seen / hit in the state word
//   select_finish_kernel  state word -> label
//
// Every comparison is written so that a NaN fails it.  Compiled with -ffp-contract=off: products and sums stay apart, left to right.
#include "common.h"
#include "internal.h"

#pragma clang fp contract(off)

#include "project.h"

using namespace readhip;

namespace {

constexpr int MAX_BOXES = 1024;
constexpr int BOX_FLOATS = 12;

struct Cam1 {
    float m[16];
};

// LDS: K * 12 floats (the matrices), then K labels — 52 B per box, 52 KiB at K = 1024.
__global__ __launch_bounds__(256) void select_boxes_kernel(const float *__restrict__ xyz, long long n, const float *__restrict__ boxes,
                                                           const int32_t *__restrict__ label_of, int K, const int32_t *labels_in,
                                                           int32_t *labels_out)
{
    extern __shared__ float lds[];
    float *A = lds;
    int32_t *lab = reinterpret_cast<int32_t *>(lds + (size_t)K * BOX_FLOATS);
    for (int j = threadIdx.x; j < K * BOX_FLOATS; j += blockDim.x) A[j] = boxes[j];
    for (int j = threadIdx.x; j < K; j += blockDim.x) lab[j] = label_of[j];
    __syncthreads();
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        int found = -1;
        for (int k = 0; k < K; ++k) {
            const float *a = A + k * BOX_FLOATS;
            const float t0 = a[0] * x + a[1] * y + a[2] * z + a[3] * 1.0f;
            const float t1 = a[4] * x + a[5] * y + a[6] * z + a[7] * 1.0f;
            const float t2 = a[8] * x + a[9] * y + a[10] * z + a[11] * 1.0f;
            const float m0 = fabsf(t0), m1 = fabsf(t1), m2 = fabsf(t2);
            const bool inside = (m0 <= 1.0f) & (m1 <= 1.0f) & (m2 <= 1.0f);
            if (inside & (found < 0)) found = lab[k];
            if (__ballot(found < 0) == 0ull) break;          // every lane of the wave has its first box
        }
        if (found < 0) found = labels_in ? labels_in[i] : 0;  // own element, read before it is written: labels_in may be labels_out
        labels_out[i] = found;
    }
}

__device__ __forceinline__ float clip_w(const float *M, float x, float y, float z)
{
    return M[12] * x + M[13] * y + M[14] * z + M[15] * 1.0f;          // c3 of project_one
}

__global__ __launch_bounds__(256) void select_near_kernel(const float *__restrict__ xyz, long long n, Cam1 cam, long long pixels,
                                                          const int32_t *__restrict__ idx0, const float *__restrict__ depth0,
                                                          float *__restrict__ near)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= pixels) return;
    const int32_t id = idx0[p];
    const bool empty = (id == 0) & (__float_as_uint(depth0[p]) == 0u);
    float w = __uint_as_float(0x7f800000u);
    // an id outside the cloud cannot come from a frame of this cloud: the pixel counts as empty, nothing is read
    if (!empty && id >= 0 && (long long)id < n) w = clip_w(cam.m, xyz[3ll * id], xyz[3ll * id + 1], xyz[3ll * id + 2]);
    near[p] = w;
}

__global__ __launch_bounds__(256) void select_vote_kernel(const float *__restrict__ xyz, long long n, Cam1 cam, int W, int H,
                                                          const float *__restrict__ near, const int32_t *__restrict__ mask,
                                                          float scale, float slack, uint32_t *__restrict__ state)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
    float d;
    int xx, yy;
    const int pix = project_one(x, y, z, cam.m, W, H, d, xx, yy);
    if (pix < 0) return;                                     // out of view: this view says nothing about the point
    const float lim = near[pix] * scale + slack;
    if (!(clip_w(cam.m, x, y, z) <= lim)) return;            // occluded (or NaN)
    const uint32_t m = (uint32_t)mask[pix];
    uint32_t s = state[i];
    uint32_t cand = s >> 16, hit = (s >> 8) & 0xffu, seen = s & 0xffu;
    seen += 1;
    if (m != 0u) {
        if (cand == 0u) {
            cand = m;
            hit = 1;
        } else if (m == cand) {
            hit += 1;
        }
    }
    state[i] = cand << 16 | hit << 8 | seen;
}

__global__ __launch_bounds__(256) void select_finish_kernel(const uint32_t *__restrict__ state, long long n, int min_hits, int num,
                                                            int den, const int32_t *labels_in, int32_t *labels_out)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t s = state[i];
    const long long cand = s >> 16, hit = (s >> 8) & 0xffu, seen = s & 0xffu;
    const bool keep = (cand != 0) & (hit >= min_hits) & (hit * den >= (long long)num * seen);
    labels_out[i] = keep ? (int32_t)cand : (labels_in ? labels_in[i] : 0);
}

// one item per thread; n < 2^31 * 256 keeps the grid inside gridDim.x
constexpr int64_t MAX_ITEMS = ((int64_t)1 << 31) * 256 - 256;

}  // namespace

extern "C" int read_select_boxes(const float *xyz, int64_t n, const float *boxes, const int32_t *label_of, int K,
                                 const int32_t *labels_in, int32_t *labels_out, void *stream)
{
    READ_CHECK_ARG(n >= 0, "read_select_boxes: n = %lld", (long long)n);
    READ_CHECK_ARG(K >= 0 && K <= MAX_BOXES, "read_select_boxes: K = %d outside [0, %d]", K, MAX_BOXES);
    READ_CHECK_ARG(n == 0 || (xyz && labels_out), "read_select_boxes: null pointer (xyz / labels_out)");
    READ_CHECK_ARG(n == 0 || K == 0 || (boxes && label_of), "read_select_boxes: null pointer (boxes / label_of) with K = %d", K);
    if (n == 0) return READ_OK;
    hipStream_t s = as_stream(stream);
    if (K == 0) {
        if (!labels_in)
            READ_CHECK_HIP(hipMemsetAsync(labels_out, 0, (size_t)n * sizeof(int32_t), s));
        else if (labels_in != labels_out)
            READ_CHECK_HIP(hipMemcpyAsync(labels_out, labels_in, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
        return READ_OK;
    }
    int64_t blocks = ceil_div64(n, 256);
    if (blocks > (int64_t)device_cus() * 8) blocks = (int64_t)device_cus() * 8;      // grid-stride: the staging is paid once per block
    const size_t lds = (size_t)K * (BOX_FLOATS * sizeof(float) + sizeof(int32_t));
    hipLaunchKernelGGL(select_boxes_kernel, dim3((unsigned)blocks), dim3(256), lds, s, xyz, (long long)n, boxes, label_of, K,
                       labels_in, labels_out);
    READ_CHECK_LAUNCH();
    return READ_OK;
}

extern "C" int read_select_near(const float *xyz, int64_t n, const float *M_host, int W, int H, const int32_t *idx0,
                                const float *depth0, float *near, void *stream)
{
    READ_CHECK_ARG(n >= 0 && n <= MAX_ITEMS, "read_select_near: n = %lld", (long long)n);
    READ_CHECK_ARG(M_host, "read_select_near: M_host is null");
    READ_CHECK_ARG(W >= 1 && H >= 1 && (long long)W * H < (1ll << 31), "read_select_near: bad W/H (%d,%d)", W, H);
    READ_CHECK_ARG(n == 0 || (xyz && idx0 && depth0 && near), "read_select_near: null pointer");
    if (n == 0) return READ_OK;
    Cam1 cam;
    for (int i = 0; i < 16; ++i) cam.m[i] = M_host[i];
    const long long pixels = (long long)W * H;
    hipLaunchKernelGGL(select_near_kernel, dim3((unsigned)ceil_div64(pixels, 256)), dim3(256), 0, as_stream(stream), xyz,
                       (long long)n, cam, pixels, idx0, depth0, near);
    READ_CHECK_LAUNCH();
    return READ_OK;
}

extern "C" int read_select_vote(const float *xyz, int64_t n, const float *M_host, int W, int H, const float *near,
                                const int32_t *mask, float scale, float slack, uint32_t *state, void *stream)
{
    READ_CHECK_ARG(n >= 0 && n <= MAX_ITEMS, "read_select_vote: n = %lld", (long long)n);
    READ_CHECK_ARG(M_host, "read_select_vote: M_host is null");
    READ_CHECK_ARG(W >= 1 && H >= 1 && (long long)W * H < (1ll << 31), "read_select_vote: bad W/H (%d,%d)", W, H);
    // written so that a NaN fails: scale in [1, inf), slack in [0, inf)
    READ_CHECK_ARG(scale >= 1.0f && scale <= 3.402823466e38f, "read_select_vote: scale = %g (finite, >= 1)", (double)scale);
    READ_CHECK_ARG(slack >= 0.0f && slack <= 3.402823466e38f, "read_select_vote: slack = %g (finite, >= 0)", (double)slack);
    READ_CHECK_ARG(n == 0 || (xyz && near && mask && state), "read_select_vote: null pointer");
    if (n == 0) return READ_OK;
    Cam1 cam;
    for (int i = 0; i < 16; ++i) cam.m[i] = M_host[i];
    hipLaunchKernelGGL(select_vote_kernel, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, as_stream(stream), xyz, (long long)n,
                       cam, W, H, near, mask, scale, slack, state);
    READ_CHECK_LAUNCH();
    return READ_OK;
}

extern "C" int read_select_finish(const uint32_t *state, int64_t n, int min_hits, int num, int den, const int32_t *labels_in,
                                  int32_t *labels_out, void *stream)
{
    READ_CHECK_ARG(n >= 0 && n <= MAX_ITEMS, "read_select_finish: n = %lld", (long long)n);
    READ_CHECK_ARG(min_hits >= 1 && min_hits <= 255, "read_select_finish: min_hits = %d outside [1, 255]", min_hits);
    READ_CHECK_ARG(den >= 1, "read_select_finish: den = %d < 1", den);
    READ_CHECK_ARG(num >= 0 && num <= den, "read_select_finish: num = %d outside [0, den = %d]", num, den);
    READ_CHECK_ARG(n == 0 || (state && labels_out), "read_select_finish: null pointer (state / labels_out)");
    if (n == 0) return READ_OK;
    hipLaunchKernelGGL(select_finish_kernel, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, as_stream(stream), state,
                       (long long)n, min_hits, num, den, labels_in, labels_out);
    READ_CHECK_LAUNCH();
    return READ_OK;
}
