// Frame annotations for gfx950: which object and which instance drew each pixel of an edited level-0 frame, and per-instance 2-D
// boxes, counts and nearest depth (the contract is tests/annotate_model.py, held bit for bit).
//
//   annotate_init_kernel     the statistics rows (zeros, INT32_MAX, -1 and n_pts: no memset writes all of them) and the counter
//   annotate_pixels_kernel   one lane per pixel (pixel_tables.h, shared with flow.hip): id -> object through the labels / the foreign ranges, then the first instance of that
//                            object whose matrix puts the point on this pixel at this depth; 16 B per pixel; the visible statistics go
//                            out once per wave and instance, not once per pixel
//   annotate_extents_kernel  the shape of range_splat_kernel<PinholeCam>: <= 32 ranges per launch, four points per thread; a workgroup reduces
//                            count, box and nearest depth and issues one set of atomics; 12 B per drawn point
//
// The match is exact because project_one here is the frame's device function on the same matrix bits.  Compiled with
// -ffp-contract=off.  Everything is integer min / max / add: the result does not depend on the order of execution.
#include "common.h"
#include "internal.h"

#pragma clang fp contract(off)

#include "pixel_tables.h"
#include "project.h"

using namespace readhip;

namespace {

constexpr int STATS = READ_ANNOTATE_STATS;
constexpr int MAX_FOREIGN = PIXEL_MAX_FOREIGN;
constexpr int32_t I32_MAX = 0x7fffffff;
// stats row: 0 vis_px | 1 vx0 2 vy0 3 vx1 4 vy1 | 5 in_pts | 6 ax0 7 ay0 8 ax1 9 ay1 | 10 near_bits | 11 n_pts

__global__ __launch_bounds__(256) void annotate_init_kernel(int32_t *__restrict__ stats, const int32_t *__restrict__ npts, int count,
                                                            int32_t *__restrict__ unmatched)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i == 0) *unmatched = 0;
    if (i >= count) return;
    int32_t *s = stats + (size_t)i * STATS;
    s[0] = 0;
    s[1] = I32_MAX; s[2] = I32_MAX; s[3] = -1; s[4] = -1;
    s[5] = 0;
    s[6] = I32_MAX; s[7] = I32_MAX; s[8] = -1; s[9] = -1;
    s[10] = I32_MAX;
    s[11] = npts[i];
}

__device__ __forceinline__ int wave_min(int v)
{
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_max(int v)
{
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

__global__ __launch_bounds__(256) void annotate_pixels_kernel(const float *__restrict__ xyz, long long n,
                                                              const int32_t *__restrict__ labels, const float *__restrict__ pool_xyz,
                                                              ForeignRanges fr, PixelTables tb, const int32_t *__restrict__ idx0,
                                                              const float *__restrict__ depth0, int W, int H, long long pixels,
                                                              int32_t *__restrict__ out_obj, int32_t *__restrict__ out_inst,
                                                              int32_t *__restrict__ stats, int32_t *__restrict__ unmatched)
{
    const long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool live = p < pixels;
    int obj = -1, value = -1, won = -1;                       // won: list position of the matching instance
    bool lost = false;
    if (live) {
        const int32_t id = idx0[p];
        const uint32_t dbits = __float_as_uint(depth0[p]);
        if (!((id == 0) & (dbits == 0u))) {
            const float *pt;
            const int k = pixel_object(id, xyz, n, labels, pool_xyz, fr, tb.K_own, pt);
            if (k < 0) {
                lost = true;
            } else if (k == 0) {
                obj = 0;
            } else {
                obj = k;
                won = pixel_drawer(tb, k, pt, p, dbits, W, H);
                if (won >= 0) value = tb.value[won];
                lost = won < 0;
            }
        }
        out_obj[p] = obj;
        out_inst[p] = value;
    }
    // visible statistics, one atomic set per wave and instance: the lowest lane that still has an instance names it, every lane of
    // that instance joins a wave reduction of count and box, the lane that named it issues the set.  (One set per RUN of equal
    // instances degenerates where copies interleave: a run is then one pixel long and every set lands on one of I cache lines — with
    // a peek in front of every bound, over a millisecond at 1216x352 on 16 interleaved copies, profiles/README.md.)  A wave may span two image rows (80-wide rows): x and
    // y reduce apart.
    const int lane = (int)(threadIdx.x & 63u);
    const int xcol = live ? (int)(p % W) : 0, yrow = live ? (int)(p / W) : 0;
    unsigned long long todo = __ballot(won >= 0);
    while (todo != 0ull) {
        const int leader = __ffsll((long long)todo) - 1;
        const int w = __shfl(won, leader);
        const bool mine = won == w;
        const unsigned long long members = __ballot(mine);
        todo &= ~members;                                     // the leader is a member: todo shrinks every turn
        const int x0 = wave_min(mine ? xcol : I32_MAX), y0 = wave_min(mine ? yrow : I32_MAX);
        const int x1 = wave_max(mine ? xcol : -1), y1 = wave_max(mine ? yrow : -1);
        if (lane == leader) {
            int32_t *s = stats + (size_t)w * STATS;
            atomicAdd(s + 0, (int)__popcll(members));
            atomicMin(s + 1, x0);
            atomicMin(s + 2, y0);
            atomicMax(s + 3, x1);
            atomicMax(s + 4, y1);
        }
    }
    const unsigned long long losers = __ballot(lost);
    if (losers != 0ull && lane == 0) atomicAdd(unmatched, (int)__popcll(losers));
}

constexpr int EXT_MAX = 32;
constexpr int EXT_PTS = 4;                           // points per thread: a workgroup covers 1024 points and issues one atomic set
struct ExtBatch {
    float m[EXT_MAX][16];
    long long first[EXT_MAX], last[EXT_MAX];        // range k = pool points [first, last)
    int block0[EXT_MAX + 1];                        // first workgroup of range k; block0[count] = the grid
    int row[EXT_MAX];                               // its statistics row (list position)
    int count;
};

__global__ __launch_bounds__(256) void annotate_extents_kernel(const float *__restrict__ pool_xyz, ExtBatch eb, int W, int H,
                                                               int32_t *__restrict__ stats)
{
    __shared__ int red[4][6];
    const int b = (int)blockIdx.x;
    int j = 0;
    for (int k = 1; k < eb.count; ++k)
        if (b >= eb.block0[k]) j = k;
    const long long i0 = eb.first[j] + (long long)(b - eb.block0[j]) * (256 * EXT_PTS) + threadIdx.x;
    int x0 = I32_MAX, y0 = I32_MAX, x1 = -1, y1 = -1, nb = I32_MAX, cnt = 0;
#pragma unroll
    for (int q = 0; q < EXT_PTS; ++q) {
        const long long i = i0 + q * 256;
        bool in = false;
        if (i < eb.last[j]) {
            float d;
            int xx, yy;
            const int pix = project_one(pool_xyz[3 * i], pool_xyz[3 * i + 1], pool_xyz[3 * i + 2], eb.m[j], W, H, d, xx, yy);
            if (pix >= 0) {
                in = true;
                x0 = min(x0, xx); x1 = max(x1, xx);
                y0 = min(y0, yy); y1 = max(y1, yy);
                nb = min(nb, (int)__float_as_uint(d));
            }
        }
        cnt += (int)__popcll(__ballot(in));
    }
    x0 = wave_min(x0);
    y0 = wave_min(y0);
    x1 = wave_max(x1);
    y1 = wave_max(y1);
    nb = wave_min(nb);
    const int wave = (int)(threadIdx.x >> 6);
    if ((threadIdx.x & 63u) == 0) {
        red[wave][0] = cnt; red[wave][1] = x0; red[wave][2] = y0; red[wave][3] = x1; red[wave][4] = y1; red[wave][5] = nb;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int c = 0;
        x0 = y0 = nb = I32_MAX;
        x1 = y1 = -1;
        for (int w = 0; w < 4; ++w) {
            c += red[w][0];
            x0 = min(x0, red[w][1]); y0 = min(y0, red[w][2]);
            x1 = max(x1, red[w][3]); y1 = max(y1, red[w][4]);
            nb = min(nb, red[w][5]);
        }
        if (c > 0) {
            int32_t *s = stats + (size_t)eb.row[j] * STATS;
            atomicAdd(s + 5, c);
            atomicMin(s + 6, x0);
            atomicMin(s + 7, y0);
            atomicMax(s + 8, x1);
            atomicMax(s + 9, y1);
            atomicMin(s + 10, nb);
        }
    }
}

int extents_flush(ExtBatch &eb, int &blocks, const float *pool_xyz, int W, int H, int32_t *stats, hipStream_t stream)
{
    if (eb.count == 0) return READ_OK;
    eb.block0[eb.count] = blocks;
    hipLaunchKernelGGL(annotate_extents_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, pool_xyz, eb, W, H, stats);
    READ_CHECK_LAUNCH();
    eb.count = 0;
    blocks = 0;
    return READ_OK;
}

}  // namespace

extern "C" int read_annotate_frame(const read_annotate_args *a, void *stream)
{
    READ_CHECK_ARG(a, "read_annotate_frame: args is null");
    READ_CHECK_ARG(a->W >= 1 && a->H >= 1 && (long long)a->W * a->H < (1ll << 31), "read_annotate_frame: bad W/H (%d,%d): W * H < 2^31",
                   a->W, a->H);
    READ_CHECK_ARG(a->n >= 0 && a->n <= (int64_t)I32_MAX, "read_annotate_frame: n = %lld", (long long)a->n);
    READ_CHECK_ARG(a->K_own >= 0, "read_annotate_frame: K_own = %d", a->K_own);
    READ_CHECK_ARG(a->count >= 0, "read_annotate_frame: count = %d", a->count);
    READ_CHECK_ARG(a->pool_n >= 0 && a->pool_n <= (int64_t)I32_MAX, "read_annotate_frame: pool_n = %lld", (long long)a->pool_n);
    READ_CHECK_ARG(a->n_foreign >= 0 && a->n_foreign <= MAX_FOREIGN, "read_annotate_frame: n_foreign = %d outside [0, %d]",
                   a->n_foreign, MAX_FOREIGN);
    READ_CHECK_ARG(a->idx0 && a->depth0 && a->out_obj && a->out_inst && a->unmatched,
                   "read_annotate_frame: null pointer (idx0 / depth0 / out_obj / out_inst / unmatched)");
    READ_CHECK_ARG(a->n == 0 || a->xyz, "read_annotate_frame: xyz is null with n = %lld", (long long)a->n);
    READ_CHECK_ARG(a->n_foreign == 0 || (a->foreign && a->pool_xyz), "read_annotate_frame: null pointer (foreign / pool_xyz) with "
                   "n_foreign = %d", a->n_foreign);
    ForeignRanges fr;
    memset(&fr, 0, sizeof(fr));
    fr.count = a->n_foreign;
    int64_t at = a->n;
    for (int f = 0; f < a->n_foreign; ++f) {
        const read_annotate_foreign &g = a->foreign[f];
        READ_CHECK_ARG(g.n >= 0 && g.id_base >= at && g.id_base + g.n <= (int64_t)I32_MAX,
                       "read_annotate_frame: foreign range %d = [%lld, +%lld): bases ascend from n = %lld without overlap, ids stay in int32",
                       f, (long long)g.id_base, (long long)g.n, (long long)a->n);
        READ_CHECK_ARG(g.pool_first >= 0 && g.pool_first + g.n <= a->pool_n,
                       "read_annotate_frame: foreign range %d: pool points [%lld, +%lld) past the pool of %lld", f,
                       (long long)g.pool_first, (long long)g.n, (long long)a->pool_n);
        fr.base[f] = g.id_base;
        fr.n[f] = g.n;
        fr.first[f] = g.pool_first;
        at = g.id_base + g.n;
    }
    const int K = a->K_own + a->n_foreign;
    if (a->count > 0) {
        READ_CHECK_ARG(a->first && a->npts && a->obj && a->M, "read_annotate_frame: null host table (first / npts / obj / M) with count = %d",
                       a->count);
        READ_CHECK_ARG(a->d_M && a->d_visible && a->d_value && a->d_npts && a->d_obj_begin && a->d_obj_list && a->stats,
                       "read_annotate_frame: null device table (d_M / d_visible / d_value / d_npts / d_obj_begin / d_obj_list / stats) "
                       "with count = %d", a->count);
        for (int i = 0; i < a->count; ++i) {
            READ_CHECK_ARG(a->obj[i] >= 1 && a->obj[i] <= K, "read_annotate_frame: instance %d draws object %d outside [1, %d]", i,
                           a->obj[i], K);
            READ_CHECK_ARG(a->first[i] >= 0 && a->npts[i] >= 0, "read_annotate_frame: instance %d: first = %lld, npts = %lld", i,
                           (long long)a->first[i], (long long)a->npts[i]);
            READ_CHECK_ARG(a->first[i] + a->npts[i] <= a->pool_n, "read_annotate_frame: instance %d: first + npts = %lld past the pool "
                           "of %lld", i, (long long)(a->first[i] + a->npts[i]), (long long)a->pool_n);
            READ_CHECK_ARG(a->npts[i] == 0 || a->pool_xyz, "read_annotate_frame: pool_xyz is null with points to draw");
        }
    }
    hipStream_t s = as_stream(stream);
    hipLaunchKernelGGL(annotate_init_kernel, dim3((unsigned)ceil_div(a->count > 0 ? a->count : 1, 256)), dim3(256), 0, s, a->stats,
                       a->d_npts, a->count, a->unmatched);
    READ_CHECK_LAUNCH();
    PixelTables tb;
    tb.M = a->d_M;
    tb.visible = a->d_visible;
    tb.value = a->d_value;
    tb.obj_begin = a->d_obj_begin;
    tb.obj_list = a->d_obj_list;
    tb.count = a->count;
    tb.K = K;
    tb.K_own = a->K_own;
    const long long pixels = (long long)a->W * a->H;
    hipLaunchKernelGGL(annotate_pixels_kernel, dim3((unsigned)ceil_div64(pixels, 256)), dim3(256), 0, s, a->xyz, (long long)a->n,
                       a->labels, a->pool_xyz, fr, tb, a->idx0, a->depth0, a->W, a->H, pixels, a->out_obj, a->out_inst, a->stats,
                       a->unmatched);
    READ_CHECK_LAUNCH();
    ExtBatch eb;
    memset(&eb, 0, sizeof(eb));
    int blocks = 0, rc;
    for (int i = 0; i < a->count; ++i) {
        if ((a->visible && !a->visible[i]) || a->npts[i] == 0) continue;             // hidden or empty: not launched
        const int k = eb.count++;
        memcpy(eb.m[k], a->M + 16 * (size_t)i, sizeof(eb.m[k]));
        eb.first[k] = a->first[i];
        eb.last[k] = a->first[i] + a->npts[i];
        eb.block0[k] = blocks;
        eb.row[k] = i;
        blocks += (int)ceil_div64(a->npts[i], 256 * EXT_PTS);
        if (eb.count == EXT_MAX && (rc = extents_flush(eb, blocks, a->pool_xyz, a->W, a->H, a->stats, s)) != READ_OK) return rc;
    }
    return extents_flush(eb, blocks, a->pool_xyz, a->W, a->H, a->stats, s);
}
