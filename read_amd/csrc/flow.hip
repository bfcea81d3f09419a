// Frame flow for gfx950: where each pixel's surface point of an edited level-0 frame goes in the next frame — optical flow, the depth
// there, and whether it is still seen, covered, beside the image, cut by a plane or hidden (the contract is
// tests/flow_model.py, held bit for bit).
//
//   flow_init_kernel     the eight state counts, the statistics rows and the counter: every value is 0
//   flow_pixels_kernel   one lane per pixel of frame A, 256 pixels per workgroup and turn, at most 512 workgroups: id -> object and
//                        point, then the drawer as the annotation finds it (pixel_tables.h; the static scene's two matrices travel
//                        in the kernel arguments, so a static pixel reads no table), the point
//                        under the drawer's matrix in A and in B, and B's key test at the pixel it lands on; 8 B read and 16 B written per
//                        pixel, the flow as one 8-byte store; the state counts (one ballot and popcount per state and wave) go out once per
//                        workgroup, the per-instance rows once per wave, turn and instance (the annotation's leader loop)
//
// The labels are exact because project_one_subpixel is the frame's device function on the same matrix bits.  Compiled with
// -ffp-contract=off.  Every counter is an integer add: the result does not depend on the order of execution.
#include "common.h"
#include "internal.h"

#pragma clang fp contract(off)

#include "pixel_tables.h"
#include "project.h"

using namespace readhip;

namespace {

constexpr int STATES = READ_FLOW_STATES;
constexpr int STATS = READ_FLOW_STATS;
constexpr int32_t I32_MAX = 0x7fffffff;
// stats row: 0 px | 1 visible | 2 occluded | 3 outside
constexpr int MAX_BLOCKS = 512;                               // two workgroups per CU; a larger frame takes more turns per workgroup

struct Mat16 {
    float m[16];
    __device__ __forceinline__ float operator[](int i) const { return m[i]; }
};

__global__ __launch_bounds__(256) void flow_init_kernel(int32_t *__restrict__ counts, int32_t *__restrict__ stats, int n_stats,
                                                        int32_t *__restrict__ unmatched)
{
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i == 0) *unmatched = 0;
    if (i < STATES) counts[i] = 0;
    if (i < n_stats) stats[i] = 0;
}

__global__ __launch_bounds__(256) void flow_pixels_kernel(const float *__restrict__ xyz, long long n, const int32_t *__restrict__ labels,
                                                          const float *__restrict__ pool_xyz, ForeignRanges fr, PixelTables tb,
                                                          const float *__restrict__ M_next, const int32_t *__restrict__ visible_next,
                                                          Mat16 M0a, Mat16 M0b, const int32_t *__restrict__ idx0,
                                                          const float *__restrict__ depth0, const int32_t *__restrict__ idx0_next,
                                                          const float *__restrict__ depth0_next, int W, int H, long long pixels,
                                                          float2 *__restrict__ flow, float *__restrict__ depth_next,
                                                          int32_t *__restrict__ state, int32_t *__restrict__ counts,
                                                          int32_t *__restrict__ stats, int32_t *__restrict__ unmatched)
{
    __shared__ int block_counts[READ_FLOW_UNMATCHED + 1];
    const int lane = (int)(threadIdx.x & 63u);
    int mine_count = 0;                                       // lane s < 7 of every wave keeps state s's count over the wave's pixels
    // a workgroup takes 256 pixels per turn; every lane of a wave stays in the loop to its end (the ballots want the whole wave)
    for (long long base = (long long)blockIdx.x * blockDim.x; base < pixels; base += (long long)gridDim.x * blockDim.x) {
        const long long p = base + threadIdx.x;
        const bool live = p < pixels;
        int st = -1, won = -1;                                // won: list position of the drawing instance
        if (live) {
            const int32_t id = idx0[p];
            const uint32_t dbits = __float_as_uint(depth0[p]);
            float fu = 0.0f, fv = 0.0f, dn = 0.0f;
            st = READ_FLOW_EMPTY;
            if (!((id == 0) & (dbits == 0u))) {
                st = READ_FLOW_UNMATCHED;
                const float *pt;
                const int k = pixel_object(id, xyz, n, labels, pool_xyz, fr, tb.K_own, pt);
                SubPixel a, b;
                bool drawn = false, hidden = false;
                if (k == 0) {
                    const float x = pt[0], y = pt[1], z = pt[2];
                    a = project_one_subpixel(x, y, z, M0a, W, H);
                    drawn = (long long)a.pix == p && __float_as_uint(a.depth) == dbits;
                    if (drawn) b = project_one_subpixel(x, y, z, M0b, W, H);
                } else if (k >= 1) {
                    won = pixel_drawer(tb, k, pt, p, dbits, W, H);
                    if (won >= 0) {
                        const float x = pt[0], y = pt[1], z = pt[2];
                        drawn = true;
                        a = project_one_subpixel(x, y, z, tb.M + 16 * (size_t)won, W, H);
                        b = project_one_subpixel(x, y, z, M_next + 16 * (size_t)won, W, H);
                        hidden = visible_next[won] == 0;
                    }
                }
                if (drawn) {
                    if (hidden) {
                        st = READ_FLOW_HIDDEN;
                    } else {
                        if (b.pix >= 0) {                          // b.pix < W * H: the projection accepts a point only inside the image
                            const bool same = idx0_next[b.pix] == id && __float_as_uint(depth0_next[b.pix]) == __float_as_uint(b.depth);
                            st = same ? READ_FLOW_VISIBLE : READ_FLOW_OCCLUDED;
                        } else {
                            const bool beside = b.nz >= -1.0f && b.nz <= 1.0f && fabsf(b.nx) < INFINITY && fabsf(b.ny) < INFINITY;
                            st = beside ? READ_FLOW_OFF_IMAGE : READ_FLOW_CLIPPED;
                        }
                        if (st != READ_FLOW_CLIPPED) {
                            fu = b.u - a.u;
                            fv = b.v - a.v;
                            dn = b.depth;
                        }
                    }
                }
            }
            flow[p] = make_float2(fu, fv);
            depth_next[p] = dn;
            state[p] = st;
        }
        // the state counts: one ballot and popcount per state
#pragma unroll
        for (int s = 0; s < READ_FLOW_UNMATCHED + 1; ++s) {
            const int c = (int)__popcll(__ballot(st == s));
            if (lane == s) mine_count += c;
        }
        // the per-instance rows, one atomic set per wave and instance (annotate.hip's leader loop): the lowest lane that still has an
        // instance names it, every lane of that instance joins the ballots, the lane that named it issues the adds that are not zero
        unsigned long long todo = __ballot(won >= 0);
        while (todo != 0ull) {
            const int leader = __ffsll((long long)todo) - 1;
            const int w = __shfl(won, leader);
            const bool mine = won == w;
            const unsigned long long members = __ballot(mine);
            todo &= ~members;                                     // the leader is a member: todo shrinks every turn
            const int vis = (int)__popcll(__ballot(mine && st == READ_FLOW_VISIBLE));
            const int occ = (int)__popcll(__ballot(mine && st == READ_FLOW_OCCLUDED));
            const int out = (int)__popcll(__ballot(mine && (st == READ_FLOW_OFF_IMAGE || st == READ_FLOW_CLIPPED)));
            if (lane == leader) {
                int32_t *s = stats + (size_t)w * STATS;
                atomicAdd(s + 0, (int)__popcll(members));
                if (vis) atomicAdd(s + 1, vis);
                if (occ) atomicAdd(s + 2, occ);
                if (out) atomicAdd(s + 3, out);
            }
        }
    }
    // the counts leave once per workgroup: the waves add theirs up in LDS, seven lanes issue the global adds that are not zero.  Every
    // add lands on ONE cache line and the memory side takes them one after another (about 12 ns each): one set per wave of a grid of
    // one lane per pixel cost 92 us at 1216x352 whatever the frame held (profiles/README.md), which is why the grid is capped.
    if (threadIdx.x <= READ_FLOW_UNMATCHED) block_counts[threadIdx.x] = 0;
    __syncthreads();
    if (lane <= READ_FLOW_UNMATCHED && mine_count != 0) atomicAdd(block_counts + lane, mine_count);
    __syncthreads();
    if (threadIdx.x <= READ_FLOW_UNMATCHED) {
        const int c = block_counts[threadIdx.x];
        if (c != 0) {
            atomicAdd(counts + threadIdx.x, c);
            if (threadIdx.x == READ_FLOW_UNMATCHED) atomicAdd(unmatched, c);
        }
    }
}

}  // namespace

extern "C" int read_flow_frame(const read_flow_args *a, void *stream)
{
    READ_CHECK_ARG(a, "read_flow_frame: args is null");
    READ_CHECK_ARG(a->W >= 1 && a->H >= 1 && (long long)a->W * a->H < (1ll << 31), "read_flow_frame: bad W/H (%d,%d): W * H < 2^31", a->W,
                   a->H);
    READ_CHECK_ARG(a->n >= 0 && a->n <= (int64_t)I32_MAX, "read_flow_frame: n = %lld", (long long)a->n);
    READ_CHECK_ARG(a->K_own >= 0, "read_flow_frame: K_own = %d", a->K_own);
    READ_CHECK_ARG(a->count >= 0, "read_flow_frame: count = %d", a->count);
    READ_CHECK_ARG(a->pool_n >= 0 && a->pool_n <= (int64_t)I32_MAX, "read_flow_frame: pool_n = %lld", (long long)a->pool_n);
    READ_CHECK_ARG(a->n_foreign >= 0 && a->n_foreign <= PIXEL_MAX_FOREIGN, "read_flow_frame: n_foreign = %d outside [0, %d]", a->n_foreign,
                   PIXEL_MAX_FOREIGN);
    READ_CHECK_ARG(a->idx0 && a->depth0 && a->idx0_next && a->depth0_next,
                   "read_flow_frame: null pointer (idx0 / depth0 / idx0_next / depth0_next)");
    READ_CHECK_ARG(a->flow && a->depth_next && a->state && a->counts && a->unmatched,
                   "read_flow_frame: null pointer (flow / depth_next / state / counts / unmatched)");
    READ_CHECK_ARG(((uintptr_t)a->flow & 7u) == 0, "read_flow_frame: flow is not 8-byte aligned");
    READ_CHECK_ARG(a->M0 && a->M0_next, "read_flow_frame: null pointer (M0 / M0_next)");
    READ_CHECK_ARG(a->n == 0 || a->xyz, "read_flow_frame: xyz is null with n = %lld", (long long)a->n);
    READ_CHECK_ARG(a->n_foreign == 0 || (a->foreign && a->pool_xyz), "read_flow_frame: null pointer (foreign / pool_xyz) with "
                   "n_foreign = %d", a->n_foreign);
    Mat16 M0a, M0b;
    for (int i = 0; i < 16; ++i) {
        READ_CHECK_ARG(std::isfinite(a->M0[i]), "read_flow_frame: M0[%d] is not finite", i);
        READ_CHECK_ARG(std::isfinite(a->M0_next[i]), "read_flow_frame: M0_next[%d] is not finite", i);
        M0a.m[i] = a->M0[i];
        M0b.m[i] = a->M0_next[i];
    }
    ForeignRanges fr;
    memset(&fr, 0, sizeof(fr));
    fr.count = a->n_foreign;
    int64_t at = a->n;
    for (int f = 0; f < a->n_foreign; ++f) {
        const read_annotate_foreign &g = a->foreign[f];
        READ_CHECK_ARG(g.n >= 0 && g.id_base >= at && g.id_base + g.n <= (int64_t)I32_MAX,
                       "read_flow_frame: foreign range %d = [%lld, +%lld): bases ascend from n = %lld without overlap, ids stay in int32", f,
                       (long long)g.id_base, (long long)g.n, (long long)a->n);
        READ_CHECK_ARG(g.pool_first >= 0 && g.pool_first + g.n <= a->pool_n,
                       "read_flow_frame: foreign range %d: pool points [%lld, +%lld) past the pool of %lld", f, (long long)g.pool_first,
                       (long long)g.n, (long long)a->pool_n);
        fr.base[f] = g.id_base;
        fr.n[f] = g.n;
        fr.first[f] = g.pool_first;
        at = g.id_base + g.n;
    }
    const int K = a->K_own + a->n_foreign;
    if (a->count > 0) {
        READ_CHECK_ARG(a->obj, "read_flow_frame: null host table (obj) with count = %d", a->count);
        READ_CHECK_ARG(a->d_M && a->d_visible && a->d_obj_begin && a->d_obj_list && a->d_M_next && a->d_visible_next && a->stats,
                       "read_flow_frame: null device table (d_M / d_visible / d_obj_begin / d_obj_list / d_M_next / d_visible_next / stats) "
                       "with count = %d", a->count);
        READ_CHECK_ARG((long long)a->count * STATS <= (long long)I32_MAX, "read_flow_frame: count = %d", a->count);
        for (int i = 0; i < a->count; ++i)
            READ_CHECK_ARG(a->obj[i] >= 1 && a->obj[i] <= K, "read_flow_frame: instance %d draws object %d outside [1, %d]", i, a->obj[i],
                           K);
    }
    hipStream_t s = as_stream(stream);
    const int n_stats = a->count * STATS;
    hipLaunchKernelGGL(flow_init_kernel, dim3((unsigned)ceil_div(n_stats > STATES ? n_stats : STATES, 256)), dim3(256), 0, s, a->counts,
                       a->stats, n_stats, a->unmatched);
    READ_CHECK_LAUNCH();
    PixelTables tb;
    tb.M = a->d_M;
    tb.visible = a->d_visible;
    tb.value = nullptr;
    tb.obj_begin = a->d_obj_begin;
    tb.obj_list = a->d_obj_list;
    tb.count = a->count;
    tb.K = K;
    tb.K_own = a->K_own;
    const long long pixels = (long long)a->W * a->H;
    const long long blocks = ceil_div64(pixels, 256);
    hipLaunchKernelGGL(flow_pixels_kernel, dim3((unsigned)(blocks < MAX_BLOCKS ? blocks : MAX_BLOCKS)), dim3(256), 0, s, a->xyz, (long long)a->n, a->labels,
                       a->pool_xyz, fr, tb, a->d_M_next, a->d_visible_next, M0a, M0b, a->idx0, a->depth0, a->idx0_next, a->depth0_next,
                       a->W, a->H, pixels, reinterpret_cast<float2 *>(a->flow), a->depth_next, a->state, a->counts, a->stats,
                       a->unmatched);
    READ_CHECK_LAUNCH();
    return READ_OK;
}
