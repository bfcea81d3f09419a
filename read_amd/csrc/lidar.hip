// LiDAR sweep: the range image and the return list of a spinning LiDAR placed in the fitted scene (read_lidar_sweep, DESIGN.md
// §10.7).  tests/lidar_model.py is the definition; this restates it bit for bit: fp32, no contraction (compiled with
// -ffp-contract=off), sums left to right, IEEE division, correctly rounded square root, the panorama's arctangent (project.h).
//
// A sweep is the pass (every range of points folded into the B x W key image by the 64-bit min the rasteriser uses) and three
// short dependent launches: filter + unpack + per-tile counts, one scan of the tile counts, scatter of the list + reset.  No
// kernel waits for another workgroup.  The workspace is [keys | filtered keys | tile counts | tile offsets], and every byte of it
// is 0xFF between sweeps (EMPTY keys; the scatter launch puts back what the sweep used), so the next sweep may have any size.
#include <cmath>

#include "internal.h"
#include "project.h"
#include "ranges.h"

namespace readhip {
namespace {

constexpr int LIDAR_MAX_BEAMS = 128;
constexpr int LIDAR_MAX_WINDOW = 4;
constexpr int LIDAR_TILE = 256;                      // cells per workgroup of the three image launches: one per lane
constexpr unsigned long long EMPTY = 0xFFFFFFFFFFFFFFFFull;

struct BeamTable {
    float e[LIDAR_MAX_BEAMS];
};
struct LidarCam {
    float m[16];
};
// The beam of elevation angle phi in the ascending table e[0..B) (LDS): lo = the number of entries below phi by a branch-free
// binary search, then the two neighbours lo - 1 and lo, the tie to the lower.  The model defines the beam by a linear scan for
// the first smallest d_b = |phi - e[b]|; fp32 subtraction is monotone, so d_b does not rise up to lo - 1 and does not fall from lo
// on, and the smallest is at one of the two.  Entries that round to the SAME d lie directly below lo - 1: the walk takes the first
// of them, which is the scan's tie rule (tests/test_lidar_cpu.py::test_beam_search_equals_the_linear_definition).  A NaN phi
// compares false throughout: b = 0, d = NaN, and the caller's d <= delta rejects it.
__device__ __forceinline__ int lidar_beam(float phi, const float *e, int B, float &d)
{
    int lo = 0;
#pragma unroll
    for (int step = LIDAR_MAX_BEAMS; step >= 1; step >>= 1) {
        const int t = lo + step;
        if (t <= B && e[t - 1] < phi) lo = t;
    }
    const int a = max(lo - 1, 0), b = min(lo, B - 1);
    const float da = fabsf(phi - e[a]), db = fabsf(phi - e[b]);
    int best = da <= db ? a : b;
    d = da <= db ? da : db;
    while (best > 0 && fabsf(phi - e[best - 1]) == d) --best;
    return best;
}

// One point under one LiDAR camera; returns the cell or -1.  NaN and Inf fall out through the comparisons.
__device__ __forceinline__ int lidar_project_one(float x, float y, float z, const float *c, const float *e, int B, int W, float &r)
{
    const float c0 = c[0] * x + c[1] * y + c[2] * z + c[3] * 1.0f;
    const float c1 = c[4] * x + c[5] * y + c[6] * z + c[7] * 1.0f;
    const float c3 = c[8] * x + c[9] * y + c[10] * z + c[11] * 1.0f;
    const float q = c0 * c0 + c3 * c3;
    const float rho = __builtin_sqrtf(q);
    const float theta = pano_atan2(c0, c3);
    const float phi = pano_atan2(c1, rho);
    r = __builtin_sqrtf(q + c1 * c1);
    const float nx = theta * c[12];
    const bool inside = (nx >= -1.0f) & (nx <= 1.0f);
    const float u = ((float)W * (nx + 1.0f)) * 0.5f;
    const int col = (int)u;
    bool ok = inside & (col >= 0) & (col < W) & (c[13] <= r) & (r <= c[14]);
    if (!ok) return -1;                              // most rejections end here, before the table is read
    float d;
    const int b = lidar_beam(phi, e, B, d);
    return d <= c[15] ? b * W + col : -1;
}

// range_splat_kernel's shape under LiDAR cameras: ob.m[k] holds range k's 16 camera floats, workgroup -> range from the host prefix
// (ranges.h).  The whole cloud (or a labelled cloud's static part) is one range; ids == NULL: the id is the point's index.  The
// beam table comes in the kernel arguments and is staged into LDS once per workgroup: the search indexes it per lane.
__global__ __launch_bounds__(256) void lidar_pass_kernel(const float *__restrict__ xyz, const int32_t *__restrict__ ids,
                                                         ObjBatch ob, BeamTable bt, int B, int W,
                                                         unsigned long long *__restrict__ keys)
{
    __shared__ float e[LIDAR_MAX_BEAMS];
    if (threadIdx.x < LIDAR_MAX_BEAMS) e[threadIdx.x] = bt.e[threadIdx.x];
    __syncthreads();
    const int b = (int)blockIdx.x, j = range_of_block(ob, b);
    const long long i = range_point(ob, j, b);
    if (i >= ob.last[j]) return;
    float r;
    const int cell = lidar_project_one(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], ob.m[j], e, B, W, r);
    if (cell < 0) return;
    const unsigned id = ids ? (unsigned)ids[i] : (unsigned)i;
    const unsigned long long key = ((unsigned long long)__float_as_uint(r) << 32) | id;
    unsigned long long *k = keys + cell;
    if (key < peek_key_agent(k)) fold_key_agent(k, key);         // keys only decrease: "not below what I see" is final
}

// The per-point function alone (read_lidar_project_points).
__global__ __launch_bounds__(256) void lidar_project_points_kernel(const float *__restrict__ xyz, long long n, LidarCam cam,
                                                                   BeamTable bt, int B, int W, int32_t *__restrict__ cell,
                                                                   float *__restrict__ range)
{
    __shared__ float e[LIDAR_MAX_BEAMS];
    if (threadIdx.x < LIDAR_MAX_BEAMS) e[threadIdx.x] = bt.e[threadIdx.x];
    __syncthreads();
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float r;
    const int c = lidar_project_one(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], cam.m, e, B, W, r);
    cell[i] = c;
    if (range) range[i] = c >= 0 ? r : 0.0f;
}

// The number of kept cells of this workgroup's tile before the calling lane's, and (total) in the whole tile.
__device__ __forceinline__ int tile_rank(bool kept, int &total)
{
    __shared__ int wave_count[LIDAR_TILE / 64];
    const unsigned long long mask = __ballot(kept);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_count[wave] = __popcll(mask);
    __syncthreads();
    int before = __popcll(mask & ((1ull << lane) - 1ull));
    total = 0;
    for (int w = 0; w < LIDAR_TILE / 64; ++w) {
        if (w < wave) before += wave_count[w];
        total += wave_count[w];
    }
    return before;
}

// See-through filter + unpack + tile counts, one lane per cell.  Reads the complete key image of the pass and writes elsewhere
// (fkeys, range, idx), so the rule does not depend on the order cells are visited in.  Range bits of positive floats order as
// unsigned integers and EMPTY's upper half is above all of them: near is a plain unsigned min over the window.
__global__ __launch_bounds__(LIDAR_TILE) void lidar_filter_kernel(const unsigned long long *__restrict__ keys, int B, int W, int wb,
                                                                  int wc, int wrap, float scale, float slack,
                                                                  unsigned long long *__restrict__ fkeys, float *__restrict__ range,
                                                                  int32_t *__restrict__ idx, unsigned *__restrict__ counts)
{
    const long long cells = (long long)B * W;
    const long long cell = (long long)blockIdx.x * LIDAR_TILE + threadIdx.x;
    bool kept = false;
    unsigned long long key = EMPTY;
    if (cell < cells) {
        key = keys[cell];
        if (key != EMPTY) {
            const int b = (int)(cell / W), c = (int)(cell - (long long)b * W);
            unsigned near = (unsigned)(key >> 32);
            const int b0 = max(b - wb, 0), b1 = min(b + wb, B - 1);
            for (int bb = b0; bb <= b1; ++bb)
                for (int dc = -wc; dc <= wc; ++dc) {
                    int cc = c + dc;
                    if (wrap) {
                        cc %= W;                     // |dc| <= 4 may exceed a tiny W: a true modulo
                        if (cc < 0) cc += W;
                    } else if (cc < 0 || cc >= W) {
                        continue;
                    }
                    near = min(near, (unsigned)(keys[(long long)bb * W + cc] >> 32));
                }
            const float lim = __uint_as_float(near) * scale + slack;
            kept = __uint_as_float((unsigned)(key >> 32)) <= lim;
        }
        if (!kept) key = EMPTY;
        fkeys[cell] = key;
        if (range) range[cell] = kept ? __uint_as_float((unsigned)(key >> 32)) : 0.0f;
        if (idx) idx[cell] = kept ? (int32_t)(unsigned)key : 0;
    }
    int total;
    tile_rank(kept, total);
    if (threadIdx.x == 0) counts[blockIdx.x] = (unsigned)total;
}

// Exclusive scan of the tile counts by ONE workgroup, 256 tiles a round with a running carry; *count = the sum.
__global__ __launch_bounds__(256) void lidar_scan_kernel(const unsigned *__restrict__ counts, int tiles, unsigned *__restrict__ offsets,
                                                         int32_t *__restrict__ count)
{
    __shared__ unsigned s[256];
    unsigned carry = 0;
    for (int base = 0; base < tiles; base += 256) {
        const int t = base + (int)threadIdx.x;
        const unsigned own = t < tiles ? counts[t] : 0u;
        s[threadIdx.x] = own;
        __syncthreads();
        for (int step = 1; step < 256; step <<= 1) {
            const unsigned add = threadIdx.x >= (unsigned)step ? s[threadIdx.x - step] : 0u;
            __syncthreads();
            s[threadIdx.x] += add;
            __syncthreads();
        }
        if (t < tiles) offsets[t] = carry + s[threadIdx.x] - own;
        carry += s[255];
        __syncthreads();
    }
    if (threadIdx.x == 0 && count) *count = (int32_t)carry;
}

// The return list in ascending cell order — tile offset + rank inside the tile, bounded by the capacity — and the reset: every
// word of the workspace this sweep used goes back to 0xFF.
__global__ __launch_bounds__(LIDAR_TILE) void lidar_scatter_kernel(unsigned long long *__restrict__ keys, unsigned long long *__restrict__ fkeys,
                                                                   unsigned *__restrict__ counts, unsigned *__restrict__ offsets, int B, int W,
                                                                   const float *__restrict__ beam_dir, const float *__restrict__ col_dir,
                                                                   int32_t *__restrict__ cell_out, int32_t *__restrict__ id_out,
                                                                   float *__restrict__ xyz_out, long long capacity)
{
    const long long cells = (long long)B * W;
    const long long cell = (long long)blockIdx.x * LIDAR_TILE + threadIdx.x;
    const unsigned long long key = cell < cells ? fkeys[cell] : EMPTY;
    const bool kept = key != EMPTY;
    int total;
    const long long pos = (long long)offsets[blockIdx.x] + tile_rank(kept, total);
    if (kept && pos < capacity) {
        if (cell_out) cell_out[pos] = (int32_t)cell;
        if (id_out) id_out[pos] = (int32_t)(unsigned)key;
        if (xyz_out) {
            const int b = (int)(cell / W), c = (int)(cell - (long long)b * W);
            const float r = __uint_as_float((unsigned)(key >> 32));
            const float h = r * beam_dir[2 * b];
            xyz_out[3 * pos] = h * col_dir[2 * c];
            xyz_out[3 * pos + 1] = r * beam_dir[2 * b + 1];
            xyz_out[3 * pos + 2] = -(h * col_dir[2 * c + 1]);
        }
    }
    if (cell < cells) {
        keys[cell] = EMPTY;
        fkeys[cell] = EMPTY;
    }
    __syncthreads();                                 // every lane has read offsets[blockIdx.x]
    if (threadIdx.x == 0) {
        counts[blockIdx.x] = 0xFFFFFFFFu;
        offsets[blockIdx.x] = 0xFFFFFFFFu;
    }
}

struct LidarLayout {
    unsigned long long *keys, *fkeys;
    unsigned *counts, *offsets;
    int tiles;
    size_t bytes;
};

LidarLayout lidar_layout(void *ws, int B, int W)
{
    const size_t cells = (size_t)B * (size_t)W;
    LidarLayout L;
    L.tiles = (int)((cells + LIDAR_TILE - 1) / LIDAR_TILE);
    char *p = (char *)ws;
    L.keys = (unsigned long long *)p;
    L.fkeys = L.keys + cells;
    L.counts = (unsigned *)(L.fkeys + cells);
    L.offsets = L.counts + L.tiles;
    L.bytes = (2 * cells * 8 + 2 * (size_t)L.tiles * 4 + 255) / 256 * 256;
    return L;
}

// the host-side conditions on the sensor: sizes, the beam table, the camera's 16 floats
int check_sensor(const char *who, const float *cam_host, const float *elev_host, int B, int W)
{
    READ_CHECK_ARG(cam_host && elev_host, "%s: null pointer (cam_host or elev_host)", who);
    READ_CHECK_ARG(B >= 1 && B <= LIDAR_MAX_BEAMS, "%s: B = %d beams, must be 1..%d", who, B, LIDAR_MAX_BEAMS);
    READ_CHECK_ARG(W >= 1 && (long long)B * W < (1ll << 31), "%s: bad size: B = %d, W = %d (W >= 1, B W < 2^31)", who, B, W);
    for (int b = 0; b < B; ++b) {
        READ_CHECK_ARG(std::isfinite(elev_host[b]), "%s: elev_host[%d] is not finite", who, b);
        READ_CHECK_ARG(b == 0 || elev_host[b] > elev_host[b - 1], "%s: elev_host is not strictly ascending at %d", who, b);
    }
    for (int i = 0; i < 16; ++i) READ_CHECK_ARG(std::isfinite(cam_host[i]), "%s: cam_host: a camera entry is not finite", who);
    READ_CHECK_ARG(cam_host[12] >= (float)(1.0 / 3.14159265358979323846),
                   "%s: cam_host: kx = 2 / hfov_rad must be >= 1 / pi (a field of at most 360 degrees)", who);
    READ_CHECK_ARG(cam_host[13] > 0.0f, "%s: cam_host: rmin must be > 0", who);
    READ_CHECK_ARG(cam_host[14] >= cam_host[13], "%s: cam_host: rmax must be >= rmin", who);
    READ_CHECK_ARG(cam_host[15] >= 0.0f, "%s: cam_host: delta (a beam's half-width) must be >= 0", who);
    return READ_OK;
}

// the instance list (check_instances, as read_splat_forward_pano_instances asks) and the 16 floats of every drawn instance
int check_lidar_instances(const char *who, const read_splat_instances *inst)
{
    if (const int rc = check_instances(who, inst); rc != READ_OK) return rc;
    return for_each_range(nullptr, inst, [&](int i, int64_t, int64_t, const float *M) -> int {
        for (int k = 0; k < 16; ++k)
            READ_CHECK_ARG(std::isfinite(M[k]), "%s: inst->M of instance %d: a camera entry is not finite", who, i);
        return READ_OK;
    });
}

}  // namespace
}  // namespace readhip

using namespace readhip;

extern "C" size_t read_lidar_workspace_bytes(int B, int W)
{
    if (B < 1 || B > LIDAR_MAX_BEAMS || W < 1 || (long long)B * W >= (1ll << 31)) return 0;
    return lidar_layout(nullptr, B, W).bytes;
}

extern "C" int read_lidar_workspace_init(void *ws, size_t ws_bytes, void *stream)
{
    READ_CHECK_ARG(ws && ws_bytes > 0, "read_lidar_workspace_init: null or empty workspace");
    READ_CHECK_ARG((uintptr_t)ws % 256 == 0, "read_lidar_workspace_init: workspace must be 256-byte aligned");
    READ_CHECK_HIP(hipMemsetAsync(ws, 0xFF, ws_bytes, as_stream(stream)));
    return READ_OK;
}

extern "C" int read_lidar_sweep(const read_lidar_args *a, void *stream)
{
    const char *who = "read_lidar_sweep";
    READ_CHECK_ARG(a, "%s: args is null", who);
    int rc = check_sensor(who, a->cam_host, a->elev_host, a->B, a->W);
    if (rc != READ_OK) return rc;
    READ_CHECK_ARG(a->n >= 0 && a->n <= 0xFFFFFFFEll, "%s: n out of range", who);
    READ_CHECK_ARG(a->n == 0 || a->xyz, "%s: null pointer (xyz)", who);
    if (a->inst && (rc = check_lidar_instances(who, a->inst)) != READ_OK) return rc;
    READ_CHECK_ARG(a->wb >= 0 && a->wb <= LIDAR_MAX_WINDOW && a->wc >= 0 && a->wc <= LIDAR_MAX_WINDOW,
                   "%s: the filter's window (wb, wc) = (%d, %d) must lie in 0..%d", who, a->wb, a->wc, LIDAR_MAX_WINDOW);
    READ_CHECK_ARG(std::isfinite(a->scale) && a->scale >= 1.0f, "%s: scale = %g must be finite and >= 1", who, (double)a->scale);
    READ_CHECK_ARG(std::isfinite(a->slack) && a->slack >= 0.0f, "%s: slack = %g must be finite and >= 0", who, (double)a->slack);
    READ_CHECK_ARG(a->capacity >= 0, "%s: capacity = %lld is negative", who, (long long)a->capacity);
    READ_CHECK_ARG(!(a->ret_xyz && a->capacity > 0) || (a->beam_dir && a->col_dir), "%s: null pointer (beam_dir or col_dir, with ret_xyz)", who);
    READ_CHECK_ARG(a->workspace, "%s: null pointer (workspace)", who);
    READ_CHECK_ARG((uintptr_t)a->workspace % 256 == 0, "%s: workspace must be 256-byte aligned", who);
    const LidarLayout L = lidar_layout(a->workspace, a->B, a->W);
    if (a->workspace_bytes < L.bytes) {
        set_error("%s: workspace %zu < %zu bytes", who, a->workspace_bytes, L.bytes);
        return READ_ENOMEM;
    }
    hipStream_t s = as_stream(stream);
    BeamTable bt;
    for (int b = 0; b < LIDAR_MAX_BEAMS; ++b) bt.e[b] = a->elev_host[b < a->B ? b : a->B - 1];
    // the pass: the static part, then every visible, non-empty instance, OBJ_MAX ranges per launch
    rc = launch_ranges(a->xyz, a->ids, a->n, a->cam_host, nullptr, a->inst,
                       [&](const ObjBatch &ob, int blocks, const float *xyz, const int32_t *ids) -> int {
                           hipLaunchKernelGGL(lidar_pass_kernel, dim3((unsigned)blocks), dim3(256), 0, s, xyz, ids, ob, bt, a->B, a->W, L.keys);
                           READ_CHECK_LAUNCH();
                           return READ_OK;
                       });
    if (rc != READ_OK) return rc;
    hipLaunchKernelGGL(lidar_filter_kernel, dim3((unsigned)L.tiles), dim3(LIDAR_TILE), 0, s, L.keys, a->B, a->W, a->wb, a->wc, a->wrap ? 1 : 0,
                       a->scale, a->slack, L.fkeys, a->range, a->idx, L.counts);
    READ_CHECK_LAUNCH();
    hipLaunchKernelGGL(lidar_scan_kernel, dim3(1), dim3(256), 0, s, L.counts, L.tiles, L.offsets, a->count);
    READ_CHECK_LAUNCH();
    hipLaunchKernelGGL(lidar_scatter_kernel, dim3((unsigned)L.tiles), dim3(LIDAR_TILE), 0, s, L.keys, L.fkeys, L.counts, L.offsets, a->B, a->W,
                       a->beam_dir, a->col_dir, a->cell, a->ret_id, a->ret_xyz, (long long)a->capacity);
    READ_CHECK_LAUNCH();
    return READ_OK;
}

extern "C" int read_lidar_project_points(const float *xyz, int64_t n, const float *cam_host, const float *elev_host, int B, int W,
                                         int32_t *cell, float *range, void *stream)
{
    const char *who = "read_lidar_project_points";
    READ_CHECK_ARG(n >= 0 && n <= 0xFFFFFFFEll && (n == 0 || (xyz && cell)), "%s: null pointer (xyz or cell), or n out of range", who);
    const int rc = check_sensor(who, cam_host, elev_host, B, W);
    if (rc != READ_OK) return rc;
    if (n == 0) return READ_OK;
    LidarCam cam;
    memcpy(cam.m, cam_host, sizeof(cam.m));
    BeamTable bt;
    for (int b = 0; b < LIDAR_MAX_BEAMS; ++b) bt.e[b] = elev_host[b < B ? b : B - 1];
    hipLaunchKernelGGL(lidar_project_points_kernel, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, as_stream(stream), xyz, (long long)n,
                       cam, bt, B, W, cell, range);
    READ_CHECK_LAUNCH();
    return READ_OK;
}
