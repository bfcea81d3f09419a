// Descriptor gather / scatter-add for gfx950.
//
// Replaces PointTexture.forward (READ/models/texture.py:42-70: index_select over a (C, B*N)
// channel-major table, i.e. C scattered 4-byte reads per pixel at stride 4*N bytes) with a
// row-major N x C table (32-byte rows at C = 8): one 16-byte load + one 16-byte NHWC store per
// lane, all pyramid levels in a single launch.  Background pixels carry id 0 and therefore
// receive descriptor[0], exactly as the reference (SURVEY.md "Empty pixels sample point 0").
// Backward = scatter-add of dL/dfeat into the rows (autograd of texture.py:61).
// HBM-bound: algorithmic bytes = sum_l px_l * (4 + 4C + 4C).
// Scene stitching (stitch_gather_kernel): the same gather over S parts' pyramids, the nearest part per pixel — 8S + 4C + 4C.
// Several tables behind one index image (gather_tables_kernel) and its adjoint (gather_tables_backward_kernel: 4 + 4C + 4C [+ 4C with an
// activation] per pixel in pairs mode) — what a stitched scene trains through.
#include "common.h"

using namespace readhip;

namespace {

struct LevelTable {
    const int32_t *idx[READ_MAX_LEVELS];
    float *feat[READ_MAX_LEVELS];
    long long end[READ_MAX_LEVELS];   // exclusive prefix end, in units of (pixel, quad) items
    int levels;
};

__device__ __forceinline__ float act_apply(float v, int activation)
{
    if (activation == 1) return 1.0f / (1.0f + expf(-v));
    if (activation == 2) return tanhf(v);
    return v;
}

// item = (pixel, quad of 4 channels); consecutive lanes -> consecutive quads of consecutive pixels,
// so the NHWC store is fully coalesced.
__global__ __launch_bounds__(256) void gather_forward_kernel(const float *__restrict__ rows, long long n, int C,
                                                             LevelTable tab, int activation)
{
    const int qpp = C >> 2;
    const long long total = tab.end[tab.levels - 1];
    for (long long item = (long long)blockIdx.x * blockDim.x + threadIdx.x; item < total;
         item += (long long)gridDim.x * blockDim.x) {
        int l = 0;
        long long base = 0;
#pragma unroll
        for (int k = 0; k < READ_MAX_LEVELS - 1; ++k)
            if (k < tab.levels - 1 && item >= tab.end[k]) { l = k + 1; base = tab.end[k]; }
        const long long local = item - base;
        const long long pix = local / qpp;
        const int q = (int)(local - pix * qpp);
        long long id = tab.idx[l][pix];
        id = id < 0 ? 0 : (id >= n ? n - 1 : id);   // defensive clamp; ids come from the rasteriser
        float4 v = *reinterpret_cast<const float4 *>(rows + id * C + 4 * q);
        if (activation) {
            v.x = act_apply(v.x, activation);
            v.y = act_apply(v.y, activation);
            v.z = act_apply(v.z, activation);
            v.w = act_apply(v.w, activation);
        }
        *reinterpret_cast<float4 *>(tab.feat[l] + pix * C + 4 * q) = v;
    }
}

// Supersampled lookup: index maps at ss x the output size; out = bilinear downscale (align_corners = False) of the activated
// samples — torch's F.interpolate(scale_factor = 1 / ss) as READ/models/compose.py:162-163 applies it to the texture samples.
struct LevelTableSS {
    const int32_t *idx[READ_MAX_LEVELS];
    float *feat[READ_MAX_LEVELS];
    long long end[READ_MAX_LEVELS];   // exclusive prefix end in (pixel, quad) items over all B images of a level
    int h[READ_MAX_LEVELS], w[READ_MAX_LEVELS];
    int levels;
};

__device__ __forceinline__ float4 act4(float4 v, int activation)
{
    if (activation) {
        v.x = act_apply(v.x, activation);
        v.y = act_apply(v.y, activation);
        v.z = act_apply(v.z, activation);
        v.w = act_apply(v.w, activation);
    }
    return v;
}

__global__ __launch_bounds__(256) void gather_forward_ss_kernel(const float *__restrict__ rows, long long n, int C,
                                                                LevelTableSS tab, int ss, int activation)
{
    const int qpp = C >> 2;
    const long long total = tab.end[tab.levels - 1];
    for (long long item = (long long)blockIdx.x * blockDim.x + threadIdx.x; item < total;
         item += (long long)gridDim.x * blockDim.x) {
        int l = 0;
        long long base = 0;
#pragma unroll
        for (int k = 0; k < READ_MAX_LEVELS - 1; ++k)
            if (k < tab.levels - 1 && item >= tab.end[k]) { l = k + 1; base = tab.end[k]; }
        const long long local = item - base;
        const long long pix = local / qpp;
        const int q = (int)(local - pix * qpp);
        const int h = tab.h[l], w = tab.w[l], sh = h * ss, sw = w * ss;
        const int ox = (int)(pix % w), oy = (int)((pix / w) % h);
        const long long b = pix / ((long long)w * h);
        // source coordinate (o + 0.5) * ss - 0.5 >= 0 for ss >= 1
        const float sy = ((float)oy + 0.5f) * (float)ss - 0.5f, sx = ((float)ox + 0.5f) * (float)ss - 0.5f;
        const int y0 = (int)sy, x0 = (int)sx;
        const int y1 = y0 + (y0 < sh - 1 ? 1 : 0), x1 = x0 + (x0 < sw - 1 ? 1 : 0);
        const float ly = sy - (float)y0, lx = sx - (float)x0;
        const int32_t *im = tab.idx[l] + b * (long long)sh * sw;
        float4 v[4];
        const int yy[4] = {y0, y0, y1, y1}, xx[4] = {x0, x1, x0, x1};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            long long id = im[(long long)yy[k] * sw + xx[k]];
            id = id < 0 ? 0 : (id >= n ? n - 1 : id);
            v[k] = act4(*reinterpret_cast<const float4 *>(rows + id * C + 4 * q), activation);
        }
        const float wy0 = 1.0f - ly, wx0 = 1.0f - lx;
        float4 o;
        o.x = wy0 * (wx0 * v[0].x + lx * v[1].x) + ly * (wx0 * v[2].x + lx * v[3].x);
        o.y = wy0 * (wx0 * v[0].y + lx * v[1].y) + ly * (wx0 * v[2].y + lx * v[3].y);
        o.z = wy0 * (wx0 * v[0].z + lx * v[1].z) + ly * (wx0 * v[2].z + lx * v[3].z);
        o.w = wy0 * (wx0 * v[0].w + lx * v[1].w) + ly * (wx0 * v[2].w + lx * v[3].w);
        // odd ss: the source coordinate is the centre sample itself.  The blend's zero-weight terms would turn a -0 sample into +0
        // and a non-finite neighbour into NaN; the sample is returned as it is (wave-uniform: ss is a kernel argument)
        if (ss & 1) o = v[0];
        *reinterpret_cast<float4 *>(tab.feat[l] + pix * C + 4 * q) = o;
    }
}

// Scene stitching: up to READ_STITCH_MAX_PARTS pyramids of local ids + depths -> per pixel the visible candidate with the smallest
// depth bit pattern (ties: the lowest part), its descriptor row from ITS table with ITS activation, and optionally the merged
// index / depth / part images.  Same item mapping as gather_forward_kernel; the tables travel by value in the kernel arguments.
struct StitchTable {
    const int32_t *idx[READ_STITCH_MAX_PARTS][READ_MAX_LEVELS];
    const float *depth[READ_STITCH_MAX_PARTS][READ_MAX_LEVELS];
    const float *rows[READ_STITCH_MAX_PARTS];
    long long n[READ_STITCH_MAX_PARTS];
    int id_base[READ_STITCH_MAX_PARTS];
    int act[READ_STITCH_MAX_PARTS];
    int32_t *out_idx[READ_MAX_LEVELS];        // each output: all levels set, or none (then the flag below is 0)
    float *out_depth[READ_MAX_LEVELS];
    unsigned char *out_part[READ_MAX_LEVELS];
    float *feat[READ_MAX_LEVELS];
    long long end[READ_MAX_LEVELS];
    unsigned visible;                         // bit s: part s has a pyramid (a hidden part has none and is never read)
    int levels, count;
    int want_idx, want_depth, want_part, want_feat;
};

__global__ __launch_bounds__(256) void stitch_gather_kernel(StitchTable tab, int C)
{
    const int qpp = C >> 2;
    const long long total = tab.end[tab.levels - 1];
    for (long long item = (long long)blockIdx.x * blockDim.x + threadIdx.x; item < total;
         item += (long long)gridDim.x * blockDim.x) {
        int l = 0;
        long long base = 0;
#pragma unroll
        for (int k = 0; k < READ_MAX_LEVELS - 1; ++k)
            if (k < tab.levels - 1 && item >= tab.end[k]) { l = k + 1; base = tab.end[k]; }
        const long long local = item - base;
        const long long pix = local / qpp;
        const int q = (int)(local - pix * qpp);
        // running winner by compare-and-select; the loop over parts is wave-uniform (count and visible are kernel arguments)
        int win = -1, win_id = 0;
        unsigned win_d = 0u;
        for (int s = 0; s < tab.count; ++s) {
            if (!((tab.visible >> s) & 1u)) continue;
            const int id = tab.idx[s][l][pix];
            const unsigned d = __float_as_uint(tab.depth[s][l][pix]);
            const bool take = ((unsigned)id | d) != 0u && (win < 0 || d < win_d);     // strict <: a tie stays with the lower part
            win = take ? s : win;
            win_id = take ? id : win_id;
            win_d = take ? d : win_d;
        }
        const int src = win < 0 ? 0 : win;                                            // no candidate: descriptor 0 of part 0
        const long long n = tab.n[src];
        long long id = win_id;
        id = id < 0 ? 0 : (id >= n ? n - 1 : id);   // defensive clamp; ids come from the rasteriser
        if (tab.want_feat) {
            const float4 v = act4(*reinterpret_cast<const float4 *>(tab.rows[src] + id * C + 4 * q), tab.act[src]);
            *reinterpret_cast<float4 *>(tab.feat[l] + pix * C + 4 * q) = v;
        }
        if (q == 0) {
            if (tab.want_idx) tab.out_idx[l][pix] = win < 0 ? 0 : tab.id_base[src] + (int)id;
            if (tab.want_depth) tab.out_depth[l][pix] = __uint_as_float(win_d);
            if (tab.want_part) tab.out_part[l][pix] = (unsigned char)(win < 0 ? 255 : win);
        }
    }
}

// The gather over several tables (read_gather_forward_tables): gather_forward_kernel's item mapping, loads and stores; the table list
// travels by value in the kernel arguments.  Table t serves ids in [base_t, base_t + n_t), bases ascending from 0: the table of an id
// is the LAST one whose base is <= id — a loop of compare-and-selects with a wave-uniform trip count, no divergent branch; the local id
// is clamped to [0, n_t) (an id in a gap or past the end reads its table's last row, an id below 0 row 0 of table 0: the plain
// kernel's defensive clamp, generalised).
struct GatherTables {
    const float *rows[READ_GATHER_MAX_TABLES];
    long long n[READ_GATHER_MAX_TABLES];
    long long base[READ_GATHER_MAX_TABLES];
    int act[READ_GATHER_MAX_TABLES];
    int count;
};

__global__ __launch_bounds__(256) void gather_tables_kernel(GatherTables tt, int C, LevelTable tab)
{
    const int qpp = C >> 2;
    const long long total = tab.end[tab.levels - 1];
    for (long long item = (long long)blockIdx.x * blockDim.x + threadIdx.x; item < total;
         item += (long long)gridDim.x * blockDim.x) {
        int l = 0;
        long long base = 0;
#pragma unroll
        for (int k = 0; k < READ_MAX_LEVELS - 1; ++k)
            if (k < tab.levels - 1 && item >= tab.end[k]) { l = k + 1; base = tab.end[k]; }
        const long long local = item - base;
        const long long pix = local / qpp;
        const int q = (int)(local - pix * qpp);
        const long long gid = tab.idx[l][pix];
        const float *rows = tt.rows[0];
        long long n = tt.n[0], b = 0;
        int act = tt.act[0];
        for (int t = 1; t < tt.count; ++t) {
            const bool take = gid >= tt.base[t];
            rows = take ? tt.rows[t] : rows;
            n = take ? tt.n[t] : n;
            b = take ? tt.base[t] : b;
            act = take ? tt.act[t] : act;
        }
        long long id = gid - b;
        id = id < 0 ? 0 : (id >= n ? n - 1 : id);
        const float4 v = act4(*reinterpret_cast<const float4 *>(rows + id * C + 4 * q), act);
        *reinterpret_cast<float4 *>(tab.feat[l] + pix * C + 4 * q) = v;
    }
}

// Bilinear down-scale by an integer factor of NCHW planes: torch's F.interpolate(scale_factor = 1 / ss, mode = 'bilinear',
// align_corners = False) as READ/models/compose.py:162-163 applies it to the concatenated (non-uv extras + texture sample)
// network inputs.  out[p][oy][ox] = blend of the 4 samples around ((o + 0.5) * ss - 0.5); lane = output pixel of a plane.
__global__ __launch_bounds__(256) void bilinear_down_kernel(const float *__restrict__ in, long long planes, int h, int w, int ss,
                                                            float *__restrict__ out)
{
    const long long total = planes * h * w;
    const int sh = h * ss, sw = w * ss;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int ox = (int)(i % w), oy = (int)((i / w) % h);
        const long long p = i / ((long long)w * h);
        const float sy = ((float)oy + 0.5f) * (float)ss - 0.5f, sx = ((float)ox + 0.5f) * (float)ss - 0.5f;
        const int y0 = (int)sy, x0 = (int)sx;
        const int y1 = y0 + (y0 < sh - 1 ? 1 : 0), x1 = x0 + (x0 < sw - 1 ? 1 : 0);
        const float ly = sy - (float)y0, lx = sx - (float)x0, wy0 = 1.0f - ly, wx0 = 1.0f - lx;
        const float *im = in + p * (long long)sh * sw;
        out[i] = wy0 * (wx0 * im[(long long)y0 * sw + x0] + lx * im[(long long)y0 * sw + x1]) +
                 ly * (wx0 * im[(long long)y1 * sw + x0] + lx * im[(long long)y1 * sw + x1]);
    }
}

// Its adjoint.  For ss >= 2 the 2x2 footprints of different outputs are disjoint, so the gradient of an input sample comes
// from at most one output: a gather, no atomics.  lane = input sample.
__global__ __launch_bounds__(256) void bilinear_down_backward_kernel(const float *__restrict__ dout, long long planes, int h, int w,
                                                                     int ss, float *__restrict__ din)
{
    const int sh = h * ss, sw = w * ss;
    const long long total = planes * sh * sw;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(i % sw), y = (int)((i / sw) % sh);
        const long long p = i / ((long long)sw * sh);
        const int oy = y / ss, ox = x / ss;
        const float sy = ((float)oy + 0.5f) * (float)ss - 0.5f, sx = ((float)ox + 0.5f) * (float)ss - 0.5f;
        const int y0 = (int)sy, x0 = (int)sx;
        const int y1 = y0 + (y0 < sh - 1 ? 1 : 0), x1 = x0 + (x0 < sw - 1 ? 1 : 0);
        const float ly = sy - (float)y0, lx = sx - (float)x0;
        float wy = 0.0f, wx = 0.0f;
        if (y == y0) wy += 1.0f - ly;
        if (y == y1) wy += ly;
        if (x == x0) wx += 1.0f - lx;
        if (x == x1) wx += lx;
        const float wgt = wy * wx;                  // 1/4 on the footprint of even ss, 1 on the centre of odd ss, 0 elsewhere
        din[i] = wgt != 0.0f ? wgt * dout[(p * h + oy) * w + ox] : 0.0f;   // +0 outside the footprint, whatever the sign of dout
    }
}

struct LevelTableBwd {
    const int32_t *idx[READ_MAX_LEVELS];
    const float *dfeat[READ_MAX_LEVELS];
    long long end[READ_MAX_LEVELS];
    int levels;
};

__global__ __launch_bounds__(256) void gather_backward_kernel(float *__restrict__ drows, long long n, int C,
                                                              LevelTableBwd tab)
{
    const int qpp = C >> 2;
    const long long total = tab.end[tab.levels - 1];
    for (long long item = (long long)blockIdx.x * blockDim.x + threadIdx.x; item < total;
         item += (long long)gridDim.x * blockDim.x) {
        int l = 0;
        long long base = 0;
#pragma unroll
        for (int k = 0; k < READ_MAX_LEVELS - 1; ++k)
            if (k < tab.levels - 1 && item >= tab.end[k]) { l = k + 1; base = tab.end[k]; }
        const long long local = item - base;
        const long long pix = local / qpp;
        const int q = (int)(local - pix * qpp);
        long long id = tab.idx[l][pix];
        id = id < 0 ? 0 : (id >= n ? n - 1 : id);
        const float4 g = *reinterpret_cast<const float4 *>(tab.dfeat[l] + pix * C + 4 * q);
        float *dst = drows + id * C + 4 * q;
        atomicAdd(dst + 0, g.x);
        atomicAdd(dst + 1, g.y);
        atomicAdd(dst + 2, g.z);
        atomicAdd(dst + 3, g.w);
    }
}

// The adjoint of gather_tables_kernel (read_gather_backward_tables): its item mapping, its table selection and its clamps, so the row
// addressed is the row the forward read.  g = dfeat * act'(y) from the forward's own output y; written per pixel (pairs: one 16-byte
// store per lane, no atomics) and / or added into the selected table's gradient rows (dense; a NULL table is frozen and skipped).
struct GatherTablesBwd {
    float *drows[READ_GATHER_MAX_TABLES];
    long long n[READ_GATHER_MAX_TABLES];
    long long base[READ_GATHER_MAX_TABLES];
    int act[READ_GATHER_MAX_TABLES];
    int count;
};

struct LevelTableBwdT {
    const int32_t *idx[READ_MAX_LEVELS];
    const float *dfeat[READ_MAX_LEVELS];
    const float *feat[READ_MAX_LEVELS];       // the forward's output; not read where the selected table's activation is 0
    float *g[READ_MAX_LEVELS];                // pairs mode: all levels set, or none (then want_pairs is 0)
    long long end[READ_MAX_LEVELS];
    int levels;
};

__device__ __forceinline__ float act_slope(float y, int activation)      // act'(x) from y = act(x)
{
    return activation == 1 ? y * (1.0f - y) : 1.0f - y * y;
}

__global__ __launch_bounds__(256) void gather_tables_backward_kernel(GatherTablesBwd tt, int C, LevelTableBwdT tab, int want_pairs,
                                                                     int want_dense)
{
    const int qpp = C >> 2;
    const long long total = tab.end[tab.levels - 1];
    for (long long item = (long long)blockIdx.x * blockDim.x + threadIdx.x; item < total;
         item += (long long)gridDim.x * blockDim.x) {
        int l = 0;
        long long base = 0;
#pragma unroll
        for (int k = 0; k < READ_MAX_LEVELS - 1; ++k)
            if (k < tab.levels - 1 && item >= tab.end[k]) { l = k + 1; base = tab.end[k]; }
        const long long local = item - base;
        const long long pix = local / qpp;
        const int q = (int)(local - pix * qpp);
        const long long gid = tab.idx[l][pix];
        float *drows = tt.drows[0];
        long long n = tt.n[0], b = 0;
        int act = tt.act[0];
        for (int t = 1; t < tt.count; ++t) {
            const bool take = gid >= tt.base[t];
            drows = take ? tt.drows[t] : drows;
            n = take ? tt.n[t] : n;
            b = take ? tt.base[t] : b;
            act = take ? tt.act[t] : act;
        }
        long long id = gid - b;
        id = id < 0 ? 0 : (id >= n ? n - 1 : id);
        float4 g = *reinterpret_cast<const float4 *>(tab.dfeat[l] + pix * C + 4 * q);
        if (act) {
            const float4 y = *reinterpret_cast<const float4 *>(tab.feat[l] + pix * C + 4 * q);
            g.x *= act_slope(y.x, act);
            g.y *= act_slope(y.y, act);
            g.z *= act_slope(y.z, act);
            g.w *= act_slope(y.w, act);
        }
        if (want_pairs) *reinterpret_cast<float4 *>(tab.g[l] + pix * C + 4 * q) = g;
        if (want_dense && drows) {
            float *dst = drows + id * C + 4 * q;
            atomicAdd(dst + 0, g.x);
            atomicAdd(dst + 1, g.y);
            atomicAdd(dst + 2, g.z);
            atomicAdd(dst + 3, g.w);
        }
    }
}

// (C, N) -> N x C: lane = point, C strided-but-coalesced loads, one contiguous row store.
__global__ __launch_bounds__(256) void texture_to_rows_kernel(const float *__restrict__ tex, long long n, int C,
                                                              float *__restrict__ rows)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int c = 0; c < C; c += 4) {
        float4 v;
        v.x = tex[(long long)(c + 0) * n + i];
        v.y = tex[(long long)(c + 1) * n + i];
        v.z = tex[(long long)(c + 2) * n + i];
        v.w = tex[(long long)(c + 3) * n + i];
        *reinterpret_cast<float4 *>(rows + i * C + c) = v;
    }
}

__global__ __launch_bounds__(256) void rows_to_texture_kernel(const float *__restrict__ rows, long long n, int C,
                                                              float *__restrict__ tex)
{
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int c = 0; c < C; c += 4) {
        const float4 v = *reinterpret_cast<const float4 *>(rows + i * C + c);
        tex[(long long)(c + 0) * n + i] = v.x;
        tex[(long long)(c + 1) * n + i] = v.y;
        tex[(long long)(c + 2) * n + i] = v.z;
        tex[(long long)(c + 3) * n + i] = v.w;
    }
}

int check_levels(const char *who, int64_t n, int C, int levels, const void *idx, const int64_t *count, const void *ptrs)
{
    READ_CHECK_ARG(n >= 1, "%s: empty descriptor table", who);
    READ_CHECK_ARG(C >= 4 && C % 4 == 0 && C <= 64, "%s: C must be a multiple of 4 in [4,64] (got %d)", who, C);
    READ_CHECK_ARG(levels >= 1 && levels <= READ_MAX_LEVELS, "%s: levels must be 1..%d", who, READ_MAX_LEVELS);
    READ_CHECK_ARG(idx && count && ptrs, "%s: null level table", who);
    return READ_OK;
}

// The table list of read_gather_forward_tables / read_gather_backward_tables: the id-range rule, checked once for both.  The backward
// never reads the rows (need_rows false).
int fill_tables(const char *who, const read_gather_table *tables, int count, GatherTables *tt, bool need_rows = true)
{
    memset(tt, 0, sizeof(*tt));
    for (int t = 0; t < count; ++t) {
        const read_gather_table &g = tables[t];
        READ_CHECK_ARG(!need_rows || (g.rows_nc && (uintptr_t)g.rows_nc % 16 == 0), "%s: table %d: rows null or misaligned", who, t);
        READ_CHECK_ARG(g.n >= 1, "%s: table %d: empty descriptor table", who, t);
        READ_CHECK_ARG(g.activation >= 0 && g.activation <= 2, "%s: table %d: activation must be 0,1,2", who, t);
        if (t == 0)
            READ_CHECK_ARG(g.id_base == 0, "%s: table 0: id_base must be 0 (got %lld)", who, (long long)g.id_base);
        else {
            READ_CHECK_ARG(g.id_base > tables[t - 1].id_base, "%s: table %d: id_base %lld does not ascend", who, t,
                           (long long)g.id_base);
            READ_CHECK_ARG(g.id_base >= tables[t - 1].id_base + tables[t - 1].n,
                           "%s: table %d: id_base %lld overlaps the range of table %d, which ends at %lld", who, t,
                           (long long)g.id_base, t - 1, (long long)(tables[t - 1].id_base + tables[t - 1].n));
        }
        READ_CHECK_ARG(g.id_base <= (int64_t)INT32_MAX && g.n <= (int64_t)INT32_MAX && g.id_base + g.n <= (int64_t)INT32_MAX,
                       "%s: table %d: id_base %lld + n %lld leaves the int32 id range", who, t, (long long)g.id_base, (long long)g.n);
        tt->rows[t] = g.rows_nc;
        tt->n[t] = g.n;
        tt->base[t] = g.id_base;
        tt->act[t] = g.activation;
    }
    tt->count = count;
    return READ_OK;
}

}  // namespace

extern "C" int read_texture_to_rows(const float *tex_cn, int64_t n, int C, float *rows_nc, void *stream)
{
    READ_CHECK_ARG(tex_cn && rows_nc && n >= 1, "read_texture_to_rows: null pointer or empty table");
    READ_CHECK_ARG(C >= 4 && C % 4 == 0, "read_texture_to_rows: C must be a multiple of 4");
    READ_CHECK_ARG((uintptr_t)rows_nc % 16 == 0, "read_texture_to_rows: rows must be 16-byte aligned");
    hipLaunchKernelGGL(texture_to_rows_kernel, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, as_stream(stream),
                       tex_cn, (long long)n, C, rows_nc);
    READ_CHECK_LAUNCH();
    return READ_OK;
}

extern "C" int read_rows_to_texture(const float *rows_nc, int64_t n, int C, float *tex_cn, void *stream)
{
    READ_CHECK_ARG(tex_cn && rows_nc && n >= 1, "read_rows_to_texture: null pointer or empty table");
    READ_CHECK_ARG(C >= 4 && C % 4 == 0, "read_rows_to_texture: C must be a multiple of 4");
    READ_CHECK_ARG((uintptr_t)rows_nc % 16 == 0, "read_rows_to_texture: rows must be 16-byte aligned");
    hipLaunchKernelGGL(rows_to_texture_kernel, dim3((unsigned)ceil_div64(n, 256)), dim3(256), 0, as_stream(stream),
                       rows_nc, (long long)n, C, tex_cn);
    READ_CHECK_LAUNCH();
    return READ_OK;
}

extern "C" int read_gather_forward(const float *rows_nc, int64_t n, int C, int levels,
                                   const int32_t *const *idx_levels, const int64_t *count_levels,
                                   float *const *feat_levels, int activation, void *stream)
{
    int rc = check_levels("read_gather_forward", n, C, levels, idx_levels, count_levels, feat_levels);
    if (rc) return rc;
    READ_CHECK_ARG(rows_nc && (uintptr_t)rows_nc % 16 == 0, "read_gather_forward: rows null or misaligned");
    READ_CHECK_ARG(activation >= 0 && activation <= 2, "read_gather_forward: activation must be 0,1,2");
    LevelTable tab;
    memset(&tab, 0, sizeof(tab));
    long long acc = 0;
    const int qpp = C / 4;
    for (int l = 0; l < levels; ++l) {
        READ_CHECK_ARG(count_levels[l] >= 0, "read_gather_forward: negative pixel count");
        READ_CHECK_ARG(count_levels[l] == 0 || (idx_levels[l] && feat_levels[l]), "read_gather_forward: null level %d", l);
        READ_CHECK_ARG((uintptr_t)feat_levels[l] % 16 == 0, "read_gather_forward: feat level %d misaligned", l);
        tab.idx[l] = idx_levels[l];
        tab.feat[l] = feat_levels[l];
        acc += count_levels[l] * qpp;
        tab.end[l] = acc;
    }
    tab.levels = levels;
    if (acc == 0) return READ_OK;
    int64_t blocks = ceil_div64(acc, 256);
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(gather_forward_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), rows_nc,
                       (long long)n, C, tab, activation);
    READ_CHECK_LAUNCH();
    return READ_OK;
}

extern "C" int read_gather_forward_tables(const read_gather_table *tables, int count, int C, int levels,
                                          const int32_t *const *idx_levels, const int64_t *count_levels,
                                          float *const *feat_levels, void *stream)
{
    const char *who = "read_gather_forward_tables";
    READ_CHECK_ARG(count >= 1 && count <= READ_GATHER_MAX_TABLES, "%s: count must be 1..%d tables (got %d)", who,
                   READ_GATHER_MAX_TABLES, count);
    READ_CHECK_ARG(C >= 4 && C % 4 == 0 && C <= 64, "%s: C must be a multiple of 4 in [4,64] (got %d)", who, C);
    READ_CHECK_ARG(levels >= 1 && levels <= READ_MAX_LEVELS, "%s: levels must be 1..%d (got %d)", who, READ_MAX_LEVELS, levels);
    READ_CHECK_ARG(tables && idx_levels && count_levels && feat_levels, "%s: null table list or level table", who);
    GatherTables tt;
    int rc = fill_tables(who, tables, count, &tt);
    if (rc) return rc;
    LevelTable tab;
    memset(&tab, 0, sizeof(tab));
    long long acc = 0;
    const int qpp = C / 4;
    for (int l = 0; l < levels; ++l) {
        READ_CHECK_ARG(count_levels[l] >= 0, "%s: negative pixel count", who);
        READ_CHECK_ARG(count_levels[l] == 0 || (idx_levels[l] && feat_levels[l]), "%s: null level %d", who, l);
        READ_CHECK_ARG((uintptr_t)feat_levels[l] % 16 == 0, "%s: feat level %d misaligned", who, l);
        tab.idx[l] = idx_levels[l];
        tab.feat[l] = feat_levels[l];
        acc += count_levels[l] * qpp;
        tab.end[l] = acc;
    }
    tab.levels = levels;
    if (acc == 0) return READ_OK;
    int64_t blocks = ceil_div64(acc, 256);
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(gather_tables_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), tt, C, tab);
    READ_CHECK_LAUNCH();
    return READ_OK;
}

extern "C" int read_gather_forward_ss(const float *rows_nc, int64_t n, int C, int levels, int B,
                                      const int32_t *const *idx_levels, const int *h_levels, const int *w_levels, int ss,
                                      float *const *feat_levels, int activation, void *stream)
{
    int rc = check_levels("read_gather_forward_ss", n, C, levels, idx_levels, (const int64_t *)h_levels, feat_levels);
    if (rc) return rc;
    READ_CHECK_ARG(rows_nc && (uintptr_t)rows_nc % 16 == 0, "read_gather_forward_ss: rows null or misaligned");
    READ_CHECK_ARG(w_levels && B >= 1 && ss >= 1 && ss <= 8, "read_gather_forward_ss: bad B / ss / sizes");
    READ_CHECK_ARG(activation >= 0 && activation <= 2, "read_gather_forward_ss: activation must be 0,1,2");
    LevelTableSS tab;
    memset(&tab, 0, sizeof(tab));
    long long acc = 0;
    const int qpp = C / 4;
    for (int l = 0; l < levels; ++l) {
        READ_CHECK_ARG(h_levels[l] >= 1 && w_levels[l] >= 1 && idx_levels[l] && feat_levels[l],
                       "read_gather_forward_ss: bad level %d", l);
        READ_CHECK_ARG((uintptr_t)feat_levels[l] % 16 == 0, "read_gather_forward_ss: feat level %d misaligned", l);
        tab.idx[l] = idx_levels[l];
        tab.feat[l] = feat_levels[l];
        tab.h[l] = h_levels[l];
        tab.w[l] = w_levels[l];
        acc += (long long)B * h_levels[l] * w_levels[l] * qpp;
        tab.end[l] = acc;
    }
    tab.levels = levels;
    int64_t blocks = ceil_div64(acc, 256);
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(gather_forward_ss_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), rows_nc,
                       (long long)n, C, tab, ss, activation);
    READ_CHECK_LAUNCH();
    return READ_OK;
}

extern "C" int read_stitch_gather_forward(const read_stitch_part *parts, int count, int C, int levels,
                                          const int64_t *count_levels, int32_t *const *idx_levels, float *const *depth_levels,
                                          unsigned char *const *part_levels, float *const *feat_levels, void *stream)
{
    const char *who = "read_stitch_gather_forward";
    READ_CHECK_ARG(count >= 1 && count <= READ_STITCH_MAX_PARTS, "%s: count must be 1..%d parts (got %d)", who,
                   READ_STITCH_MAX_PARTS, count);
    READ_CHECK_ARG(C >= 4 && C % 4 == 0 && C <= 64, "%s: C must be a multiple of 4 in [4,64] (got %d)", who, C);
    READ_CHECK_ARG(levels >= 1 && levels <= READ_MAX_LEVELS, "%s: levels must be 1..%d (got %d)", who, READ_MAX_LEVELS, levels);
    READ_CHECK_ARG(parts && count_levels, "%s: null part table", who);
    READ_CHECK_ARG(idx_levels || depth_levels || part_levels || feat_levels, "%s: no outputs (all four output tables are null)", who);
    StitchTable tab;
    memset(&tab, 0, sizeof(tab));
    for (int s = 0; s < count; ++s) {
        const read_stitch_part &p = parts[s];
        READ_CHECK_ARG(!feat_levels || p.rows_nc, "%s: part %d: rows_nc is null while features are requested", who, s);
        READ_CHECK_ARG(!feat_levels || (uintptr_t)p.rows_nc % 16 == 0, "%s: part %d: rows misaligned", who, s);
        READ_CHECK_ARG(p.n >= 1, "%s: part %d: empty descriptor table", who, s);
        READ_CHECK_ARG(p.id_base >= 0 && (int64_t)p.id_base + p.n <= (int64_t)INT32_MAX,
                       "%s: part %d: id_base %d + n %lld leaves the int32 id range", who, s, p.id_base, (long long)p.n);
        READ_CHECK_ARG(p.activation >= 0 && p.activation <= 2, "%s: part %d: activation must be 0,1,2", who, s);
        READ_CHECK_ARG(!p.idx_levels == !p.depth_levels, "%s: part %d: index and depth pyramids go together (both, or both null = hidden)",
                       who, s);
        tab.rows[s] = p.rows_nc;
        tab.n[s] = p.n;
        tab.id_base[s] = p.id_base;
        tab.act[s] = p.activation;
        if (p.idx_levels) tab.visible |= 1u << s;
    }
    long long acc = 0;
    const int Ck = feat_levels ? C : 4;       // without features one lane per pixel
    const int qpp = Ck / 4;
    for (int l = 0; l < levels; ++l) {
        READ_CHECK_ARG(count_levels[l] >= 0, "%s: negative pixel count", who);
        for (int s = 0; s < count; ++s) {
            if (!parts[s].idx_levels) continue;
            READ_CHECK_ARG(count_levels[l] == 0 || (parts[s].idx_levels[l] && parts[s].depth_levels[l]), "%s: part %d: null level %d",
                           who, s, l);
            tab.idx[s][l] = parts[s].idx_levels[l];
            tab.depth[s][l] = parts[s].depth_levels[l];
        }
        READ_CHECK_ARG(count_levels[l] == 0 || ((!idx_levels || idx_levels[l]) && (!depth_levels || depth_levels[l]) &&
                                                (!part_levels || part_levels[l]) && (!feat_levels || feat_levels[l])),
                       "%s: null output level %d", who, l);
        READ_CHECK_ARG(!feat_levels || (uintptr_t)feat_levels[l] % 16 == 0, "%s: feat level %d misaligned", who, l);
        if (idx_levels) tab.out_idx[l] = idx_levels[l];
        if (depth_levels) tab.out_depth[l] = depth_levels[l];
        if (part_levels) tab.out_part[l] = part_levels[l];
        if (feat_levels) tab.feat[l] = feat_levels[l];
        acc += count_levels[l] * qpp;
        tab.end[l] = acc;
    }
    tab.levels = levels;
    tab.count = count;
    tab.want_idx = idx_levels != nullptr;
    tab.want_depth = depth_levels != nullptr;
    tab.want_part = part_levels != nullptr;
    tab.want_feat = feat_levels != nullptr;
    if (acc == 0) return READ_OK;
    int64_t blocks = ceil_div64(acc, 256);
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(stitch_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), tab, Ck);
    READ_CHECK_LAUNCH();
    return READ_OK;
}

extern "C" int read_gather_backward(float *drows_nc, int64_t n, int C, int levels,
                                    const int32_t *const *idx_levels, const int64_t *count_levels,
                                    const float *const *dfeat_levels, void *stream)
{
    int rc = check_levels("read_gather_backward", n, C, levels, idx_levels, count_levels, dfeat_levels);
    if (rc) return rc;
    READ_CHECK_ARG(drows_nc, "read_gather_backward: drows is null");
    LevelTableBwd tab;
    memset(&tab, 0, sizeof(tab));
    long long acc = 0;
    const int qpp = C / 4;
    for (int l = 0; l < levels; ++l) {
        READ_CHECK_ARG(count_levels[l] >= 0, "read_gather_backward: negative pixel count");
        READ_CHECK_ARG(count_levels[l] == 0 || (idx_levels[l] && dfeat_levels[l]), "read_gather_backward: null level %d", l);
        READ_CHECK_ARG((uintptr_t)dfeat_levels[l] % 16 == 0, "read_gather_backward: dfeat level %d misaligned", l);
        tab.idx[l] = idx_levels[l];
        tab.dfeat[l] = dfeat_levels[l];
        acc += count_levels[l] * qpp;
        tab.end[l] = acc;
    }
    tab.levels = levels;
    if (acc == 0) return READ_OK;
    int64_t blocks = ceil_div64(acc, 256);
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(gather_backward_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), drows_nc,
                       (long long)n, C, tab);
    READ_CHECK_LAUNCH();
    return READ_OK;
}

extern "C" int read_gather_backward_tables(const read_gather_table *tables, int count, int C, int levels,
                                           const int32_t *const *idx_levels, const int64_t *count_levels,
                                           const float *const *dfeat_levels, const float *const *feat_levels,
                                           float *const *g_levels, float *const *drows_tables, void *stream)
{
    const char *who = "read_gather_backward_tables";
    READ_CHECK_ARG(count >= 1 && count <= READ_GATHER_MAX_TABLES, "%s: count must be 1..%d tables (got %d)", who,
                   READ_GATHER_MAX_TABLES, count);
    READ_CHECK_ARG(C >= 4 && C % 4 == 0 && C <= 64, "%s: C must be a multiple of 4 in [4,64] (got %d)", who, C);
    READ_CHECK_ARG(levels >= 1 && levels <= READ_MAX_LEVELS, "%s: levels must be 1..%d (got %d)", who, READ_MAX_LEVELS, levels);
    READ_CHECK_ARG(tables && idx_levels && count_levels && dfeat_levels, "%s: null table list or level table", who);
    GatherTables fwd;
    int rc = fill_tables(who, tables, count, &fwd, false);
    if (rc) return rc;
    GatherTablesBwd tt;
    memset(&tt, 0, sizeof(tt));
    bool any_act = false, any_dense = false;
    for (int t = 0; t < count; ++t) {
        tt.n[t] = fwd.n[t];
        tt.base[t] = fwd.base[t];
        tt.act[t] = fwd.act[t];
        any_act = any_act || fwd.act[t] != 0;
        if (drows_tables && drows_tables[t]) {
            READ_CHECK_ARG((uintptr_t)drows_tables[t] % 16 == 0, "%s: table %d: gradient rows misaligned", who, t);
            tt.drows[t] = drows_tables[t];
            any_dense = true;
        }
    }
    tt.count = count;
    READ_CHECK_ARG(feat_levels || !any_act, "%s: feat_levels is null while a table has an activation (act' needs the forward's output)",
                   who);
    READ_CHECK_ARG(g_levels || any_dense, "%s: no outputs (g_levels is null and no table has gradient rows)", who);
    LevelTableBwdT tab;
    memset(&tab, 0, sizeof(tab));
    long long acc = 0;
    const int qpp = C / 4;
    for (int l = 0; l < levels; ++l) {
        READ_CHECK_ARG(count_levels[l] >= 0, "%s: negative pixel count", who);
        READ_CHECK_ARG(count_levels[l] == 0 || (idx_levels[l] && dfeat_levels[l] && (!any_act || feat_levels[l]) &&
                                                (!g_levels || g_levels[l])), "%s: null level %d", who, l);
        READ_CHECK_ARG((uintptr_t)dfeat_levels[l] % 16 == 0, "%s: dfeat level %d misaligned", who, l);
        READ_CHECK_ARG(!any_act || (uintptr_t)feat_levels[l] % 16 == 0, "%s: feat level %d misaligned", who, l);
        READ_CHECK_ARG(!g_levels || (uintptr_t)g_levels[l] % 16 == 0, "%s: g level %d misaligned", who, l);
        tab.idx[l] = idx_levels[l];
        tab.dfeat[l] = dfeat_levels[l];
        if (any_act) tab.feat[l] = feat_levels[l];
        if (g_levels) tab.g[l] = g_levels[l];
        acc += count_levels[l] * qpp;
        tab.end[l] = acc;
    }
    tab.levels = levels;
    if (acc == 0) return READ_OK;
    int64_t blocks = ceil_div64(acc, 256);
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(gather_tables_backward_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), tt, C, tab,
                       g_levels != nullptr ? 1 : 0, any_dense ? 1 : 0);
    READ_CHECK_LAUNCH();
    return READ_OK;
}

extern "C" int read_bilinear_down(const float *in, int64_t planes, int h, int w, int ss, float *out, void *stream)
{
    READ_CHECK_ARG(in && out && planes >= 1 && h >= 1 && w >= 1, "read_bilinear_down: null pointer or empty tensor");
    READ_CHECK_ARG(ss >= 2 && ss <= 8, "read_bilinear_down: the factor must be 2..8 (got %d)", ss);
    int64_t blocks = ceil_div64(planes * h * w, 256);
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(bilinear_down_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), in, (long long)planes, h, w,
                       ss, out);
    READ_CHECK_LAUNCH();
    return READ_OK;
}

extern "C" int read_bilinear_down_backward(const float *dout, int64_t planes, int h, int w, int ss, float *din, void *stream)
{
    READ_CHECK_ARG(dout && din && planes >= 1 && h >= 1 && w >= 1, "read_bilinear_down_backward: null pointer or empty tensor");
    READ_CHECK_ARG(ss >= 2 && ss <= 8, "read_bilinear_down_backward: the factor must be 2..8 (got %d)", ss);
    int64_t blocks = ceil_div64(planes * h * w * ss * ss, 256);
    if (blocks > 256 * 8) blocks = 256 * 8;
    hipLaunchKernelGGL(bilinear_down_backward_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream), dout,
                       (long long)planes, h, w, ss, din);
    READ_CHECK_LAUNCH();
    return READ_OK;
}
