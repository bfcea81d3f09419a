// Ranges of points folded into a 64-bit key image, each under its own 16 camera floats: what the rasteriser's edited frames
// (splat.hip) and the LiDAR pass (lidar.hip) share on both sides of a launch.
#pragma once
#include "common.h"

namespace readhip {

// relaxed agent-scope load = global_load_dwordx2 sc1: served by L2, never by the CU's stale L1
__device__ __forceinline__ unsigned long long peek_key_agent(const unsigned long long *k)
{
    return __hip_atomic_load(k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void fold_key_agent(unsigned long long *k, unsigned long long key)
{
    __hip_atomic_fetch_min(k, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Up to OBJ_MAX ranges per launch, their camera floats in the kernel arguments; workgroup b works on the range whose first
// workgroup (a host prefix of block counts) is the last one <= b — a scalar scan of <= OBJ_MAX entries per workgroup, no search
// per point.
constexpr int OBJ_MAX = 32;
struct ObjBatch {
    float m[OBJ_MAX][16];
    long long first[OBJ_MAX], last[OBJ_MAX];        // range k = points [first, last) of the compacted arrays
    int block0[OBJ_MAX + 1];                        // first workgroup of range k; block0[count] = the grid
    int count;
};

// The range workgroup b works on, and the point of range j that the calling thread of workgroup b works on (the caller compares it
// with ob.last[j]).
__device__ __forceinline__ int range_of_block(const ObjBatch &ob, int b)
{
    int j = 0;
    for (int k = 1; k < ob.count; ++k)
        if (b >= ob.block0[k]) j = k;
    return j;
}
__device__ __forceinline__ long long range_point(const ObjBatch &ob, int j, int b)
{
    return ob.first[j] + (long long)(b - ob.block0[j]) * 256 + threadIdx.x;
}

// Every range that will be launched — visible and non-empty — of a partition (objs), of a list (inst) or of neither:
// f(k, first, last, M_k) -> READ_OK or the code to stop with.
template <class F>
int for_each_range(const read_splat_objects *objs, const read_splat_instances *inst, F &&f)
{
    const int count = objs ? objs->count : inst ? inst->count : 0;
    const float *M = objs ? objs->M : inst ? inst->M : nullptr;
    const unsigned char *visible = objs ? objs->visible : inst ? inst->visible : nullptr;
    for (int k = 0; k < count; ++k) {
        const int64_t first = objs ? objs->begin[k] : inst->first[k], last = objs ? objs->begin[k + 1] : first + inst->npts[k];
        if ((visible && !visible[k]) || last == first) continue;                            // hidden or empty: not launched
        if (const int rc = f(k, first, last, M + 16 * (size_t)k); rc != READ_OK) return rc;
    }
    return READ_OK;
}

// The static part (n0 points of xyz0 / ids0 under M0; n0 = 0: none) as a launch of its own, then every range of objs / inst,
// OBJ_MAX per launch: stream-ordered, no synchronisation.  launch(ob, blocks, xyz, ids) -> READ_OK or an error.
template <class Launch>
int launch_ranges(const float *xyz0, const int32_t *ids0, int64_t n0, const float *M0, const read_splat_objects *objs,
                  const read_splat_instances *inst, Launch &&launch)
{
    ObjBatch ob;
    memset(&ob, 0, sizeof(ob));
    int blocks = 0;
    auto add = [&](int64_t first, int64_t last, const float *M) {
        const int k = ob.count++;
        memcpy(ob.m[k], M, sizeof(ob.m[k]));
        ob.first[k] = first;
        ob.last[k] = last;
        ob.block0[k] = blocks;
        blocks += (int)ceil_div64(last - first, 256);
    };
    auto flush = [&](const float *xyz, const int32_t *ids) -> int {
        if (ob.count == 0) return READ_OK;
        ob.block0[ob.count] = blocks;
        const int rc = launch(ob, blocks, xyz, ids);
        ob.count = 0;
        blocks = 0;
        return rc;
    };
    if (n0 > 0) {
        add(0, n0, M0);
        if (const int rc = flush(xyz0, ids0); rc != READ_OK) return rc;
    }
    const float *xyz = objs ? objs->xyz : inst ? inst->xyz : nullptr;
    const int32_t *ids = objs ? objs->ids : inst ? inst->ids : nullptr;
    const int rc = for_each_range(objs, inst, [&](int, int64_t first, int64_t last, const float *M) -> int {
        add(first, last, M);
        return ob.count == OBJ_MAX ? flush(xyz, ids) : READ_OK;
    });
    return rc != READ_OK ? rc : flush(xyz, ids);
}

}  // namespace readhip
