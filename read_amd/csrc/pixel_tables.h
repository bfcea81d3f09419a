// From a pixel of an edited level-0 frame back to what drew it, shared by the two pixel passes that need it (annotate.hip, flow.hip):
// the id -> (object, point) resolution through the labels and the foreign ranges, and the walk over the instances of that object
// for the first visible one whose matrix lands the point on this pixel at this depth.  The match is exact because
// project_one is the frame's device function on the same matrix bits: include only from files compiled with -ffp-contract=off.
#pragma once
#include "common.h"
#include "project.h"

namespace readhip {

constexpr int PIXEL_MAX_FOREIGN = READ_GATHER_MAX_TABLES - 1;

// foreign range f: ids [base, base + n) are pool points [first, first + n); travels by value in the kernel arguments
struct ForeignRanges {
    long long base[PIXEL_MAX_FOREIGN], n[PIXEL_MAX_FOREIGN], first[PIXEL_MAX_FOREIGN];
    int count;
};

// the instance list in device memory: object k's instances are obj_list[obj_begin[k - 1] .. obj_begin[k]), list positions ascending
struct PixelTables {
    const float *M;
    const int32_t *visible, *value, *obj_begin, *obj_list;
    int count, K, K_own;
};

// id -> the object k (0 = the static scene) and the point; -1 where no range holds the id or the label lies past the own objects
__device__ __forceinline__ int pixel_object(int32_t id, const float *__restrict__ xyz, long long n, const int32_t *__restrict__ labels,
                                            const float *__restrict__ pool_xyz, const ForeignRanges &fr, int K_own, const float *&pt)
{
    int k = -1;
    pt = nullptr;
    if (id >= 0 && (long long)id < n) {
        k = labels ? labels[id] : 0;
        if (k > K_own) k = -1;                     // a label past the own objects: no range holds it
        pt = xyz + 3ll * id;
    } else {
        for (int f = 0; f < fr.count; ++f)
            if ((long long)id >= fr.base[f] && (long long)id < fr.base[f] + fr.n[f]) {
                k = K_own + 1 + f;
                pt = pool_xyz + 3 * (fr.first[f] + ((long long)id - fr.base[f]));
            }
    }
    return k;
}

// the list position of the first visible instance of object k >= 1 that projects the point pt to pixel p with depth bits dbits; -1: none
__device__ __forceinline__ int pixel_drawer(const PixelTables &tb, int k, const float *__restrict__ pt, long long p, uint32_t dbits, int W,
                                            int H)
{
    if (tb.count <= 0) return -1;                               // no list: no table and no point is read
    const float x = pt[0], y = pt[1], z = pt[2];
    const int j1 = min(tb.obj_begin[k], tb.count);              // a table out of step must not read past its end
    for (int j = max(tb.obj_begin[k - 1], 0); j < j1; ++j) {
        const int i = tb.obj_list[j];
        if ((unsigned)i >= (unsigned)tb.count || tb.visible[i] == 0) continue;
        float d;
        int xx, yy;
        const int pix = project_one(x, y, z, tb.M + 16 * (size_t)i, W, H, d, xx, yy);
        if ((long long)pix == p && __float_as_uint(d) == dbits) return i;
    }
    return -1;
}

}  // namespace readhip
