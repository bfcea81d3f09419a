// What one translation unit of libreadhip.so defines and another one calls: declared here once (none of it is C ABI).
#pragma once
#include "common.h"

namespace readhip {

// api_common.cpp: compute units of the current device, queried once per process (256 where the query fails)
int device_cus();

// Output channels padded to whole 32-channel groups: the unit of every packed weight order and of the conv kernels
static inline int pad32(int c) { return (c + 31) / 32 * 32; }

// conv.hip
// Validates a descriptor, routes it (conv_route) and launches: shared by read_gated_conv_forward[_f4x1] and the UNet executor.
// wp_f4x1: the F(4,3)-by-rows operand beside the descriptor, or NULL.
int launch_gated_conv(const read_conv_desc *d, hipStream_t stream, const void *wp_f4x1);
// The public family number (read_conv_kernel_family) of the kernel this descriptor runs on under the current knobs.
int conv_family(const read_conv_desc *d);
void conv_set_trace(void *buf, size_t bytes);

// splat.hip
// What a read_splat_instances must be (count, pointers, every range inside its n points): READ_OK, or READ_EINVAL with a message
// that starts with `who`.  The checks of read_splat_forward_instances and its panorama and lens twins; read_lidar_sweep shares them.
int check_instances(const char *who, const read_splat_instances *inst);

// One row of a module's table of tuning keys; the order of the rows is the order read_tuning_key enumerates them in.
enum TuneNorm {
    TN_RAW,
    TN_FLAG,      // != 0
    TN_CLAMP,     // into [lo, hi]
    TN_POW2,      // into [lo, hi] (powers of two), then down to a power of two
    TN_EITHER     // lo or hi; anything else is refused
};
struct TuneRow {
    const char *key;
    int *value;
    TuneNorm norm;
    int lo, hi;
};
// api_common.cpp: 1 = key known and the normalised value stored, 0 = no such key in the table, READ_EINVAL = value refused
int tune_set(const TuneRow *rows, int n, const char *key, int value);
int tune_get(const TuneRow *rows, int n, const char *key, int *value);
const char *tune_key(const TuneRow *rows, int n, int i);       // NULL past the end

// splat.hip, unet.cpp, conv.hip, train.hip: the "splat_*" / "unet_*" / "conv_*" / "wgrad_wino" keys, each through tune_set / tune_get / tune_key
int splat_set(const char *key, int value);
int splat_get(const char *key, int *value);
const char *splat_key(int i);
int unet_set(const char *key, int value);
int unet_get(const char *key, int *value);
const char *unet_key(int i);
int conv_set(const char *key, int value);
int conv_get(const char *key, int *value);
const char *conv_key(int i);
int train_set(const char *key, int value);
int train_get(const char *key, int *value);
const char *train_key(int i);

}  // namespace readhip
