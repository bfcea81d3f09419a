// What one translation unit of libreadhip.so defines and another one calls: declared here once (none of it is C ABI).
#pragma once
#include "common.h"

namespace readhip {

// api_common.cpp: compute units of the current device, queried once per process (256 where the query fails)
int device_cus();

// conv.hip
// Validates a descriptor, routes it (conv_route) and launches: shared by read_gated_conv_forward[_f4x1] and the UNet executor.
// wp_f4x1: the F(4,3)-by-rows operand beside the descriptor, or NULL.
int launch_gated_conv(const read_conv_desc *d, hipStream_t stream, const void *wp_f4x1);
// The public family number (read_conv_kernel_family) of the kernel this descriptor runs on under the current knobs.
int conv_family(const read_conv_desc *d);
// The "conv_*" tuning knobs, one table: 1 = key known (conv_set stores the normalised value), 0 = not a conv key of this build.
int conv_set(const char *key, int value);
int conv_get(const char *key, int *value);
// i-th key of the table's release rows (debug_only = false) or of its -DREAD_DEBUG_KNOBS rows; NULL past the end
const char *conv_key(int i, bool debug_only);
void conv_set_trace(void *buf, size_t bytes);

// splat.hip
int splat_set_mode(int m);
void splat_set_subset(int v);
void splat_set_stats(int v);
void splat_set_near(int v);
void splat_set_cells(int v);
void splat_set_seeds(int v);
void splat_set_cells_sub(int v);
void splat_set_items(int v);
void splat_set_strips(int v);
void splat_set_wgs(int v);
void splat_set_zl2(int v);
void splat_set_lds(int v);
void splat_set_bins(int v);
void splat_set_ahead(int v);
void splat_set_prof(int v);
void splat_set_mark(int v);
void splat_set_cells_batch(int v);
void splat_set_compact(int v);
void splat_set_wgs_b(int v);
void splat_set_sticky(int v);
void splat_set_kslot(int v);
int splat_get(const char *key, int *value);

// unet.cpp
void unet_set_streams(int v);
void unet_set_aff_split(int v);
void unet_set_up_fold(int v);
int unet_get(const char *key, int *value);

// train.hip
void train_set_wgrad_wino(int v);
int train_get(const char *key, int *value);

}  // namespace readhip
