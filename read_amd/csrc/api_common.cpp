// Error plumbing + device query of the C ABI.
#include <stdarg.h>

#include "common.h"
#include "internal.h"

namespace readhip {
static thread_local char g_err[512] = "";
void set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace readhip

extern "C" const char *read_last_error(void) { return readhip::g_err; }
extern "C" int read_abi_version(void) { return 3; }   // 2: read_conv_desc.wpacked_w4h / wpacked_d3h; 3: wpacked_t3h at the end of the struct (round 6)

extern "C" int read_device_arch(char *name, int len)
{
    READ_CHECK_ARG(name && len > 0, "read_device_arch: bad buffer");
    int dev = 0;
    READ_CHECK_HIP(hipGetDevice(&dev));
    hipDeviceProp_t p;
    READ_CHECK_HIP(hipGetDeviceProperties(&p, dev));
    snprintf(name, (size_t)len, "%s", p.gcnArchName);
    char *colon = strchr(name, ':');
    if (colon) *colon = 0;
    return READ_OK;
}

namespace readhip {
int device_cus()
{
    static int n_cu = 0;
    if (!n_cu) {
        int dev = 0;
        hipDeviceProp_t prop;
        n_cu = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess &&
                prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
    }
    return n_cu;
}
}  // namespace readhip

// Debug: per-workgroup timeline of the next gated-conv launches.  buf = device memory, 64 bytes per
// workgroup: s_memrealtime (100 MHz) at kernel entry / after the prologue / after the k-loop / at exit,
// HW_ID, XCC_ID, blockIdx.x, blockIdx.y.  NULL switches it off.
#ifdef READ_DEBUG_KNOBS
extern "C" int read_debug_set_trace(void *buf, size_t bytes)
{
    readhip::conv_set_trace(buf, bytes);
    return READ_OK;
}
#endif

// Tuning knobs for A/B measurements on the GPU box (not needed in production).  Every knob of the release library
// selects between implementations that produce the SAME results; the attribution probes whose results are invalid
// ("conv_ablate") exist only in builds with -DREAD_DEBUG_KNOBS.
// read_tuning_key enumerates these, then the release rows of the conv table (conv_key), "wgrad_wino", then the conv table's debug-only rows.
static const char *const k_head_keys[] = {"splat_mode", "splat_stats", "splat_subset", "splat_near", "splat_cells",
                                          "splat_cells_sub", "splat_seeds", "splat_items", "splat_strips", "splat_wgs", "splat_zl2", "splat_lds", "splat_bins", "splat_ahead", "splat_prof", "splat_mark", "splat_cells_batch", "splat_compact", "splat_sticky", "splat_wgs_b", "splat_kslot", "unet_streams", "unet_aff_split", "unet_up_fold"};
constexpr int N_HEAD_KEYS = sizeof(k_head_keys) / sizeof(k_head_keys[0]);

extern "C" int read_tuning_set(const char *key, int value)
{
    READ_CHECK_ARG(key, "read_tuning_set: null key");
    if (!strcmp(key, "splat_mode")) {
        const int rc = readhip::splat_set_mode(value);
        if (rc) readhip::set_error("read_tuning_set: splat_mode must be 1 (agent atomics) or 7 (warm start + hi-z)");
        return rc;
    }
    if (!strcmp(key, "splat_stats")) { readhip::splat_set_stats(value); return READ_OK; }
    if (!strcmp(key, "splat_subset")) { readhip::splat_set_subset(value); return READ_OK; }
    // cell path: expected points per pixel in front of the pass-A split distance
    if (!strcmp(key, "splat_near")) { readhip::splat_set_near(value); return READ_OK; }
    if (!strcmp(key, "splat_cells_sub")) { readhip::splat_set_cells_sub(value); return READ_OK; }
    if (!strcmp(key, "splat_seeds")) { readhip::splat_set_seeds(value); return READ_OK; }     // 0: no warm start
    if (!strcmp(key, "splat_cells")) { readhip::splat_set_cells(value); return READ_OK; }     // 0: ignore the cell-ordered copy
    if (!strcmp(key, "splat_items")) { readhip::splat_set_items(value); return READ_OK; }     // work items per chunk: 1, 2, 4
    if (!strcmp(key, "splat_kslot")) { readhip::splat_set_kslot(value); return READ_OK; }     // key-image layout: 0 linear, 1 strided, 2 scattered
    if (!strcmp(key, "splat_lds")) { readhip::splat_set_lds(value); return READ_OK; }         // 0: no LDS table in front of the atomics
    if (!strcmp(key, "splat_bins")) { readhip::splat_set_bins(value); return READ_OK; }       // 0: pass A with one atomic per candidate
    if (!strcmp(key, "splat_ahead")) { readhip::splat_set_ahead(value); return READ_OK; }     // 0: never fold the next frame's first launch into this frame's last
    if (!strcmp(key, "splat_wgs_b")) { readhip::splat_set_wgs_b(value); return READ_OK; }     // workgroups per CU of pass B (0: as pass A)
    if (!strcmp(key, "splat_cells_batch")) { readhip::splat_set_cells_batch(value); return READ_OK; }   // 0: camera batches on the plain pass
    if (!strcmp(key, "splat_compact")) { readhip::splat_set_compact(value); return READ_OK; }  // 0: pass A bins its candidates from four masked slots per lane
    if (!strcmp(key, "splat_mark")) { readhip::splat_set_mark(value); return READ_OK; }       // 0: only pass-B survivors are promoted into list A
    if (!strcmp(key, "splat_sticky")) { readhip::splat_set_sticky(value); return READ_OK; }   // frames a front chunk stays in list A
    if (!strcmp(key, "splat_prof")) { readhip::splat_set_prof(value); return READ_OK; }       // events around the cell path's launches
    if (!strcmp(key, "splat_zl2")) { readhip::splat_set_zl2(value); return READ_OK; }         // 1: early-z loads bypass the L1
    if (!strcmp(key, "splat_wgs")) { readhip::splat_set_wgs(value); return READ_OK; }         // workgroups per CU of the passes
    if (!strcmp(key, "splat_strips")) { readhip::splat_set_strips(value); return READ_OK; }   // column strips: 1, 2, 4, 8
    if (!strcmp(key, "unet_streams")) { readhip::unet_set_streams(value); return READ_OK; }   // 0: SCM chains on the caller's stream
    // 0: AFF first convs as single 480-channel launches (takes effect for plans created afterwards)
    if (!strcmp(key, "unet_aff_split")) { readhip::unet_set_aff_split(value != 0); return READ_OK; }
    // 0: Upsample4(bilinear) as a separate pass and Convs.k over the concat (takes effect for plans created afterwards)
    if (!strcmp(key, "unet_up_fold")) { readhip::unet_set_up_fold(value != 0); return READ_OK; }
    if (readhip::conv_set(key, value)) return READ_OK;                                          // the "conv_*" keys: one table in conv.hip
    if (!strcmp(key, "wgrad_wino")) { readhip::train_set_wgrad_wino(value); return READ_OK; }   // 0: 3x3 weight gradients on the direct kernel
    readhip::set_error("read_tuning_set: unknown key '%s'", key);
    return READ_EINVAL;
}

extern "C" int read_tuning_get(const char *key, int *value)
{
    READ_CHECK_ARG(key && value, "read_tuning_get: null pointer");
    if (readhip::splat_get(key, value) || readhip::conv_get(key, value) || readhip::unet_get(key, value) || readhip::train_get(key, value)) return READ_OK;
    readhip::set_error("read_tuning_get: unknown key '%s'", key);
    return READ_EINVAL;
}

extern "C" const char *read_tuning_key(int i)
{
    if (i < 0) return nullptr;
    if (i < N_HEAD_KEYS) return k_head_keys[i];
    i -= N_HEAD_KEYS;
    int n_conv = 0;
    while (readhip::conv_key(n_conv, false)) ++n_conv;
    if (i < n_conv) return readhip::conv_key(i, false);
    return i == n_conv ? "wgrad_wino" : readhip::conv_key(i - n_conv - 1, true);
}
