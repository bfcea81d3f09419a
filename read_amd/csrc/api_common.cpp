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

// Tuning knobs for A/B measurements on the GPU box (not needed in production).  Every knob selects between implementations
// that produce the SAME results, in the release library and in builds with -DREAD_DEBUG_KNOBS alike.
// Each module keeps its keys in one table (internal.h); read_tuning_key enumerates the tables in the order of k_key.
namespace readhip {
static const TuneRow *find_row(const TuneRow *rows, int n, const char *key)
{
    for (int i = 0; i < n; ++i)
        if (!strcmp(key, rows[i].key)) return rows + i;
    return nullptr;
}

int tune_set(const TuneRow *rows, int n, const char *key, int v)
{
    const TuneRow *r = find_row(rows, n, key);
    if (!r) return 0;
    if (r->norm == TN_EITHER && v != r->lo && v != r->hi) return READ_EINVAL;
    if (r->norm == TN_FLAG) v = v != 0;
    if (r->norm == TN_CLAMP || r->norm == TN_POW2) v = v < r->lo ? r->lo : v > r->hi ? r->hi : v;
    if (r->norm == TN_POW2)
        while (v & (v - 1)) v &= v - 1;
    *r->value = v;
    return 1;
}

int tune_get(const TuneRow *rows, int n, const char *key, int *value)
{
    const TuneRow *r = find_row(rows, n, key);
    if (r) *value = *r->value;
    return r != nullptr;
}
const char *tune_key(const TuneRow *rows, int n, int i) { return i >= 0 && i < n ? rows[i].key : nullptr; }

static int (*const k_set[])(const char *, int) = {splat_set, unet_set, conv_set, train_set};
static int (*const k_get[])(const char *, int *) = {splat_get, unet_get, conv_get, train_get};
static const char *(*const k_key[])(int) = {splat_key, unet_key, conv_key, train_key};
}  // namespace readhip

extern "C" int read_tuning_set(const char *key, int value)
{
    READ_CHECK_ARG(key, "read_tuning_set: null key");
    for (const auto set : readhip::k_set)
        if (const int rc = set(key, value)) return rc < 0 ? rc : READ_OK;     // refused: the module has said why
    readhip::set_error("read_tuning_set: unknown key '%s'", key);
    return READ_EINVAL;
}

extern "C" int read_tuning_get(const char *key, int *value)
{
    READ_CHECK_ARG(key && value, "read_tuning_get: null pointer");
    for (const auto get : readhip::k_get)
        if (get(key, value)) return READ_OK;
    readhip::set_error("read_tuning_get: unknown key '%s'", key);
    return READ_EINVAL;
}

extern "C" const char *read_tuning_key(int i)
{
    if (i < 0) return nullptr;
    for (const auto key : readhip::k_key)
        for (int j = 0; key(j); ++j)
            if (i-- == 0) return key(j);
    return nullptr;
}
