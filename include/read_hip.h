/*
 * read_hip.h — C ABI of libreadhip.so: READ's per-frame render path on MI355X (gfx950).
 *
 * This is the drop-in boundary.  Everything above it (the Python mirror of READ's
 * pcpr / MyRender / PointTexture / UNet / NetAndTexture / TexturePipeline / OGL API in
 * read_amd/) and any other host (C++, cgo, JNI, ctypes) binds exactly these symbols.
 *
 * Conventions
 *   - every function returns 0 (READ_OK) or a negative READ_E* code and never throws;
 *     read_last_error() gives the message of the calling thread's last failure;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); all work is
 *     enqueued on it, nothing synchronises, nothing allocates after *_create / workspace setup;
 *   - pointers are DEVICE pointers owned by the caller unless the name ends in `_host`;
 *   - images are row-major, row 0 = image top; activations are NHWC fp32;
 *   - matrices are row-major 4x4 applied as M * [x y z 1]^T (point_render.cu:96-121).
 *
 * Reference interfaces replaced (file:line under the reference repo):
 *   read_splat_forward        MyRender/CloudProjection/pcpr_cuda.cpp:23-42 (pcpr.forward),
 *                             point_render.cu:125-200 (DepthProject + GPU_PCPR), called 5x per
 *                             iteration by src/READ/gl/myrender.py:32-40; GL twin:
 *                             READ/gl/render.py:52-85 + READ/gl/programs.py:121-125,164-167
 *   read_index_to_float       point_render.cu:158 (`out_index[ind] = (float)ids`)
 *   read_gather_forward       READ/models/texture.py:42-70 (PointTexture.forward = index_select)
 *   read_gather_backward      autograd of texture.py:61 (index_add into texture_.grad)
 *   read_texture_to_rows      layout change of PointTexture.texture_ (1,C,N) -> N x C rows
 *   read_gated_conv_forward   READ/models/unet.py:22-53 (BasicConv) incl. the ResBlock add (:19-20),
 *                             FAM multiply/add (:115-117), torch.cat (:88,:104,:262,:270,:278) and
 *                             F.interpolate nearest (:239-250) folded into its prologue/epilogue
 *   read_bilinear_up4         READ/models/unet.py:200 (nn.Upsample(scale_factor=4, 'bilinear'))
 *   read_unet_*               READ/models/unet.py:121-285 (UNet.__init__/forward)
 */
#ifndef READ_HIP_H
#define READ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define READ_OK        0
#define READ_EINVAL  (-22)   /* bad argument (shape, alignment, null pointer) */
#define READ_ENOMEM  (-12)   /* workspace too small */
#define READ_EHIP     (-5)   /* a HIP runtime call failed; see read_last_error() */

#define READ_MAX_LEVELS      5
#define READ_DESC_CHANNELS   8   /* descriptor size the UNet consumes (READ/pipelines/ogl.py:19-25) */

const char *read_last_error(void);
int read_abi_version(void);
/* Fills name[0..len) with the gfx arch of the current device ("gfx950"); READ_EHIP without a GPU. */
int read_device_arch(char *name, int len);

/* Measurement knobs (A/B runs on the GPU box).  Every knob selects between implementations that produce the SAME results, in
 * every build of the library (-DREAD_DEBUG_KNOBS adds entry points, no key):
 *   "splat_mode"      plain path: 7 (default) warm start + LDS hierarchical-Z, 1 = agent-scope atomics + early-z only
 *   "splat_cells"     0: ignore the cell-ordered copy (plain path everywhere)
 *   "splat_seeds"     0: no warm start from the previous frame
 *   "splat_near"      cell path: expected points per pixel in front of the pass-A split distance (default 12)
 *   "splat_cells_sub" cell path: every n-th chunk joins pass A (default 0 = only on a workspace's first frame, every 32nd; rounds 2-4: 32)
 *   "splat_subset"    plain path: bootstrap pass over every n-th chunk (default 8)
 *   "splat_stats"     debug counters in the workspace header
 *   "conv_wino"       largest Cin that takes the Winograd F(2x2,3x3) kernel (0 = direct implicit-GEMM kernels everywhere)
 *   "conv_sc"         8 (default): gated 3x3/s1 layers with Cin = 32, Cout <= 4 on the vector-pipe kernel, 8 input channels per LDS
 *                     phase (16, 32: larger phases); 0: on the MFMA kernels
 *   "splat_mark"      1 (default): a chunk one of whose points reaches a depth bound is listed in pass A for the next "splat_sticky"
 *                     (default 1) classifications, wherever it lies — on surface-like scenes the chunks beyond the near split that hold
 *                     front points then run banded and binned in pass A instead of surviving pass B's bound test every frame
 *                     (street scene 81.7 -> 70.9 us per frame; volumetric slab unchanged); 0: only pass B's survivors are promoted
 *   "splat_cells_batch" 1 (default): a batch of cameras runs as B cell-path frames; 0: the plain pass over the whole cloud
 *   "splat_prof"      1: HIP events around every launch of a cell-path frame (read_splat_profile_last); 0 (default)
 *   "splat_ahead"     1 (default): with an announced next camera (read_splat_hint_next_camera) a cell-path frame's resolve launch
 *                     also classifies / seeds the next frame — 4 dependent launches per frame instead of 5; 0: always 5
 *   "unet_up_fold"    0 (default): nn.Upsample(x4, bilinear) as a pass of its own; 1: folded into the Convs.k launches
 *                     (read_conv_desc.pre_bilinear; measured level-to-slower, profiles/r5_up_fold_ab.md); plans created afterwards
 *   "wgrad_wino"      1 (default): 3x3/s1 weight gradients in the Winograd F(4x4,3x3) domain; 0: direct MFMA kernel; v > 1: the same
 *                     with 128 v workgroups aimed at (default 256)
 *   "conv_wave", "conv_kc32", "conv_stagger": see csrc/conv.hip.
 * read_tuning_key(i) enumerates the keys (NULL past the end); read_tuning_get reads the current value, so that a
 * benchmark can record the state it ran with. */
int read_tuning_set(const char *key, int value);
int read_tuning_get(const char *key, int *value);
const char *read_tuning_key(int i);
/* Debug entry points (timeline trace of the conv kernels, issue / operand / MFMA-ceiling probes) are NOT part of this ABI: they
 * exist only in libreadhip_debug.so (python -m read_amd.build --debug, -DREAD_DEBUG_KNOBS) and are declared in read_hip_debug.h. */

/* ---------------------------------------------------------------- rasteriser (z-buffer splat) */

/* Bytes of the persistent rasteriser state for ONE (B, W, H): an 8192-byte header (frame state, two sets of chunk-list counters),
 * the key images (min(B,8) cameras x W*H x 8 B, depth_bits<<32 | point_id), the hierarchical-Z bound image, two seed images (the
 * warm start of the next frame), the two depth-bound images of the cell path (frames alternate between them) and its bins.  A workspace serves the (B, W, H) it
 * was sized for; re-run read_splat_workspace_init before using it with another size.  256-byte aligned. */
size_t read_splat_workspace_bytes(int B, int W, int H);
/* Must be called once on a fresh workspace (sets every key to EMPTY).  read_splat_forward
 * leaves the workspace EMPTY again, so consecutive frames need no further clears. */
int read_splat_workspace_init(void *ws, size_t ws_bytes, void *stream);

/*
 * One pass over the cloud for B cameras and `levels` scales.
 *   xyz          N x 3 fp32 (device)
 *   M_host       B x 16 fp32 on the HOST: proj @ inv(view) per camera (myrender.py:28-30)
 *   W,H          level-0 size; level l is int(W*0.5^l) x int(H*0.5^l) (myrender.py:33-34)
 *   idx_levels   host array of `levels` device pointers, level l = int32 [B][h_l][w_l]
 *   depth_levels same shape, fp32; either array (or single entries) may be NULL to skip
 * Semantics (bit-exact, deterministic): per pixel the accepted point of minimum fp32 depth,
 * ties -> minimum point id; empty pixels (0, 0.0f).  When W or H is not a multiple of
 * 2^(levels-1) each level is rasterised by its own pass over the points.
 */
int read_splat_forward(const float *xyz, int64_t n, const float *M_host, int B, int W, int H,
                       int levels, int32_t *const *idx_levels, float *const *depth_levels,
                       void *ws, size_t ws_bytes, void *stream);

/* Cell-ordered copy of a cloud (optional accelerator of the single-camera path; results are bit-identical).
 * read_splat_cells_build() sorts the points once along a Morton curve into chunks of 1024 records
 * (x, y, z, original id) with their bounding boxes, on the device (device cloud in, device blob of read_splat_cells_bytes(n)
 * out, a few milliseconds); read_splat_cells_build_host() writes the same blob on the host (multi-threaded; the caller uploads
 * it, e.g. after one rank built it for all).  The blob (256-byte aligned) is then passed to read_splat_forward_cells().
 * Whole chunks outside the frustum, or behind the far depth bound of every 4x4 pixel block they can touch, are then
 * skipped without reading their points, and the z-test runs XCD-striped against an L2-resident bound image
 * (csrc/splat.hip).  The tail of the blob is per-frame scratch (chunk lists), so one blob serves one stream at a
 * time.  With cells == NULL, B > 1, n < 2^20, W % 16 != 0 or sizes that are not multiples of 2^(levels-1) the call is
 * exactly read_splat_forward(). */
/* read_splat_hint_next_camera(workspace, M_next_host): optional, before a read_splat_forward_cells call — "the NEXT call on this
 * workspace will use camera M_next" (16 floats on the host; NULL withdraws the hint).  A sweep, a trajectory replay or a viewer
 * that extrapolates its camera knows that matrix one frame ahead.  The hinted frame's last launch then also does the next frame's
 * first one (chunk classification for M_next, seeds re-projected with M_next into the other bound image): a frame is 4 dependent
 * launches instead of 5.  Purely a performance device with identical results: if the next call comes with another matrix, size or
 * tuning state, the prepared state is wiped (two small memsets) and the frame runs as without a hint.  The hint is consumed by
 * the next forward call on the workspace; the frame counter behind it lives on the host, keyed by the workspace address. */
int read_splat_hint_next_camera(void *workspace, const float *M_next_host);
/* Per-kernel durations (ms) of the LAST cell-path frame, HIP events on the launch stream around every launch; needs
 * read_tuning_set("splat_prof", 1) before the frame.  ms5[0] seeds + classification (0 when the previous frame's resolve launch did
 * that work), [1] pass A, [2] bin merge + bounds, [3] pass B (+ the object launches of read_splat_forward_objects), [4] resolve (+ the
 * next frame's seeds / classification).  Synchronises. */
int read_splat_profile_last(float *ms5);
size_t read_splat_cells_bytes(int64_t n);
int read_splat_cells_build_host(const float *xyz_host, int64_t n, void *cells_host, size_t cells_bytes);
/* The same blob built on the device from a cloud already in HBM (xyz, cells and scratch are device pointers; cells and scratch
 * 256-byte aligned): byte for byte what read_splat_cells_build_host writes, except possibly the sign of a zero in a min / max
 * field.  Stream-ordered; allocates nothing: the caller provides read_splat_cells_build_scratch_bytes(n) bytes of scratch
 * (0 when n is out of range; about 8 bytes per point).  A non-finite point fails with the host builder's message and the smallest
 * bad index, the blob left as it was; that costs one small device -> host read and one synchronisation of the stream at the end
 * of the call, the only one.  Rewriting a blob in place includes read_splat_cells_invalidate(cells, n). */
size_t read_splat_cells_build_scratch_bytes(int64_t n);
int read_splat_cells_build(const float *xyz_dev, int64_t n, void *cells_dev, size_t cells_bytes, void *scratch_dev,
                           size_t scratch_bytes, void *stream);
/* The library keeps host-side bookkeeping per cell blob ADDRESS (which frames ran over its chunk lists; a frame prepared for an
 * announced camera is only consumed while nothing else touched them).  Whoever rewrites a blob in place, copies another cloud's
 * blob over it, or frees it (the allocator may hand the address out again) calls this: pending preparations made against the old
 * contents then no longer match and are wiped instead of consumed, and the entry is forgotten.  Cheap; no device work. */
int read_splat_cells_invalidate(const void *cells, int64_t n);
int read_splat_forward_cells(const float *xyz, void *cells, int64_t n, const float *M_host, int B, int W, int H,
                             int levels, int32_t *const *idx_levels, float *const *depth_levels,
                             void *workspace, size_t workspace_bytes, void *stream);

/* Scene editing (csrc/splat.hip, range_splat_kernel<PinholeCam>).  A scene = a static part (label 0) plus objects k = 0..count-1, each with its
 * own matrix M_k = M_0 @ P_k (P_k maps the object's points, in the cloud's coordinates, to their new place; computed on the host).
 * Every visible point is projected with its label's matrix by the arithmetic of every pass; per pixel the minimum (depth, ORIGINAL
 * id) wins, empty pixels are (0, 0.0f), levels are formed as in read_splat_forward.  Index images carry the original ids.
 *
 * read_splat_cells_build_ids: read_splat_cells_build of the static part's own xyz (n points, gathered), whose records carry
 *   ids[i] (device, n entries: the original ids) instead of i.  Same blob otherwise, same scratch, same checks. */
int read_splat_cells_build_ids(const float *xyz_dev, const int32_t *ids_dev, int64_t n, void *cells_dev, size_t cells_bytes,
                               void *scratch_dev, size_t scratch_bytes, void *stream);
typedef struct read_splat_objects {
    const float *xyz;              /* device, n x 3: every object's points, object after object */
    const int32_t *ids;            /* device, n: their original ids */
    int64_t n;
    int count;
    const int64_t *begin;          /* host, count + 1: object k = points [begin[k], begin[k+1]); begin[0] = 0, begin[count] = n */
    const float *M;                /* host, count x 16 row-major: M_k */
    const unsigned char *visible;  /* host, count entries (0 = hidden, not launched), or NULL = all visible */
} read_splat_objects;
/* One camera M_host (= M_0, 16 floats on the host) over the static part (xyz_static / ids_static, n_static points, device; cells =
 * its blob from read_splat_cells_build_ids or NULL) and the objects.  With cells, n_static >= 2^20 and W % 16 == 0 the static part
 * takes the cell path (read_splat_hint_next_camera applies to it) and the objects join the key image after its pass B; otherwise
 * the static part is one more object range with M_0.  Stream-ordered, allocates nothing, no synchronisation; workspace of
 * read_splat_workspace_bytes(1, W, H).  READ_EINVAL before any device work for null pointers, objs->begin not starting at 0 or
 * not monotone, begin[count] != n, and W or H not a multiple of 2^(levels-1). */
int read_splat_forward_objects(const float *xyz_static, const int32_t *ids_static, void *cells, int64_t n_static,
                               const float *M_host, int W, int H, int levels, const read_splat_objects *objs,
                               int32_t *const *idx_levels, float *const *depth_levels, void *workspace, size_t workspace_bytes,
                               void *stream);

/* Panorama camera: cylindrical projection (csrc/splat.hip, range_splat_kernel<PanoCam>; the definition is tests/pano_model.py).  cam_host =
 * 16 floats on the host (camera.pano_camera): [0..11] three rows applied to (x, y, z, 1) giving c0 = x_c, c1 = P[1,1] y_c and
 * c3 = -z_c (the forward distance), [12] kx = 2 / hfov_rad, [13] ky = P[1,2], [14] za = P[2,2], [15] zb = P[2,3].  Per point, in
 * fp32 without fused operations: rho = sqrt(c0 c0 + c3 c3), nx = atan2(c0, c3) kx, ny = c1 / rho - ky, nz = (zb - za rho) / rho,
 * then pixel and depth as in every pass.  Per pixel the minimum (depth, id) wins, empty pixels are (0, 0.0f), levels are formed
 * as in read_splat_forward.
 *
 * xyz / ids / n (device): the cloud, or a labelled cloud's static part; ids == NULL: the id is the point's index.  objs: NULL, or
 * the objects of read_splat_forward_objects with objs->M = count x 16 floats in the panorama layout (the rows of object k are
 * (R4 @ P_k)[:3], R4 = the camera's rows with (0, 0, 0, 1) beneath; the four scalars repeat).  With objs == NULL and ids == NULL
 * the previous frame's winners warm-start the pass; nothing is culled (a cylinder does not take a box to the hull of its
 * corners).  Stream-ordered, allocates nothing, no synchronisation; workspace of read_splat_workspace_bytes(1, W, H), left
 * EMPTY — pinhole and panorama frames may alternate on it.  READ_EINVAL before any device work for null pointers, W or H not a
 * multiple of 2^(levels-1), non-finite camera entries, kx outside [1/pi, inf), and a malformed objs->begin. */
int read_splat_forward_pano(const float *xyz, const int32_t *ids, int64_t n, const float *cam_host, int W, int H, int levels,
                            const read_splat_objects *objs, int32_t *const *idx_levels, float *const *depth_levels,
                            void *workspace, size_t workspace_bytes, void *stream);
/* read_splat_project_points under a panorama camera: the same device function as read_splat_forward_pano's pass. */
int read_splat_pano_project_points(const float *xyz, int64_t n, const float *cam_host, int W, int H, int32_t *pixel, float *depth,
                                   void *stream);

/* Scene editing, third verb: ADD.  An instance = (a range of one point pool, its own matrix, a visible flag); ranges may repeat and
 * overlap, so one object (a labelled cluster, or a "foreign" object cut out of another fitted scene and appended to the pool with
 * ids N, N + 1, ... past the scene's) is drawn as often as it is listed.  Per pixel the minimum of depth bits << 32 | id over every
 * visible point of every visible instance and of the static part wins; two copies of one point at the same pixel and depth have the
 * same key.  The list may have any length (32 ranges per launch); hidden and empty instances are not launched.  The definition is
 * tests/instances_model.py. */
typedef struct read_splat_instances {
    const float *xyz; const int32_t *ids; int64_t n;   /* device: the point pool (own objects' points, then foreign ones) */
    int count;                                         /* instances */
    const int64_t *first; const int64_t *npts;         /* host, count each: instance i draws pool points [first[i], first[i] + npts[i]) */
    const float *M;                                    /* host, count x 16: M_i (pinhole), the panorama layout of read_splat_forward_pano, or 12 rows + 4 ignored (read_splat_forward_lens) */
    const unsigned char *visible;                      /* host, count, or NULL */
} read_splat_instances;
/* read_splat_forward_objects with an instance list in place of the partition: same routes (cell path for the static part with cells,
 * n_static >= 2^20 and W % 16 == 0, the instances after its pass B; otherwise the static part is one more range with M_0), same
 * workspace, stream ordering and read_splat_hint_next_camera behaviour; allocates nothing, no synchronisation.  With the list
 * first[k] = begin[k], npts[k] = begin[k + 1] - begin[k] the result is read_splat_forward_objects', bit for bit.  READ_EINVAL before
 * any device work for null pointers, count < 0, a negative first or npts, first + npts > n, and W or H off the pyramid. */
int read_splat_forward_instances(const float *xyz_static, const int32_t *ids_static, void *cells, int64_t n_static,
                                 const float *M_host, int W, int H, int levels, const read_splat_instances *inst,
                                 int32_t *const *idx_levels, float *const *depth_levels,
                                 void *workspace, size_t workspace_bytes, void *stream);
/* read_splat_forward_pano with an instance list (inst must not be NULL; no warm start): xyz / ids / n as there (ids == NULL: the id is
 * the point's index).  Also refuses non-finite camera entries and kx < 1 / pi, of cam_host and of every instance that is drawn. */
int read_splat_forward_pano_instances(const float *xyz, const int32_t *ids, int64_t n, const float *cam_host,
                                      int W, int H, int levels, const read_splat_instances *inst,
                                      int32_t *const *idx_levels, float *const *depth_levels,
                                      void *workspace, size_t workspace_bytes, void *stream);

/* Lens cameras: a pinhole with Brown-Conrady distortion (model 0) and a Kannala-Brandt fisheye (model 1) (csrc/splat.hip,
 * range_splat_kernel<LensCam>; the definition is tests/lens_model.py).  cam_host = 32 floats on the host (camera.lens_camera): [0..11] three
 * UNSCALED rows applied to (x, y, z, 1) giving c0 = x_c, c1 = y_c and c3 = -z_c (the forward distance); [12] sx = P[0,0],
 * [13] ox = P[0,2], [14] sy = P[1,1], [15] oy = P[1,2]; [16] za = P[2,2], [17] zb = P[2,3]; [18] the limit; [19] the model, 0.0f or
 * 1.0f; [20..24] the coefficients (model 0: OpenCV's k1, k2, p1, p2, k3; model 1: OpenCV's fisheye k1..k4); [25..31] zero.  Per
 * point, in fp32 without fused operations — model 0: a = c0 / c3, b = c1 / c3, r2 = a a + b b, drawn only if c3 > 0 and
 * r2 <= limit, (a', b') = the distorted (a, b), d = c3; model 1: rho = sqrt(c0 c0 + c1 c1), theta = atan2(rho, c3), drawn only if
 * theta <= limit, (a', b') = (c0, c1) theta_d(theta) / rho (the axis point rho = 0 lands on the principal point),
 * d = sqrt(c0 c0 + c1 c1 + c3 c3) — then nx = sx a' - ox, ny = sy b' - oy, nz = (zb - za d) / d and pixel and depth as in every
 * pass.  Per pixel the minimum (depth, id) wins, empty pixels are (0, 0.0f), levels are formed as in read_splat_forward.
 *
 * xyz / ids / n, objs, the warm start, the workspace (left EMPTY; pinhole, panorama and lens frames may alternate on it in any
 * order), stream ordering: as for read_splat_forward_pano.  objs->M (and inst->M) = count x 16 floats: the 12 rows of object k,
 * (R4 @ P_k)[:3] with R4 = the camera's rows and (0, 0, 0, 1) beneath, then 4 floats that are ignored; the twenty scalars are the
 * frame's.  READ_EINVAL before any device work for null pointers, W or H not a multiple of 2^(levels-1), non-finite camera entries
 * (the limit of model 0 may be +inf), a model other than 0 or 1, a limit that is negative or NaN or above pi for model 1, and a
 * malformed objs->begin (inst->first, inst->npts). */
int read_splat_forward_lens(const float *xyz, const int32_t *ids, int64_t n, const float *cam_host, int W, int H, int levels,
                            const read_splat_objects *objs, int32_t *const *idx_levels, float *const *depth_levels,
                            void *workspace, size_t workspace_bytes, void *stream);
/* read_splat_forward_lens with an instance list (inst must not be NULL; no warm start). */
int read_splat_forward_lens_instances(const float *xyz, const int32_t *ids, int64_t n, const float *cam_host,
                                      int W, int H, int levels, const read_splat_instances *inst,
                                      int32_t *const *idx_levels, float *const *depth_levels,
                                      void *workspace, size_t workspace_bytes, void *stream);
/* read_splat_project_points under a lens camera: the same device function as read_splat_forward_lens's pass. */
int read_splat_lens_project_points(const float *xyz, int64_t n, const float *cam_host, int W, int H, int32_t *pixel, float *depth,
                                   void *stream);

/* LiDAR sweep: the range image and the point list of a spinning LiDAR placed in the fitted scene (csrc/lidar.hip; the definition
 * is tests/lidar_model.py).  cam_host = 16 floats on the host (camera.lidar_camera): [0..11] three UNSCALED rows applied to
 * (x, y, z, 1) giving c0 = x_c, c1 = y_c and c3 = -z_c (forward), [12] kx = 2 / hfov_rad, [13] rmin > 0, [14] rmax >= rmin,
 * [15] delta >= 0, a beam's acceptance half-width in radians.  elev_host = B beam elevations in radians on the host, finite and
 * strictly ascending, 1 <= B <= 128; row b of every image is beam b.  W = azimuth columns, B W < 2^31.  Per point, in fp32 without
 * fused operations: q = c0 c0 + c3 c3, rho = sqrt(q), theta = atan2(c0, c3), phi = atan2(c1, rho), r = sqrt(q + c1 c1); column =
 * (int)((W (theta kx + 1)) 0.5) while -1 <= theta kx <= 1 and the column is below W; beam = the b of the smallest
 * |phi - elev[b]| (ties to the lower b) while that is <= delta; drawn while rmin <= r <= rmax.  Per cell b W + column the minimum of
 * range bits << 32 | id wins.
 *
 * The see-through filter then works on the complete image: a return of range r is kept iff r <= near scale + slack, near = the
 * smallest range among the returns with |db| <= wb, |dc| <= wc (rows clipped; columns modulo W iff wrap, else clipped; the cell
 * itself counts); wb = wc = 0 keeps everything.  Outputs, each NULL or a device buffer: range / idx (B x W; empty cells 0.0f / 0);
 * count (one int32: the kept returns, also beyond capacity); cell / ret_id (capacity each) and ret_xyz (capacity x 3): the first
 * min(count, capacity) kept returns in ascending cell order, ret_xyz in the sensor frame along the beam —
 * x = (r ce_b) st_c, y = r se_b, z = -((r ce_b) ct_c) from the device tables beam_dir (B x 2: cos, sin of elev[b]) and col_dir
 * (W x 2: sin, cos of ((c + 0.5) / W 2 - 1) / kx), each formed on the host in float64 and rounded once; they are needed only with
 * ret_xyz.
 *
 * xyz / ids / n (device): the cloud, or a labelled cloud's static part; ids == NULL: the id is the point's index.  inst: NULL, or
 * the list of read_splat_forward_pano_instances with inst->M = count x 16 floats in the LiDAR layout (rows (R4 @ P_i)[:3], the four
 * scalars repeat).  The workspace is the sweep's own (read_lidar_workspace_bytes(B, W), 256-byte aligned, filled once by
 * read_lidar_workspace_init): every sweep leaves all of it as init did, so sweeps of any sizes that fit follow each other on it
 * without a memset, and the rasteriser's workspace is not touched — frames and sweeps interleave freely.  Stream-ordered, allocates
 * nothing, no synchronisation, no kernel waits for another workgroup.  READ_EINVAL with a message naming the call, before any
 * device work, for: null pointers with work to do; B outside 1..128, W < 1, B W >= 2^31; a table that is not finite and strictly
 * ascending; non-finite camera entries, also of every drawn instance; kx < 1 / pi; rmin <= 0; rmax < rmin; delta < 0; wb or wc
 * outside 0..4; scale < 1 or slack < 0 or either not finite; capacity < 0; a malformed instance list; READ_ENOMEM for a workspace
 * that is too small. */
size_t read_lidar_workspace_bytes(int B, int W);
int read_lidar_workspace_init(void *workspace, size_t workspace_bytes, void *stream);
typedef struct read_lidar_args {
    const float *xyz; const int32_t *ids; int64_t n;   /* device: the cloud or the static part; ids NULL = the indices */
    const read_splat_instances *inst;                  /* NULL, or the instance list (M in the LiDAR layout) */
    const float *cam_host;                             /* host, 16 */
    const float *elev_host;                            /* host, B */
    int B, W;
    const float *beam_dir; const float *col_dir;       /* device, B x 2 and W x 2; may be NULL without ret_xyz */
    int wb, wc, wrap;                                  /* the filter's window (0..4 each) and whether columns wrap */
    float scale, slack;                                /* lim = near scale + slack; scale = fp32(1 + rel) >= 1, slack >= 0 */
    float *range; int32_t *idx;                        /* device, B x W each, or NULL */
    int32_t *count;                                    /* device, 1, or NULL */
    int32_t *cell; int32_t *ret_id; float *ret_xyz;    /* device, capacity (x 3), or NULL */
    int64_t capacity;
    void *workspace; size_t workspace_bytes;
} read_lidar_args;
int read_lidar_sweep(const read_lidar_args *args, void *stream);
/* The per-point function of read_lidar_sweep's pass alone: cell[i] = the cell of point i or -1, range[i] = its range (0.0f where
 * cell[i] = -1).  Same checks of cam_host, elev_host, B and W. */
int read_lidar_project_points(const float *xyz, int64_t n, const float *cam_host, const float *elev_host, int B, int W,
                              int32_t *cell, float *range, void *stream);

/* Measurement aid for bench.py (roofline.mfma_sustained): one workgroup of four waves per CU, every wave `iters` rounds of 16 independent
 * v_mfma_f32_16x16x4_f32 and nothing else.  scratch: >= 256 floats per CU on the device (never written); *flops receives the number of
 * floating-point operations the launch executes — the caller times the launch on `stream`.  Not on the render path. */
int read_mfma_f32_rate_probe(int iters, float *scratch, double *flops, void *stream);

/* GL twin features of the rasteriser (READ/gl/programs.py:121-198, READ/gl/render.py:52-85, READ/gl/dataset.py:39-82,
 * READ/datasets/dynamic.py:235-239): ONE level of ONE camera rasterised at its own size W x H with
 *   point_size / relative / min_point_size   "pN" tokens: a square of N pixels; "psN" tokens (relative = 1): side
 *                                             max(min_point_size, N / clip.z); never below one pixel
 *   discard                                   optional device array of N bytes, 1 = point not drawn (set_point_discard)
 *   drop_threshold, drop_seed                 seeded drop: point i is dropped iff rnd(i, seed) < threshold (0 = off);
 *                                             threshold = p * (2^32 - 1)
 *   perturb                                   optional device array N x 2 added to clip.xy (set_point_perturb)
 *   perturb_amp, perturb_seed                 seeded perturbation amp * (u01(i, seed) - 0.5) per axis (0 = off)
 * Coverage rule = OpenGL's basic point rasterisation with GL_PROGRAM_POINT_SIZE (READ/gl/render.py:55; GL 4.6 core spec
 * section 14.4.1: "a fragment for each framebuffer pixel whose center lies inside a square centered at the point's (xw, yw), with
 * side length equal to the current point size"): pixel column i is covered iff xw - s/2 <= i + 0.5 < xw + s/2, i.e.
 * i in [floor(u - (s-1)/2), floor(u + (s-1)/2)] away from exact ties — for odd AND even s; points are clipped by their CENTRE
 * (spec 13.7: a point outside the clip volume is discarded whole), sizes clamp to [1, 4096] (the aliased point size range).
 * Exact semantics: csrc/splat.hip (splat_project_gl_kernel) == oracle/raster.c (oracle_raster_level_gl).  With the default
 * options {1, 0, 1, NULL, 0, 0, NULL, 0, 0, NULL} the result equals read_splat_forward(levels = 1).  The workspace is the one of
 * read_splat_workspace_bytes(1, W, H); it is left EMPTY. */
typedef struct read_splat_gl_opts {
    float point_size;
    int relative;
    float min_point_size;
    const unsigned char *discard;
    uint32_t drop_threshold, drop_seed;
    const float *perturb;
    float perturb_amp;
    uint32_t perturb_seed;
    const float *point_sizes;    /* optional device array of N per-point sizes (NNScene.set_point_sizes, the a_point_size vertex
                                  * attribute): used instead of point_size when point_size == 0 (the shader's
                                  * "if (point_size < 1) point_size = a_point_size", READ/gl/programs.py:183-187, :339-345) */
} read_splat_gl_opts;
int read_splat_forward_gl(const float *xyz, int64_t n, const float *M_host, int W, int H,
                          const read_splat_gl_opts *opts, int32_t *idx, float *depth, void *workspace,
                          size_t workspace_bytes, void *stream);

/* out[i] = (float)idx[i] — the reference's index image dtype (ids >= 2^24 round). */
int read_index_to_float(const int32_t *idx, int64_t count, float *out, void *stream);
/* Projection alone (point_render.cu:110-147 without the z-test of :149-166): pixel[i] = yy * W + xx of point i under the
 * row-major 4x4 matrix M_host, or -1 when the point is clipped or falls outside the image; depth[i] (may be NULL) = (nz + 1) / 2
 * as the rasteriser computes it, also for rejected points.  The same device function as every rasteriser pass — per-point
 * visibility for a host, and the entry the division test drives (tests/test_gpu_splat.py). */
int read_splat_project_points(const float *xyz, int64_t n, const float *M_host, int W, int H, int32_t *pixel, float *depth,
                              void *stream);

/* ---------------------------------------------------------------- object selection (extension) */

/* Per-point object labels made on the device: the front end of scene editing.  The contract is tests/select_model.py, held bit
 * for bit: fp32, sums left to right, no fused operations, a comparison with a NaN is false.  Every pointer is a device pointer
 * except M_host; no call allocates or synchronises; n == 0 succeeds without a launch; null pointers are refused when n > 0.
 *
 * read_select_boxes: boxes = K x 12 floats, each a row-major 3x4 matrix A that maps cloud coordinates to the unit cube; point i is
 *   inside box k iff |A[4r] x + A[4r+1] y + A[4r+2] z + A[4r+3]| <= 1 for r = 0, 1, 2 (faces inclusive; a non-finite point is
 *   outside).  labels_out[i] = label_of[k] of the smallest such k, else labels_in[i] (labels_in NULL: 0).  0 <= K <= 1024; K = 0
 *   copies labels_in or zero-fills.  labels_in may be labels_out. */
int read_select_boxes(const float *xyz, int64_t n, const float *boxes, const int32_t *label_of, int K, const int32_t *labels_in,
                      int32_t *labels_out, void *stream);
/* read_select_near: near[p] for the W*H pixels of a level-0 frame (idx0, depth0 as read_splat_forward writes them) of this cloud
 *   under the pinhole matrix M_host: +inf where the pixel is empty (idx0 = 0 and the bits of depth0 = 0) or idx0 is no id of the
 *   cloud, else the clip w (M[12] x + M[13] y + M[14] z + M[15]) of point idx0[p] — for get_proj_matrix projections the metric
 *   distance along the camera axis.  W * H < 2^31. */
int read_select_near(const float *xyz, int64_t n, const float *M_host, int W, int H, const int32_t *idx0, const float *depth0,
                     float *near, void *stream);
/* read_select_vote: one view's vote into state (one uint32 per point: cand << 16 | hit << 8 | seen, zero before the first view).
 *   Point i projects as in read_splat_project_points; outside the image nothing changes; with lim = near[pix] * scale + slack,
 *   unless clip w <= lim nothing changes (occluded); else seen += 1 and, m = mask[pix] (int32 image, values in [0, 65535], 0 = no
 *   object): m != 0 and cand = 0 -> cand = m, hit = 1; m = cand -> hit += 1.  The candidate is the label of the FIRST view that
 *   names one.  scale >= 1 and slack >= 0, both finite.  At most 255 views per state: the counters are 8 bits wide and the caller
 *   counts the views. */
int read_select_vote(const float *xyz, int64_t n, const float *M_host, int W, int H, const float *near, const int32_t *mask,
                     float scale, float slack, uint32_t *state, void *stream);
/* read_select_finish: labels_out[i] = cand iff cand != 0, hit >= min_hits and hit * den >= num * seen; else labels_in[i]
 *   (labels_in NULL: 0; it may be labels_out).  1 <= min_hits <= 255, den >= 1, 0 <= num <= den. */
int read_select_finish(const uint32_t *state, int64_t n, int min_hits, int num, int den, const int32_t *labels_in,
                       int32_t *labels_out, void *stream);

/* ---------------------------------------------------------------- frame annotations (extension) */

/* What drew each pixel of an edited frame, and per-instance 2-D boxes: the back end of scene editing (csrc/annotate.hip).  The
 * contract is tests/annotate_model.py, held bit for bit.  The frame is a LEVEL-0 pinhole frame of read_splat_forward_instances
 * (idx0, depth0), the tables describe the instance list it was drawn with — same pool, same matrices M_i, bit for bit.
 *
 * Per pixel p: empty (idx0 = 0 and the bits of depth0 = 0) -> obj = inst = -1.  Otherwise id = idx0[p]: for 0 <= id < n the object is
 * k = labels[id] (labels NULL: 0) and the point xyz[id]; for id in foreign range f, [id_base_f, id_base_f + n_f), the object is
 * k = K_own + 1 + f and the point pool_xyz[pool_first_f + id - id_base_f].  k = 0: obj = 0, inst = -1.  k >= 1: obj = k and inst =
 * value[i] of the FIRST instance i in list order that is visible, draws object k and under whose M_i the point projects
 * (read_splat_project_points' device function) to pixel p with depth bits equal to depth0[p]'s; none: inst = -1 and *unmatched += 1.
 * An id no range holds, or a label outside [0, K_own]: obj = inst = -1 and *unmatched += 1.  On a frame and list that belong together
 * *unmatched is 0.
 *
 * stats[i][0..11] (int32) of instance i, by list position: vis_px = pixels instance i won; vx0, vy0, vx1, vy1 = their inclusive box;
 * in_pts = how many of its points project inside the image; ax0, ay0, ax1, ay1 = the inclusive box of those points' pixels (the
 * amodal box, clipped to the image); near_bits = the smallest depth bit pattern among them; n_pts = npts[i].  An empty minimum is
 * INT32_MAX, an empty maximum -1; a hidden instance keeps n_pts and is otherwise empty.  Integer min / max / add: order-free.
 *
 * The instance table is passed twice: on the HOST for the checks and the extents walk (32 ranges per launch, matrices in kernel
 * arguments, hidden and empty instances not launched), and on the DEVICE for the pixel pass, where a pixel walks only the instances of
 * its own object: d_obj_begin[k - 1] .. d_obj_begin[k] index d_obj_list, the list positions of object k's instances, ascending
 * (K = K_own + n_foreign objects, d_obj_begin has K + 1 entries, d_obj_list has `count`).  The caller keeps the two in step. */
#define READ_ANNOTATE_STATS 12
typedef struct read_annotate_foreign {
    int64_t id_base, n, pool_first;        /* ids [id_base, id_base + n) are pool points [pool_first, pool_first + n) */
} read_annotate_foreign;
typedef struct read_annotate_args {
    const float *xyz; int64_t n;           /* device: the scene cloud, n x 3 */
    const int32_t *labels;                 /* device, n, or NULL = every point static */
    int K_own;                             /* own objects: labels lie in [0, K_own] */
    int n_foreign;                         /* 0 .. READ_GATHER_MAX_TABLES - 1 */
    const read_annotate_foreign *foreign;  /* host, n_foreign: id bases ascend from n without overlap */
    const float *pool_xyz; int64_t pool_n; /* device: the point pool of read_splat_instances */
    int count;                             /* instances I */
    const int64_t *first; const int64_t *npts;   /* host, count each */
    const int32_t *obj;                    /* host, count: the object (1..K) instance i draws */
    const float *M;                        /* host, count x 16: M_i */
    const unsigned char *visible;          /* host, count, or NULL = all visible */
    const float *d_M;                      /* device, count x 16: the same matrices */
    const int32_t *d_visible;              /* device, count: 0 = hidden */
    const int32_t *d_value;                /* device, count: what inst[p] shows for instance i (the caller's handle) */
    const int32_t *d_npts;                 /* device, count: npts as int32 */
    const int32_t *d_obj_begin;            /* device, K + 1 */
    const int32_t *d_obj_list;             /* device, count */
    const int32_t *idx0; const float *depth0; int W, H;      /* device: the level-0 frame */
    int32_t *out_obj, *out_inst;           /* device, W * H each */
    int32_t *stats;                        /* device, count x READ_ANNOTATE_STATS */
    int32_t *unmatched;                    /* device, 1 */
} read_annotate_args;
/* Stream-ordered, allocates nothing, no synchronisation: one init launch (the statistics rows and *unmatched), the pixel pass (16 B
 * per pixel), ceil(drawn / 32) extents launches (12 B per drawn point).  count = 0: obj from the labels and inst = -1, no instance
 * walk, no table read.  READ_EINVAL with a message, before any device work, for: null pointers with work to do, W or H < 1 or
 * W * H >= 2^31, n, K_own, count or pool_n below 0 (pool_n above INT32_MAX), n_foreign outside 0 .. READ_GATHER_MAX_TABLES - 1, an
 * object number outside [1, K], foreign bases that do not ascend from n (or overlap, or pass INT32_MAX, or leave the pool), a
 * negative first or npts, first + npts past the pool. */
int read_annotate_frame(const read_annotate_args *args, void *stream);

/* ---------------------------------------------------------------- frame flow (extension) */

/* Where each pixel's surface point goes in the next frame: optical flow, the depth there and whether it is still seen, between two
 * states of one edited scene (csrc/flow.hip).  The contract is tests/flow_model.py, held bit for bit.  State A (idx0, depth0, M0, d_M,
 * d_visible) is the frame the labels live on, state B (idx0_next, depth0_next, M0_next, d_M_next, d_visible_next) the frame they point
 * into: both are LEVEL-0 pinhole frames of read_splat_forward_instances over the same cloud, labels, pool and W x H, and the B tables
 * are indexed by A's list positions (an instance that B no longer has is hidden there).
 *
 * Per pixel p of A: empty (idx0 = 0 and the bits of depth0 = 0) -> state EMPTY.  Otherwise id -> object k and point as in
 * read_annotate_frame.  The drawer: for k = 0 the static scene (M0 / M0_next; M0 must reproduce pixel p and depth0[p]'s bits), for
 * k >= 1 the FIRST instance i in list order that is visible in A, draws k and under whose d_M[i] the point projects to pixel p with
 * depth0[p]'s bits (the annotation's walk).  No drawer, an id no range holds, or a static point M0 does not reproduce: UNMATCHED and
 * *unmatched += 1.  With u = ((float)W (nx + 1)) 0.5f, v = ((float)H (1 - ny)) 0.5f the continuous pixel coordinates of the point (the
 * pixel is their integer part) and d = (nz + 1) 0.5f — fp32, no contraction, sums left to right, IEEE division —: (u_a, v_a) under A's
 * drawer matrix, (u_b, v_b, d_b) and the pixel q under B's.  The drawer hidden in B: HIDDEN.  q >= 0: VISIBLE iff idx0_next[q] = id and
 * the bits of depth0_next[q] equal d_b's (a tie of two copies of one point counts as visible), else OCCLUDED.  q = -1 with nz in
 * [-1, 1] and nx, ny finite: OFF_IMAGE; any other q = -1: CLIPPED.
 *
 * flow[p] = (u_b - u_a, v_b - v_a) and depth_next[p] = d_b for VISIBLE, OCCLUDED and OFF_IMAGE; +0.0f, all three, for every other state.
 * counts[s] = pixels in state s (counts[7] stays 0).  stats[i][0..3] of instance i, by list position: px (pixels it drew in A), visible,
 * occluded, outside (OFF_IMAGE + CLIPPED); an instance hidden in B keeps px only.  Integer adds: order-free. */
#define READ_FLOW_STATES 8
#define READ_FLOW_STATS  4
#define READ_FLOW_EMPTY     0
#define READ_FLOW_VISIBLE   1
#define READ_FLOW_OCCLUDED  2
#define READ_FLOW_OFF_IMAGE 3
#define READ_FLOW_CLIPPED   4
#define READ_FLOW_HIDDEN    5
#define READ_FLOW_UNMATCHED 6
typedef struct read_flow_args {
    const float *xyz; int64_t n;           /* device: the scene cloud, n x 3 */
    const int32_t *labels;                 /* device, n, or NULL = every point static */
    int K_own;                             /* own objects: labels lie in [0, K_own] */
    int n_foreign;                         /* 0 .. READ_GATHER_MAX_TABLES - 1 */
    const read_annotate_foreign *foreign;  /* host, n_foreign: id bases ascend from n without overlap */
    const float *pool_xyz; int64_t pool_n; /* device: the point pool of read_splat_instances */
    int count;                             /* instances I of state A */
    const int32_t *obj;                    /* host, count: the object (1..K) instance i draws (checked, not uploaded) */
    const float *d_M;                      /* device, count x 16: M_i of state A */
    const int32_t *d_visible;              /* device, count: 0 = hidden in A */
    const int32_t *d_obj_begin;            /* device, K + 1 */
    const int32_t *d_obj_list;             /* device, count */
    const float *d_M_next;                 /* device, count x 16: M_i of state B, by A's list positions */
    const int32_t *d_visible_next;         /* device, count: 0 = hidden in B (or gone) */
    const float *M0; const float *M0_next; /* host, 16 each: the cameras of A and B; they travel in the kernel arguments */
    const int32_t *idx0; const float *depth0;             /* device: A's level-0 frame */
    const int32_t *idx0_next; const float *depth0_next;   /* device: B's level-0 frame */
    int W, H;
    float *flow;                           /* device, W * H x 2, 8-byte aligned */
    float *depth_next;                     /* device, W * H */
    int32_t *state;                        /* device, W * H */
    int32_t *counts;                       /* device, READ_FLOW_STATES */
    int32_t *stats;                        /* device, count x READ_FLOW_STATS */
    int32_t *unmatched;                    /* device, 1 */
} read_flow_args;
/* Stream-ordered, allocates nothing, no synchronisation: one init launch (counts, the statistics rows and *unmatched) and the pixel
 * pass (8 B read and 16 B written per pixel, plus the points).  count = 0: no table is read, object pixels are UNMATCHED and static
 * pixels flow.  READ_EINVAL with a message, before any device work, for: null pointers with work to do (flow not 8-byte aligned
 * included), W or H < 1 or W * H >= 2^31, n, K_own, count or pool_n below 0 (n or pool_n above INT32_MAX), n_foreign outside
 * 0 .. READ_GATHER_MAX_TABLES - 1, an object number outside [1, K], foreign bases that do not ascend from n (or overlap, or pass
 * INT32_MAX, or leave the pool), a non-finite entry of M0 or M0_next. */
int read_flow_frame(const read_flow_args *args, void *stream);

/* ---------------------------------------------------------------- descriptor gather / scatter */

/* (C, N) channel-major texture  ->  N x C row-major rows (and back, for gradients). */
int read_texture_to_rows(const float *tex_cn, int64_t n, int C, float *rows_nc, void *stream);
int read_rows_to_texture(const float *rows_nc, int64_t n, int C, float *tex_cn, void *stream);

/*
 * feat_l[p][c] = act(rows[idx_l[p]][c])  for every level l and pixel p (NHWC, C % 4 == 0, C <= 64).
 *   count_levels[l] = number of pixels of level l (B*h_l*w_l; 0 = an empty level, its pointers may be NULL);
 *   activation: 0 none, 1 sigmoid, 2 tanh.  An id below 0 reads row 0, an id >= n reads row n - 1 (the clamp of the table gather).
 *   Activation 0 hands the row's bits through (-0, subnormals and NaN payloads included); NaN gives NaN, +-inf gives 0 / 1 / +-1.
 */
int read_gather_forward(const float *rows_nc, int64_t n, int C, int levels,
                        const int32_t *const *idx_levels, const int64_t *count_levels,
                        float *const *feat_levels, int activation, void *stream);
/* Supersampled lookup (READ/gl/nn.py:100-101 + READ/models/compose.py:162-163): index maps rendered at ss x the feature
 * size; feat_l = bilinear-downscale-by-ss (align_corners = False, torch's F.interpolate(scale_factor = 1/ss)) of the
 * activated samples, fused: each output pixel blends the four samples around source coordinate (o + 0.5) * ss - 0.5.
 *   h_levels[l], w_levels[l] = OUTPUT size of level l; idx_l is [B][ss*h][ss*w]; feat_l is [B][h][w][C].
 *   ss = 1..8, ids clamped as in read_gather_forward.  For odd ss the source coordinate is an integer: the output is the activated
 *   centre sample, bit for bit what read_gather_forward returns for that id (ss = 1: read_gather_forward itself), whatever its
 *   neighbours hold.  For even ss it is the mean of four activated samples (weights 1/4, at most three rounded additions); a
 *   non-finite sample makes the outputs that blend it non-finite. */
int read_gather_forward_ss(const float *rows_nc, int64_t n, int C, int levels, int B,
                           const int32_t *const *idx_levels, const int *h_levels, const int *w_levels, int ss,
                           float *const *feat_levels, int activation, void *stream);
/* The gather over several descriptor tables (csrc/gather.hip, gather_tables_kernel; the definition is tests/instances_model.py): an
 * index image may carry ids of objects that were added to a scene with their own small tables, and the scene's table is never copied
 * to append them.  Table t of count (1..READ_GATHER_MAX_TABLES) serves ids in [id_base_t, id_base_t + n_t); id_base_0 = 0, bases
 * ascend, ranges do not overlap (gaps may remain).  feat_l[p][:] = act_t(rows_t[id - id_base_t][:]) with t = the last table whose base
 * is <= id and the local id clamped to n_t - 1; an id below 0 reads row 0 of table 0.  count = 1: read_gather_forward, bit for bit;
 * equal activations and no gaps: the plain gather over the concatenated tables, bit for bit.  All levels in one launch; stream-ordered,
 * allocates nothing, no synchronisation.  READ_EINVAL before any device work for: a null table list or level table, count outside
 * 1..READ_GATHER_MAX_TABLES, C % 4 != 0, levels outside 1..READ_MAX_LEVELS, null or misaligned rows, n < 1, an activation outside
 * 0..2, id_base_0 != 0, bases not ascending or ranges overlapping, id_base + n > INT32_MAX, a null level. */
#define READ_GATHER_MAX_TABLES 8
typedef struct read_gather_table {
    const float *rows_nc; int64_t n; int64_t id_base; int activation;
} read_gather_table;
int read_gather_forward_tables(const read_gather_table *tables, int count, int C, int levels,
                               const int32_t *const *idx_levels, const int64_t *count_levels,
                               float *const *feat_levels, void *stream);
/* Its adjoint (csrc/gather.hip, gather_tables_backward_kernel; the definition is tests/joint_texture_model.py): the gradient with respect
 * to the RAW rows, g = dfeat * act_t'(y), y = the forward's output of that pixel (feat_levels, the levels read_gather_forward_tables
 * wrote; may be NULL when every table's activation is 0): act' = 1 (none), y (1 - y) (sigmoid), 1 - y y (tanh).  Same item mapping,
 * table selection and clamps as the forward, so the row addressed is exactly the row the forward read (an id below 0: row 0 of table 0;
 * an id in a gap or past the end: the last row of the last table whose base is <= id).  Two outputs, either or both:
 *   pairs  g_levels[l] is [count_l][C]: g of every pixel, written once — deterministic, no atomics; with the level's ids these are the
 *          (id, gradient row) pairs read_rmsprop_sorted_tables takes.  With activation 0, g == dfeat bit for bit.
 *   dense  drows_tables[t] is table t's [n_t][C] gradient rows, g added by fp32 atomics at the local id; a NULL entry = that table is
 *          frozen: nothing of it is written.
 * All levels in one launch; stream-ordered, allocates nothing, no synchronisation.  READ_EINVAL before any device work for everything
 * read_gather_forward_tables refuses (rows_nc itself is not read and may be NULL), and: feat_levels NULL while some activation is not 0,
 * neither output requested (g_levels NULL and no non-NULL entry of drows_tables), a buffer that is not 16-byte aligned. */
int read_gather_backward_tables(const read_gather_table *tables, int count, int C, int levels,
                                const int32_t *const *idx_levels, const int64_t *count_levels,
                                const float *const *dfeat_levels, const float *const *feat_levels,
                                float *const *g_levels, float *const *drows_tables, void *stream);
/*
 * Scene stitching: several fitted scenes ("parts", 1..READ_STITCH_MAX_PARTS) in one frame.  Every part is rasterised on its own
 * (read_splat_forward*, camera M_s = M_0 @ P_s) into a pyramid of LOCAL ids and depths; this call merges the pyramids and gathers
 * from the winner's table, all levels in one launch.  Per level and pixel:
 *   candidates  every visible part whose pixel is not the empty pattern (idx == 0 and depth bits == 0);
 *   winner      the candidate with the smallest depth bit pattern (depths are >= 0: an unsigned compare, the order of the
 *               rasteriser's 64-bit key); ties go to the lowest part number;
 *   outputs     idx_l[p] = id_base[s] + local id, depth_l[p] = its depth, part_l[p] = s (uint8),
 *               feat_l[p][:] = act_s(rows_s[local id][:]) (NHWC, C % 4 == 0) — bit for bit the values of read_gather_forward;
 *   no candidate  idx 0, depth 0.0f, part 255, feat = act_0(rows_0[0]): the "empty pixels sample descriptor 0" rule applied to the
 *               concatenation of the tables — parts[0] is that table WHETHER OR NOT part 0 is visible.
 * With id_base[s] = sum of n_t over t < s (hidden parts included, so ids stay stable) and identity placements the result equals
 * rasterising the concatenated cloud and gathering from the concatenated table.  One departure: a part's local point 0 at depth
 * bit pattern 0 cannot be told from "empty" and loses.
 * A HIDDEN part is passed with idx_levels == depth_levels == NULL: it keeps its part number and its id range, nothing of it is read
 * except, for part 0, the row the no-candidate pixels sample.  (No pyramid of empties has to be allocated or streamed for it.)
 * Each of the four output tables may be NULL (that output is skipped); without features one lane serves a pixel.  Local ids are
 * clamped to [0, n) as in read_gather_forward.  Stream-ordered, allocates nothing, no synchronisation.  READ_EINVAL before any
 * device work for: count outside 1..READ_STITCH_MAX_PARTS, C % 4 != 0, levels outside 1..READ_MAX_LEVELS, a null part table or
 * count_levels, rows_nc == NULL while features are requested, id_base < 0 or id_base + n > INT32_MAX, all four outputs NULL, a part
 * with only one of its two pyramids, a null level of a visible part or of a requested output.
 */
#define READ_STITCH_MAX_PARTS 8
typedef struct read_stitch_part {
    const int32_t *const *idx_levels;   /* host array of `levels` device pointers: this part's index images; NULL = hidden */
    const float   *const *depth_levels; /* same shape: its depth images */
    const float *rows_nc;               /* device, n x C; may be NULL when feat_levels is NULL */
    int64_t n;
    int32_t id_base;                    /* added to local ids in the merged index image */
    int activation;                     /* 0 none, 1 sigmoid, 2 tanh */
} read_stitch_part;
int read_stitch_gather_forward(const read_stitch_part *parts, int count, int C, int levels,
                               const int64_t *count_levels,
                               int32_t *const *idx_levels, float *const *depth_levels,
                               unsigned char *const *part_levels, float *const *feat_levels, void *stream);
/* drows[idx_l[p]][c] += dfeat_l[p][c]   (fp32 atomics; drows must be zeroed by the caller).  The ids are clamped as in
 * read_gather_forward: the gradient of an id below 0 lands on row 0, that of an id >= n on row n - 1 — the row the forward read.
 * Into zeroed rows, a row addressed once holds that gradient's bits and a row nobody addressed stays +0; a row addressed k times is
 * a sum in an order that changes from run to run, within (k - 1) u sum |dfeat| (u = 2^-24) of the exact sum. */
int read_gather_backward(float *drows_nc, int64_t n, int C, int levels,
                         const int32_t *const *idx_levels, const int64_t *count_levels,
                         const float *const *dfeat_levels, void *stream);

/* Bilinear down-scale by an integer factor ss (2..8) of `planes` NCHW planes [ss*h][ss*w] -> [h][w]: torch's
 * F.interpolate(scale_factor = 1/ss, mode = 'bilinear', align_corners = False) as READ/models/compose.py:162-163 applies it to
 * network inputs that mix non-uv tokens with texture samples (the all-uv case is fused into read_gather_forward_ss), and its
 * adjoint (din is written, not accumulated): exactly dout / 4 on the 2 x 2 footprint of even ss, dout on the centre sample of odd
 * ss, +0 on every other sample.  The forward at odd ss still blends with the weights 1, 0, 0, 0: finite inputs give the centre
 * sample's VALUE, but a -0 comes back as +0 and a non-finite neighbour makes the output NaN — the bit identity of odd ss is a promise
 * of read_gather_forward_ss only. */
int read_bilinear_down(const float *in, int64_t planes, int h, int w, int ss, float *out, void *stream);
int read_bilinear_down_backward(const float *dout, int64_t planes, int h, int w, int ss, float *din, void *stream);

/* ---------------------------------------------------------------- gated conv (BasicConv) */

#define READ_CONV_MAX_SRC 4

typedef struct read_conv_src {
    const float *data;   /* NHWC fp32 [srcH][srcW][C] */
    int C;               /* channels taken from this source (all of them) */
    int srcH, srcW;
    int shift;           /* nearest resample folded into addressing: >0: source is 2^shift finer
                            (src = dst << shift), <0: coarser (src = dst >> -shift), 0: same size */
} read_conv_src;

typedef struct read_conv_desc {
    int n_src;                              /* inputs concatenated along C (torch.cat order) */
    read_conv_src src[READ_CONV_MAX_SRC];
    const float *mul;                       /* optional: input := src[0] * mul (FAM), same shape */
    int inH, inW;                           /* logical input size after resampling */
    int Cout, ksize, stride;                /* ksize in {1,3,4}, stride in {1,2}; pad = (ksize-1)/2 */
    int elu;                                /* 1: ELU on the feature branch (relu=True) */
    const float *wpacked;                   /* read_conv_pack_weights() output (device) */
    const float *params;                    /* 4 x CoutPad: bias_f, bias_m, bn_scale, bn_shift */
    const float *residual;                  /* optional NHWC [outH][outW][Cout], added after BN */
    float *out;                             /* NHWC [outH][outW][out_cstride], first Cout written */
    int out_cstride;                        /* >= Cout */
    float out_fill;                         /* value for channels Cout..out_cstride-1 when fill_pad */
    int fill_pad;
    int config;                             /* tile configuration id, -1 = pick automatically */
    const float *wpacked_wino;              /* optional: read_conv_pack_wino_host() output (device); enables the
                                               Winograd F(2x2,3x3) kernel for 3x3/s1 single-source layers */
    const float *wpacked_w16;               /* optional: read_conv_pack_w16_host() output (device): the same Winograd operand in the
                                               order of the wave-autonomous F(2x2) kernel (all 16 frequencies of a tile in one wave,
                                               v_mfma_f32_16x16x4_f32); taken by non-linear launches with Cout <= 8 (the 32 -> 3
                                               output layer), with read_tuning_set("conv_w16", 1), or with config = -3 */
    const float *wpacked_w4;                /* optional: read_conv_pack_w4_host() output (device): Winograd F(4x4,3x3) operand; taken by
                                               3x3 / stride-1 single-source launches with Cin % 16 == 0, Cin >= read_tuning("conv_w4")
                                               (default 32) and Cout % 32 == 0 (linear launches: Cout % 8 == 0); config = -5
                                               forces it where the shape fits */
    int linear;                             /* 1: plain convolution (training path): out[..][c] = conv_f + b_f,
                                               out[..][Cout + c] = conv_m + b_m, out_cstride >= 2 * Cout; no gate /
                                               BatchNorm / residual; workgroup-tiled or Winograd kernel */
    /* optional pre-activation addend, NHWC [preH][preW][pre_cstride]: before bias / activation / gate,
     *   conv_f(y,x,c) += pre[y >> pre_shift][x >> pre_shift][pre_f_off + c],  conv_m likewise with pre_m_off.
     * A 1x1 convolution commutes with nearest up-sampling, so the share of torch.cat([.., F.interpolate(coarse)]) -> 1x1 conv
     * that comes from a coarser tensor is computed at the coarse resolution by a `linear` launch and enters here
     * (READ/models/unet.py:239-254, the AFF inputs).  Not available with the Winograd kernel. */
    const float *pre;
    int pre_cstride, pre_f_off, pre_m_off, pre_shift, preH, preW;
    /* optional, linear launches that run on the Winograd kernel (3x3 / stride 1, Cin % 16 == 0): ALSO store the layer's output
     * BN_eval(act(f) * sigmoid(m)), NHWC [outH][outW][Cout], in the same pass (what read_gate_forward would compute from
     * `out`); rows r of a stacked batch with r % block_h >= valid_h are written as zeros (block_h = 0: one image). */
    float *out_gated;
    int block_h, valid_h;
    const float *wpacked_sc;                /* optional: read_conv_pack_sc_host() output (device, 64-byte aligned): gated 3x3 / stride-1 launches
                                               with Cin = 32, Cout <= 4 and one unshifted source (READ's output layer 32 -> 3) run on the
                                               vector pipe — thread = pixel, weights streamed through SGPRs — instead of padding six output
                                               rows to an MFMA shape; read_tuning_set("conv_sc", 0) switches it off, config = -6 forces it */
    int pre_bilinear;                       /* 1: the pre-activation addend is sampled BILINEARLY at 4x (pre_shift must be 2): the value
                                               nn.Upsample(scale_factor=4, mode='bilinear', align_corners=False) of `pre` has at (y, x)
                                               (source index 0.25 (dst + 0.5) - 0.5 clamped at 0, neighbours clamped at the edge).  A
                                               1x1 convolution commutes with bilinear up-sampling as it does with nearest, so the share
                                               of cat[Upsample4(coarse), fine] -> 1x1 conv that comes from the coarse tensor is computed at
                                               1/16 of the pixels by a `linear` launch and enters here: no up-sampled tensor is ever
                                               written (READ/models/unet.py:261-262,269-270,277-278, the Convs.k inputs).  1x1 / stride-1
                                               layers on the pixel-lane kernel only (16-byte aligned tensors, Cin <= 256, Cout % 4 == 0) */
    const void *wpacked_w4h;                /* optional: read_conv_pack_w4h_host() output (device): the Winograd F(4x4,3x3) operand split into
                                               two f16 pieces per weight + one power-of-two scale per output row.  Gated (non-linear)
                                               launches of the F(4x4) family with Cin % 32 == 0, Cin >= read_tuning("conv_w4h") (default
                                               32, 0 = never) and Cout % 32 == 0 then run on the f16 matrix cores (v_mfma_f32_16x16x32_f16,
                                               fp32 accumulation, three piece pairs per product: fp32-level results — DESIGN.md 3.3 (a+),
                                               profiles/r6_f16split_probe.txt; transformed inputs must stay below 65504 in magnitude,
                                               i.e. activations below ~650); config = -7 forces it where the shape fits */
    const void *wpacked_d3h;                /* optional: read_conv_pack_d3h_host() output (device): the 3x3 weights themselves as two f16 pieces
                                               per weight + a power-of-two scale per output row.  Gated 3x3 / stride-1 single-source launches
                                               with Cin % 32 == 0, Cin >= read_tuning("conv_d3h") (default 0 = never: plain launches stay on the Winograd split-operand kernels; FAM's x1 * x2 launches take it through read_tuning("conv_d3h_fam"), default 32) and Cout % 32 == 0
                                               (FAM's mul included) then run as a DIRECT convolution on the f16 matrix cores — all nine
                                               taps, three piece pairs per product, fp32 accumulation: no Winograd transform on either
                                               side, fp32-level results (DESIGN.md 3.3 (a++)); inputs must stay below 65504 in magnitude;
                                               config = -8 forces it where the shape fits.  A launch it takes (those thresholds, or config = -8) does not look at
                                               wpacked_w4h / wpacked_w4; every other launch of the family goes to them as if this field were NULL.
                                               For a 1x1 / stride-1 layer the same field takes read_conv_pack_dkh_host(Cin, Cout, 1, ...): launches
                                               (gated or linear, concatenated sources, residual, pre-activation addend) with Cin % 16 == 0,
                                               read_tuning("conv_pxh") (default 16, 0 = never) <= Cin <= 256, Cout % 4 == 0 and 16-byte aligned
                                               tensors then run on the split-operand pixel-lane kernel (v_mfma_f32_32x32x16_f16, three piece
                                               pairs per product, fp32 accumulation); config = -10 forces it where the shape fits */
    const void *wpacked_t3h;                /* optional: read_conv_pack_t3h_host() output (device): the 3x3 weights of a layer with 8, 16 or 32 input
                                               channels as an implicit-GEMM operand (k = tap * Cin + channel, zero-padded to whole steps of 16) in
                                               f16 piece pairs.  3x3 / stride-1 launches (gated or linear, residual) over ONE unshifted source with
                                               C <= read_tuning("conv_t3h") (default 8: the layers that read the 8-channel descriptor pyramid; 0 =
                                               never), Cout % 4 == 0 and 16-byte aligned tensors then run on the split-operand pixel-lane kernel
                                               (zero padding at the image border, as nn.Conv2d); config = -11 forces it where the shape fits */
} read_conv_desc;

/* Sizes (in floats) of the packed weight / parameter blocks of one BasicConv. */
size_t read_conv_packed_floats(int Cin, int Cout, int ksize);
size_t read_conv_param_floats(int Cout);
/* Host-side packing from the PyTorch layout (all host pointers):
 *   wf, wm (Cout,Cin,k,k); bf, bm (Cout); BN gamma, beta, running_mean, running_var (Cout), eps.
 *   kc = input-channel chunk the kernel stages per step: 16 when every concatenated source has
 *   C % 16 == 0, else 8 (the packing order depends on it). */
int read_conv_pack_weights_host(int Cin, int Cout, int ksize, int kc, const float *wf,
                                const float *wm, float *wpacked_host);
/* Winograd F(2x2,3x3): transformed weights G g G^T in fragment order, Cin % 16 == 0 (16/9 the plain size). */
size_t read_conv_wino_floats(int Cin, int Cout);
int read_conv_pack_wino_host(int Cin, int Cout, const float *wf, const float *wm, float *wpacked_wino_host);
/* same size (read_conv_wino_floats), order of the wave-autonomous Winograd kernel: [group][wave][chunk][row][col][lane][4] */
int read_conv_pack_w16_host(int Cin, int Cout, const float *wf, const float *wm, float *wpacked_w16_host);
/* Winograd F(4x4,3x3) operand: read_conv_w4_floats(Cin, Cout) = Cin * 36 * 2 * pad32(Cout) floats,
 * [group][wave][chunk of 16 cin][frequency 36][lane][4] */
size_t read_conv_w4_floats(int Cin, int Cout);
int read_conv_pack_w4_host(int Cin, int Cout, const float *wf, const float *wm, float *wpacked_w4_host);
/* Split-operand F(4x4,3x3) operand (desc.wpacked_w4h): read_conv_w4h_floats(Cin, Cout) = Cin * 36 * 2 * pad32(Cout) + 2 * pad32(Cout)
 * floats (0: Cin % 32 != 0) — [group][wave][chunk of 32 cin][frequency 36][piece hi | lo][lane][8 halfs], then 1 / scale per output row */
size_t read_conv_w4h_floats(int Cin, int Cout);
int read_conv_pack_w4h_host(int Cin, int Cout, const float *wf, const float *wm, void *wpacked_w4h_host);
/* Direct split-operand 3x3 operand (desc.wpacked_d3h): read_conv_d3h_floats(Cin, Cout) = Cin * 18 * pad32(Cout) + 2 * pad32(Cout) floats
 * (0: Cin % 32 != 0) — [group][row half][chunk of 32 cin][tap 9][row block 2][piece hi | lo][lane][8 halfs], then 1 / scale per output row */
size_t read_conv_d3h_floats(int Cin, int Cout);
int read_conv_pack_d3h_host(int Cin, int Cout, const float *wf, const float *wm, void *wpacked_d3h_host);
/* ... for a k x k kernel, k = 3 or 4 ([tap k * k] in the order above; Cin * 2 * k * k * pad32(Cout) + 2 * pad32(Cout) floats): with stride 2, Cin % 32 == 0
 * and Cout % 32 == 0 (the encoder's 3x3 / stride-2 and the decoder's 4x4 / stride-2 layers) desc.wpacked_d3h sends the launch to the stride-2 form
 * of the direct split-operand kernel (read_tuning("conv_d3h_s2"), default 32, 0 = never; config = -9 forces it).
 * ksize = 1 (Cin % 16 == 0): the 1x1 layers' operand for the split-operand pixel-lane kernel, Cin * 2 * pad32(Cout) + 2 * pad32(Cout) floats,
 * [k16 step][tile = 2 group + (f | m)][piece hi | lo][lane][8 halfs] (lane = row (lane & 31) of the tile, cin = 16 step + 8 (lane >> 5) + e), then 1 / scale */
size_t read_conv_dkh_floats(int Cin, int Cout, int ksize);
int read_conv_pack_dkh_host(int Cin, int Cout, int ksize, const float *wf, const float *wm, void *wpacked_host);
/* Implicit-GEMM operand of the 3x3 layers with 8, 16 or 32 input channels (desc.wpacked_t3h): the ksize-1 order above for the matrix
 * W'[cout][tap * Cin + ci] padded to K = pad16(9 * Cin) columns: K * 2 * pad32(Cout) + 2 * pad32(Cout) floats (0: another Cin) */
size_t read_conv_t3h_floats(int Cin, int Cout);
int read_conv_pack_t3h_host(int Cin, int Cout, const float *wf, const float *wm, void *wpacked_t3h_host);
/* Small-Cout order [tap][cin][f0 f1 f2 f3 | m0 m1 m2 m3] (9 * Cin * 8 floats; 0 = the shape has no such order: only Cin = 32,
 * Cout <= 4 has a kernel). */
size_t read_conv_sc_floats(int Cin, int Cout);
int read_conv_pack_sc_host(int Cin, int Cout, const float *wf, const float *wm, float *wpacked_sc_host);
int read_conv_pack_params_host(int Cout, const float *bf, const float *bm, const float *gamma,
                               const float *beta, const float *mean, const float *var, float eps,
                               float *params_host);
int read_gated_conv_forward(const read_conv_desc *desc, void *stream);
/* F(4,3)-by-rows operand of the split-operand 3x3/s1 family (Winograd along x, the three ky taps direct): read_conv_f4x1_floats(Cin, Cout)
 * = Cin * 18 * 2 * pad32(Cout) + 2 * pad32(Cout) floats (half the F(4x4) order), 0 unless Cin % 32 == 0; order
 * [group][wave 4][chunk of 32 cin][ky 3][frequency 6][Uh | Ul][lane][8 halfs], then 2 * pad32(Cout) floats 1 / s.
 * read_gated_conv_forward_f4x1 is read_gated_conv_forward with that operand (device) beside the descriptor, which is frozen at ABI
 * version 3: a family-5 launch with Cin >= read_tuning("conv_f4x1") (default 32; 0 = never), or config = -12 / -13 / -14, runs on the
 * F(4,3)-by-rows kernel; every other launch is unchanged.  The kernel has three forms with the same results, bit for bit: one workgroup
 * per CU (config = -12), two resident workgroups per CU (config = -13, accepted and refused exactly where -12 is) and one eight-wave
 * workgroup per CU that shares the input transform between two channel groups (config = -14, accepted where -12 is and
 * Cout % 64 == 0, refused by name otherwise); the automatic choice takes the form that measured faster for the launch's shape
 * (profiles/f4x1_pair_ab.md, profiles/f4x1_wide_ab.md).  desc.wpacked_w4h may stay NULL when only this order was packed: a launch
 * that would then need the F(4x4) order is refused with READ_EINVAL.  The input transform amplifies by at most 10 (F(4x4): 100), so
 * the f16 pieces cover activations up to about 6500. */
size_t read_conv_f4x1_floats(int Cin, int Cout);
int read_conv_pack_f4x1_host(int Cin, int Cout, const float *wf, const float *wm, void *wpacked_f4x1_host);
int read_gated_conv_forward_f4x1(const read_conv_desc *desc, const void *wpacked_f4x1, void *stream);
/* Resident workgroups per CU that the runtime grants the two-workgroup form (2 by design); -1: the query failed. */
int read_conv_f4x1_pair_occupancy(void);
/* The inverse of read_conv_pack_weights_host: (Cout, Cin, k, k) weights, exact, out of the direct fragment order. */
int read_conv_unpack_weights_host(int Cin, int Cout, int ksize, int kc, const float *wpacked_host, float *wf, float *wm);
/* Which kernel family read_gated_conv_forward takes for this (filled) descriptor under the current tuning knobs: 8 = the same kernel as an
 * implicit GEMM over a 3x3 layer with 8 - 32 input channels (reads wpacked_t3h), 7 = 1x1 pixel-lane kernel
 * with split operands on the f16 matrix cores (reads wpacked_d3h of a 1x1 layer), 6 = direct 3x3 with
 * split operands on the f16 matrix cores (reads wpacked_d3h), 5 = the split-operand Winograd family for 3x3 / stride 1 on the f16
 * matrix cores: F(4x4,3x3) (reads wpacked_w4h) or, through read_gated_conv_forward_f4x1, F(4,3) by rows (reads wpacked_f4x1), 4 = Winograd F(4x4,3x3) on the fp32 matrix cores
 * (reads wpacked_w4), 2 = Winograd F(2x2,3x3) (reads wpacked_wino), 1 = vector-pipe small-Cout kernel (reads
 * wpacked_sc), 0 = direct implicit GEMM (reads wpacked); -1 = NULL.  A host that packs ONE fragment order per layer asks this before packing (set the pointer it intends to fill to any
 * non-NULL value); a launch whose wpacked aliases Winograd fragments it would not read is refused with READ_EINVAL. */
int read_conv_kernel_family(const read_conv_desc *desc);
/* Number of compiled tile configurations and a printable name for each (for tuning sweeps). */
int read_conv_config_count(void);
const char *read_conv_config_name(int config);

/* out[y][x][c] = bilinear x4 (align_corners=False) of in, NHWC, C % 4 == 0. */
int read_bilinear_up4(const float *in, int inH, int inW, int C, float *out, void *stream);

/* ---------------------------------------------------------------- training step (csrc/train.hip)
 * Backward of one BasicConv, y = BN_eval(act(f) * sigmoid(m)) with [f | m] = conv_{f|m}(x) + b (READ/models/unet.py:44-53 under
 * torch.autograd in src/train.py:132-203); BatchNorm as the eval-mode affine map (configs/train_example.yaml eval_in_train).
 *   forward (training)  a READ_PACK_PARAMS and a mode-0 fragment job (read_pack_job below), read_gated_conv_forward with
 *                       desc.linear = 1 -> pre-activations [pixels][2*Cout], read_gate_forward -> y
 *   backward            read_gate_backward: dy, [f|m] -> dfm [pixels][2*Cp] (Cp = Cout rounded up to 8; df | dm) and the
 *                       per-channel sums S[4][Cout] += {sum df, sum dm, sum dy, sum dy*g} (ACCUMULATED: the caller zero-fills S —
 *                       one fill for all layers of a step; read_gate_backward_bn clears its own); read_bn_param_grads turns them
 *                       into db_f, db_m, dgamma, dbeta (accumulating);
 *                       dgrad: stride 1 -> a mode-1 fragment job + read_gated_conv_forward(linear = 1) over dfm with
 *                       Cout := Cin/2, zero biases (the same MFMA kernel with flipped, transposed weights);
 *                       stride 2 -> read_conv_dgrad_generic;
 *                       read_conv_wgrad: x, dfm -> dW_f, dW_m in the PyTorch layout (Cout, Cin, k, k), MFMA, split over
 *                       pixel rows with a scratch of read_conv_wgrad_scratch_floats().  3x3 / stride-1 layers with Cin % 32 == 0 on
 *                       images of whole 4 x 4 tiles are summed in the Winograd F(4x4,3x3) domain (dg = G^T [sum over tiles of
 *                       (B^T d B) . (A dY A^T)] G: a quarter of the multiplications; read_tuning_set("wgrad_wino", 0): direct
 *                       kernel); read_conv_wgrad_family says which: 4 or 0. */
/* Packing on the device.  The optimizer changes every weight every step, so a step re-packs the parameter block, the forward
 * fragments and the dgrad fragments of every layer (294 jobs for READ's UNet).  ONE job type describes them all:
 *   kind READ_PACK_PARAMS: out[4 * pad32(Cout)] = bias_f, bias_m, bn scale, bn shift   (read_conv_pack_params_host's block)
 *        READ_PACK_DIRECT: the direct fragment order of read_conv_pack_weights_host (ksize 1 / 3 / 4, chunk kc)
 *        READ_PACK_WINO / READ_PACK_W4: the Winograd F(2x2,3x3) / F(4x4,3x3) orders of read_conv_pack_wino_host / _w4_host
 *        (3x3 / stride 1, Cin % 16 == 0; desc.wpacked_wino / desc.wpacked_w4: linear-mode launches of eligible layers then take
 *        those kernels, the F(4x4) one where Cin >= 32 and Cout % 8 == 0, storing the pre-activations and — with desc.out_gated —
 *        the gated output in the same pass)
 *   mode 0: the layer's own weights; mode 1: its dgrad as a convolution over d[f|m] — the virtual layer with 2 * pad8(Cout)
 *        input and Cin / 2 gated output channels, weights flipped and transposed (Cin even; sizes: read_conv_dgrad_*_floats).
 * read_conv_pack_job_prepare (host) is the one place that validates a job (READ_EINVAL and a message otherwise) and fills
 * Cp / total / nblocks.  Two ways to run jobs:
 *   read_conv_pack_job(job_host, stream): prepare, then ONE launch with the job passed by value (a direct-order job on its own is
 *        spread over more workgroups than the nblocks it takes in a table; the packer is grid-strided, the output the same);
 *   read_conv_pack_batch: every job of a step in ONE launch.  A host that knows its layers builds the table ONCE (the tensors keep
 *        their addresses across optimizer steps): prepare each job, set first_block to the running sum of nblocks, upload the table
 *        and pass the grand total as total_blocks, once per step.
 * The read_conv_pack_*_device entry points are read_conv_pack_job with the job filled from their arguments. */
enum { READ_PACK_PARAMS = 0, READ_PACK_DIRECT = 1, READ_PACK_WINO = 2, READ_PACK_W4 = 3 };
typedef struct read_pack_job {
    int kind, mode;                         /* mode: 0 the layer's own weights, 1 its dgrad */
    int Cin, Cout, ksize, kc;               /* kc: channel chunk of the direct order (8 / 16; 32 for a 1x1 layer's own weights) */
    int Cp, first_block, nblocks;           /* derived (prepare) / prefix sum (caller, read_conv_pack_batch only) */
    float eps;                              /* params job: BatchNorm epsilon */
    const float *wf, *wm;                   /* (Cout, Cin, k, k) conv_f / conv_m weights */
    const float *bf, *bm, *gamma, *beta, *mean, *var;   /* params job (bf / bm may be NULL) */
    float *out;
    long long total;                        /* floats written (derived) */
} read_pack_job;
int read_conv_pack_job_prepare(read_pack_job *job);
int read_conv_pack_job(read_pack_job *job_host, void *stream);
int read_conv_pack_batch(const read_pack_job *jobs_dev, int njobs, int total_blocks, void *stream);
int read_conv_pack_params_device(int Cout, const float *bf, const float *bm, const float *gamma, const float *beta,
                                 const float *mean, const float *var, float eps, float *params, void *stream);
int read_conv_pack_weights_device(int Cin, int Cout, int ksize, int kc, const float *wf, const float *wm, float *wpacked,
                                  void *stream);
int read_conv_pack_wino_device(int Cin, int Cout, const float *wf, const float *wm, float *wpacked_wino, void *stream);
int read_conv_pack_w4_device(int Cin, int Cout, const float *wf, const float *wm, float *wpacked_w4, void *stream);
size_t read_conv_dgrad_packed_floats(int Cin, int Cout, int ksize);
size_t read_conv_dgrad_wino_floats(int Cin, int Cout);
size_t read_conv_dgrad_w4_floats(int Cin, int Cout);
int read_conv_pack_dgrad_device(int Cin, int Cout, int ksize, int kc, const float *wf, const float *wm, float *wpacked,
                                void *stream);
int read_conv_pack_dgrad_wino_device(int Cin, int Cout, const float *wf, const float *wm, float *wpacked_wino, void *stream);
int read_conv_pack_dgrad_w4_device(int Cin, int Cout, const float *wf, const float *wm, float *wpacked_w4, void *stream);
/* A training batch is ONE tall image: the items stacked vertically, block_h rows per item of which the first valid_h are
 * the item and the rest a separator that stays zero in every activation — it is the zero padding between neighbours, so the
 * convolutions need no batch dimension and one launch covers the batch.  The gate kernels keep the separators zero (forward)
 * and give them zero gradient (backward); W = row length in pixels; block_h = 0 means a single image. */
int read_gate_forward(const float *fm, int64_t pixels, int Cout, const float *params, int elu, const float *residual,
                      float *y, int W, int block_h, int valid_h, void *stream);
int read_gate_backward(const float *dy, const float *fm, int64_t pixels, int Cout, const float *params, int elu, float *dfm,
                       float *sums, int W, int block_h, int valid_h, void *stream);
int read_bn_param_grads(int Cout, const float *sums, const float *mean, const float *var, float eps, float *dbf, float *dbm,
                        float *dgamma, float *dbeta, void *stream);
/* Batch-statistics BatchNorm — nn.BatchNorm2d in .train() (READ/models/unet.py:40,51; the reference's default training mode,
 * train.py:271-279,450).  read_bn_train_forward: g = act(f) * sigmoid(m) [pixels][C] (produced with an identity BatchNorm in the
 * params block: scale 1, shift 0) is normalised IN PLACE with the per-channel mean / biased variance of the valid pixels
 * (fp64 accumulation): y = (g - mean) / sqrt(var + eps) * gamma + beta; separator rows of a stacked batch stay zero and do
 * not count.
 * `groups` = number of statistic groups: 1 — the whole stacked batch is ONE BatchNorm batch (what nn.BatchNorm2d does with a
 * (B,C,h,w) tensor: UNet.forward on a batch); B = the number of stacked items — every item is normalised with ITS OWN statistics
 * and the running buffers move B times, in item order: the reference's NetAndTexture.forward calls the net once per batch item
 * (READ/models/compose.py:137-176), so its BatchNorm layers see N = 1.  stat[groups][2][C] receives {mean, biased var} per group
 * (kept for the backward pass), scale_shift (groups * 2 * pad32(C) floats) the scale / shift rows, running_mean / running_var
 * (may be NULL) move by `momentum` once per group (variance unbiased, n / (n - 1)), scratch = groups * 2 * C doubles.
 * read_gate_backward_bn: read_gate_backward through that BatchNorm: two passes (sums of dy and dy * g, then
 * dg = gamma r (dy - mean(dy) - xhat mean(dy xhat))) per group; sums[groups][4][Cout] as read_gate_backward per group, so
 * read_bn_param_grads_groups(Cout, groups, sums, stat, ...) gives db_f, db_m, dgamma, dbeta (accumulating, summed over the
 * groups); abc = groups * 3 * Cout floats of scratch.
 * Numerical range of read_gate_backward(_bn) / read_bn_param_grads(_groups) (profiles/train_accuracy_fp64.md): sums row 3 is sum dy * g, NOT centred, so dgamma = (S3 - mean S2) r and
 * dg = A dy + B + C g cancel when a channel's |mean| is large against its standard deviation: the cost is about half of |mean| / std in units of
 * u r sum |dy| |g - mean| in dgamma and a quarter of it in units of dg's condition term (u = 2^-24; measured up to 118 and 66 at
 * |mean| / std = 2^8, 1536 pixels); read_bn_train_forward's y = g scale + (beta - mean scale) carries an absolute error of about u |mean| scale. */
int read_bn_train_forward(float *g_to_y, int64_t pixels, int C, int W, int block_h, int valid_h, int groups, const float *gamma,
                          const float *beta, float eps, float momentum, float *running_mean, float *running_var, float *stat,
                          float *scale_shift, double *scratch, void *stream);
int read_gate_backward_bn(const float *dy, const float *fm, int64_t pixels, int Cout, const float *params, int elu, float *dfm,
                          float *sums, int W, int block_h, int valid_h, int groups, const float *stat, const float *gamma,
                          float eps, float *abc, void *stream);
int read_bn_param_grads_groups(int Cout, int groups, const float *sums, const float *stat, float eps, float *dbf, float *dbm,
                               float *dgamma, float *dbeta, void *stream);
size_t read_conv_dgrad_generic_floats(int Cin, int Cout, int ksize);
int read_conv_dgrad_generic(const float *dfm, int outH, int outW, int Cin, int Cout, int ksize, int stride, const float *wf,
                            const float *wm, float *wscratch, int inH, int inW, float *dx, void *stream);
size_t read_conv_wgrad_scratch_floats(int Cin, int Cout, int ksize, int outH);
int read_conv_wgrad(const float *x, int inH, int inW, int Cin, const float *dfm, int Cout, int ksize, int stride, float *dwf,
                    float *dwm, int accumulate, float *scratch, size_t scratch_floats, void *stream);
int read_conv_wgrad_family(int Cin, int ksize, int stride, int inH, int inW);
/* read_bilinear_up4 for a vertically stacked batch (rows interpolate inside an item only) and the adjoint of both:
 * dout [4*inH][4*inW][C] -> din [inH][inW][C] */
int read_bilinear_up4_blocks(const float *in, int inH, int inW, int C, float *out, int block_h, int valid_h, void *stream);
int read_bilinear_up4_backward(const float *dout, int inH, int inW, int C, float *din, int block_h, int valid_h, void *stream);
/* F.huber_loss(out, target) (delta 1, mean; src/READ/models/compose.py:35,38): *loss_sum = sum of the per-element losses
 * (divide by n), grad[i] = grad_scale * clip(out - target, -1, 1).  Either output may be NULL. */
int read_huber_loss(const float *out, const float *target, int64_t n, float grad_scale, float *loss_sum, float *grad,
                    void *stream);
/* RMSprop (READ/pipelines/ogl.py:16,99-100 defaults: alpha 0.99, eps 1e-8) over the descriptor ROWS the step touched only:
 * ids = the step's int32 index maps; every touched row is updated once, its gradient row is zeroed again, and the decay
 * of the steps in which it was not touched (gradient 0 in the dense optimizer) is applied lazily from `stamp`
 * (int32 per row, zero-initialised; step counts from 1).  rows / sq / grad are N x C. */
int read_rmsprop_sparse(float *rows, float *sq, float *grad, int32_t *stamp, int C, int64_t n_rows, const int32_t *ids,
                        int64_t n_ids, int step, float lr, float alpha, float eps, void *stream);
/* The same update without the N x C gradient table: the step's (id, gradient row) pairs sorted by id (sorted_ids ascending,
 * perm[i] = row of g that sorted_ids[i] came from, e.g. torch.sort); runs of equal ids are summed in sorted order
 * (deterministic) and applied once.  scratch: read_rmsprop_sorted_scratch_ints() int32 of device memory. */
size_t read_rmsprop_sorted_scratch_ints(void);
int read_rmsprop_sorted(float *rows, float *sq, int32_t *stamp, int C, int64_t n_rows, const int32_t *sorted_ids,
                        const int64_t *perm, const float *g, int64_t n, int step, float lr, float alpha, float eps,
                        int32_t *scratch, void *stream);
/* The sorted update over a TABLE LIST (read_gather_table's id ranges: table t of count, 1..READ_GATHER_MAX_TABLES, owns the merged ids
 * [id_base_t, id_base_t + n_t); id_base_0 = 0, bases ascend, ranges do not overlap, gaps may remain): sorted_ids are merged ids.  One
 * pass over the sorted pairs; the head of every run finds its table (the last whose base is <= id), sums the run in sorted order and
 * updates (rows_t, sq_t, stamp_t) at the local id with THAT table's step.  With contiguous ranges and equal steps this is
 * read_rmsprop_sorted on the concatenated table; count = 1: read_rmsprop_sorted itself, bit for bit.
 * A run whose id is below 0, in a gap, past the last range, or in a table with trainable == 0 is SKIPPED: no state is touched.  This
 * deliberately differs from the gather's clamp (read_gather_forward_tables reads the nearest row for such an id): as in
 * read_rmsprop_sorted an out-of-range id is a caller's error that the id range check reports, not a row to train.
 * scratch: read_rmsprop_sorted_scratch_ints() int32, as read_rmsprop_sorted's.  A table with trainable == 0 may leave rows / sq / stamp
 * NULL and step 0.  READ_EINVAL before any device work for: a null table list, sorted_ids, perm, g or scratch, count outside
 * 1..READ_GATHER_MAX_TABLES, C outside 1..16, n < 0, a table with n < 1, bases that break the rule above or leave the int32 range, a
 * trainable table with a null pointer or step < 1. */
typedef struct read_rmsprop_table {
    float *rows; float *sq; int32_t *stamp; int64_t n; int64_t id_base; int step; int trainable;
} read_rmsprop_table;
int read_rmsprop_sorted_tables(const read_rmsprop_table *tables, int count, int C, const int32_t *sorted_ids, const int64_t *perm,
                               const float *g, int64_t n, float lr, float alpha, float eps, int32_t *scratch, void *stream);

/* ---------------------------------------------------------------- UNet */

typedef struct read_unet read_unet_t;

/* The 101 BasicConvs of READ's UNet in canonical order (99 execute; ConvsOut.* are packed but
 * never run, unet.py:181-186).  For layer i: state-dict path prefix, Cin, Cout, ksize. */
int read_unet_layer_count(void);
int read_unet_layer_info(int i, const char **path, int *cin, int *cout, int *ksize, int *stride,
                         int *elu);
/* Total floats of the raw parameter blob: per layer, in order,
 *   conv_f.weight, conv_f.bias, conv_m.weight, conv_m.bias, norm.weight, norm.bias,
 *   norm.running_mean, norm.running_var. */
size_t read_unet_raw_floats(void);
size_t read_unet_packed_floats(void);
int read_unet_pack_host(const float *raw_host, float bn_eps, float *packed_host);
/* Layout of the packed blob.  FULL (the two functions above): every fragment order of every layer — direct, both F(2x2) orders,
 * F(4x4) where it exists —, so any tuning knob can send a layer to any of its kernels: 952 MB for READ's 121 MB of weights.
 * LEAN: what the default plan reads — a layer the F(4x4) kernel runs (73 of the 105 launches) carries its F(4x4) order only,
 * layers that no launch executes (ConvsOut) carry nothing: 451 MB.  read_unet_create_layout refuses a lean blob (READ_EINVAL)
 * when, under the current tuning state or at a size whose tensors reach 2 GiB, one of those layers would not run on the F(4x4)
 * kernel.  The raw blob is the same for both layouts. */
/* The F(4,3)-by-rows order (read_conv_pack_f4x1_host) of the 70 split-operand 3x3/s1 layers, which the default plan runs on that kernel:
 * LEAN carries it behind each such layer's F(4x4) split operand.  FULL is laid out exactly as before and does not carry it; it carries
 * every layer's exact weights, so the host derives the order once per blob and hands it to the plan as a side buffer — see
 * read_unet_set_f4x1 below.  LEAN_W4H is the lean layout without that order: blobs packed before the kernel existed; they, and a FULL
 * plan without a side buffer, run those layers on the F(4x4) split-operand kernel. */
enum { READ_UNET_LAYOUT_FULL = 0, READ_UNET_LAYOUT_LEAN = 1, READ_UNET_LAYOUT_LEAN_W4H = 2 };
size_t read_unet_packed_floats_layout(int layout);
int read_unet_pack_host_layout(const float *raw_host, float bn_eps, float *packed_host, int layout);
size_t read_unet_workspace_bytes(int H, int W);
/* H, W multiples of 16 (READ/gl/nn.py:107-109).  `packed` and `ws` are device memory that must
 * outlive the handle. */
int read_unet_create(read_unet_t **out, const float *packed, int H, int W, void *ws, size_t ws_bytes);
int read_unet_create_layout(read_unet_t **out, const float *packed, int H, int W, void *ws, size_t ws_bytes, int layout);
void read_unet_destroy(read_unet_t *u);
/* FULL-layout plans: for j = 0, 1, ... while read_unet_f4x1_layer(j, ...) returns 0, the layer's weights are
 * read_conv_unpack_weights_host(cin, cout, 3, 16, full_blob + w_off, wf, wm) and its order goes to side + side_off
 * (read_conv_pack_f4x1_host); read_unet_f4x1_floats() floats in all.  read_unet_set_f4x1 gives the device copy (16-byte aligned, must
 * outlive the handle; NULL takes it away) to a plan created from a FULL blob. */
size_t read_unet_f4x1_floats(void);
int read_unet_f4x1_layer(int j, size_t *w_off, size_t *side_off, int *cin, int *cout);
int read_unet_set_f4x1(read_unet_t *u, const float *side_dev);
/* x0..x3: NHWC [H>>l][W>>l][8] feature pyramids; rgb: NHWC [H][W][rgb_cstride], channels 0..2
 * written (channel 3 set to 1.0f when rgb_cstride == 4, the viewer's RGBA frame, nn.py:123-124). */
int read_unet_forward(read_unet_t *u, const float *x0, const float *x1, const float *x2,
                      const float *x3, float *rgb, int rgb_cstride, void *stream);
/* Per-layer timing of the last instrumented forward: runs one forward with hipEvents around
 * every launch and fills ms[0..n) (n = read_unet_launch_count()).  Synchronises. */
int read_unet_launch_count(read_unet_t *u);
const char *read_unet_launch_label(read_unet_t *u, int i);
/* Static facts about launch i of the plan: algorithmic FLOPs (2*MAC, both gate convs), whether it
 * is one of the dominant 3x3/s1 C->C gated convs, output size and channel counts. */
int read_unet_launch_info(read_unet_t *u, int i, double *flops, int *is_conv3x3_s1, int *outH,
                          int *outW, int *cin, int *cout);
int read_unet_profile(read_unet_t *u, const float *x0, const float *x1, const float *x2,
                      const float *x3, float *rgb, int rgb_cstride, void *stream, float *ms,
                      double *flops, int *is_conv3x3_s1);
/* Device pointer of an intermediate activation by name ("res1", "z8", ...), for layer-level tests. */
const float *read_unet_debug_tensor(read_unet_t *u, const char *name, int *H, int *W, int *C);

#ifdef __cplusplus
}
#endif
#endif /* READ_HIP_H */
