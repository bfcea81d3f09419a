"""Object selection, defined once in NumPy: per-point labels from oriented 3-D boxes and from 2-D label images
lifted over posed views.  read_amd/csrc/select.hip and read_amd/select.py are held to it bit for bit
(tests/test_select_cpu.py: model against a per-point loop; tests/test_gpu_select.py: kernels against the model).

All arithmetic is fp32, sums left to right, nothing fused (NumPy never fuses); a comparison with a NaN is false.

Boxes.  A box is 12 floats, a row-major 3x4 matrix A taking cloud coordinates to the unit cube.  Point (x, y, z) is inside iff
|t_r| <= 1 for r = 0, 1, 2 with t_r = A[4r] x + A[4r+1] y + A[4r+2] z + A[4r+3] 1 (the expression shape of project_one); faces
are inclusive, a non-finite point is outside.  labels_out[i] = label_of[k] of the smallest k whose box contains point i, else
labels_in[i] (0 without labels_in).

Views.  One uint32 state word per point, cand << 16 | hit << 8 | seen, zero at the start; views are applied in order, at most 255.
near[p] = +inf where pixel p of the level-0 frame is empty (idx0 = 0 and the bits of depth0 = 0), else c3 of point idx0[p], c3 =
M[12] x + M[13] y + M[14] z + M[15] 1 (the clip w of project_one: for get_proj_matrix projections the metric distance along the
camera axis).  Point i under a view: pix = project_one; pix < 0: nothing; lim = near[pix] scale + slack; not c3 <= lim: occluded,
nothing; else seen += 1 and with m = mask[pix]: m != 0 and cand == 0 -> cand = m, hit = 1; m != 0 and m == cand -> hit += 1; any
other m counts as seen only.  The candidate is the label of the FIRST view that names one — not a majority over labels.
Finish: labels_out[i] = cand iff cand != 0, hit >= min_hits and hit den >= num seen; else labels_in[i] (0 without).
"""
import numpy as np

from tests import pano_model as pm

f32 = np.float32
MAX_LABEL = (1 << 16) - 1
MAX_BOXES = 1024
MAX_VIEWS = 255


# ---- A. boxes ---------------------------------------------------------------------------------------------------------------------
def inside_box(xyz, A):
    """bool (N,): which points lie in the box A (12 floats)."""
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    A = np.asarray(A, f32).reshape(12)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    ok = np.ones(xyz.shape[0], bool)
    with np.errstate(all='ignore'):
        for r in range(3):
            t = A[4 * r] * x + A[4 * r + 1] * y + A[4 * r + 2] * z + A[4 * r + 3] * f32(1)
            ok &= np.abs(t) <= f32(1)
    return ok


def label_boxes(xyz, boxes, label_of=None, labels_in=None):
    """-> int32 (N,)."""
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    boxes = np.asarray(boxes, f32).reshape(-1, 12)
    K = boxes.shape[0]
    label_of = np.arange(1, K + 1, dtype=np.int32) if label_of is None else np.asarray(label_of, np.int32)
    out = np.zeros(xyz.shape[0], np.int32) if labels_in is None else np.array(labels_in, np.int32)
    for k in range(K - 1, -1, -1):                   # last to first: the smallest k is written last
        out[inside_box(xyz, boxes[k])] = label_of[k]
    return out


# ---- B. views ---------------------------------------------------------------------------------------------------------------------
def c3(xyz, M):
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    M = np.asarray(M, f32).reshape(16)
    with np.errstate(all='ignore'):
        return (M[12] * xyz[:, 0] + M[13] * xyz[:, 1] + M[14] * xyz[:, 2] + M[15] * f32(1)).astype(f32)


def project(xyz, M, W, H):
    """project_one for every point -> pixel or -1 (int32)."""
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    M = np.asarray(M, f32).reshape(16)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(all='ignore'):
        c = [M[4 * r] * x + M[4 * r + 1] * y + M[4 * r + 2] * z + M[4 * r + 3] * f32(1) for r in range(4)]
        nx, ny, nz = c[0] / c[3], c[1] / c[3], c[2] / c[3]
    return pm.tail(nx, ny, nz, W, H)[0]


def near_image(xyz, M, idx0, depth0):
    """-> fp32 (H*W,)."""
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    idx0 = np.asarray(idx0, np.int32).reshape(-1)
    bits = np.ascontiguousarray(depth0, f32).reshape(-1).view(np.uint32)
    empty = (idx0 == 0) & (bits == 0)
    empty |= (idx0 < 0) | (idx0 >= xyz.shape[0])          # no id of this cloud: the kernel reads nothing and treats it as empty
    w = c3(xyz, M)
    return np.where(empty, f32(np.inf), w[np.where(empty, 0, idx0)]).astype(f32)


def classify(xyz, M, W, H, near, scale, slack):
    """-> (pix int32 (N,), visible bool (N,)): the pixel of every point and whether the view sees it (in view and not occluded)."""
    pix = project(xyz, M, W, H)
    w = c3(xyz, M)
    with np.errstate(all='ignore'):
        lim = np.asarray(near, f32)[np.maximum(pix, 0)] * f32(scale) + f32(slack)
        vis = (pix >= 0) & (w <= lim)
    return pix, vis


def vote(state, xyz, M, W, H, near, mask, scale, slack):
    """One view: -> the new state (uint32 (N,)); ``state`` is left unchanged."""
    state = np.asarray(state, np.uint32)
    pix, vis = classify(xyz, M, W, H, near, scale, slack)
    m = np.asarray(mask, np.int32).reshape(-1)[np.maximum(pix, 0)].astype(np.uint32)
    cand, hit, seen = state >> np.uint32(16), (state >> np.uint32(8)) & np.uint32(0xff), state & np.uint32(0xff)
    first = vis & (m != 0) & (cand == 0)
    again = vis & (m != 0) & (cand != 0) & (m == cand)
    seen = seen + vis.astype(np.uint32)
    hit = np.where(first, np.uint32(1), hit + again.astype(np.uint32))
    cand = np.where(first, m, cand)
    return (cand << np.uint32(16) | hit << np.uint32(8) | seen).astype(np.uint32)


def finish(state, min_hits=1, ratio=(1, 2), labels_in=None):
    """-> int32 (N,)."""
    state = np.asarray(state, np.uint32)
    num, den = int(ratio[0]), int(ratio[1])
    cand, hit, seen = (state >> np.uint32(16)).astype(np.int64), ((state >> np.uint32(8)) & np.uint32(0xff)).astype(np.int64), \
        (state & np.uint32(0xff)).astype(np.int64)
    keep = (cand != 0) & (hit >= int(min_hits)) & (hit * den >= num * seen)
    base = np.zeros(state.shape[0], np.int32) if labels_in is None else np.asarray(labels_in, np.int32)
    return np.where(keep, cand.astype(np.int32), base).astype(np.int32)


def scale_of(rel):
    return f32(1.0 + rel)
