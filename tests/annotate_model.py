"""Frame annotations: the NumPy model of the contract (include/read_hip.h, read_annotate_frame).  Kernels
(read_amd/csrc/annotate.hip) and Python (read_amd/annotate.py) are held to it bit for bit.

Inputs: the scene cloud xyz (N,3) and labels (N, or None = all static), the foreign objects and the instance list of
tests/instances_model.py — here as [(k, P, visible)], object k = ranges[k - 1] of ``instances_model.layout`` — the camera M0, W, H
and the frame's level-0 idx / depth images as read_splat_forward_instances wrote them.

Per pixel p: empty (idx == 0 and depth bits == 0) -> obj = inst = -1.  Otherwise id = idx[p]; id < N: object k = labels[id], point
xyz[id]; id >= N: the foreign object whose [id_base, id_base + m) holds it, numbered after the own labels, point xyz_f[id - id_base];
an id no range holds: obj = inst = -1, unmatched += 1.  k == 0: obj = 0, inst = -1.  k >= 1: obj = k, inst = values[i] of the FIRST
instance i in list order that is visible and non-empty, draws object k, and under M_i = object_matrix(M0, P_i) projects the point to
pixel p with depth bits equal to depth[p]'s; none: inst = -1, unmatched += 1.

Per instance i, twelve int32: vis_px, vx0, vy0, vx1, vy1 (the pixels instance i won and their inclusive box), in_pts, ax0, ay0, ax1,
ay1 (its points that project inside the image and the inclusive box of their pixels), near_bits (their smallest depth bit pattern),
n_pts.  An empty minimum is INT32_MAX, an empty maximum -1; a hidden instance keeps n_pts and is otherwise empty."""
import numpy as np

import oracle
from read_amd.raster import object_matrix
from tests import instances_model as im

INT32_MAX = np.int32(0x7FFFFFFF)
STATS = 12
VIS_PX, VX0, VY0, VX1, VY1, IN_PTS, AX0, AY0, AX1, AY1, NEAR_BITS, N_PTS = range(STATS)


def empty_row(n_pts=0):
    return np.array([0, INT32_MAX, INT32_MAX, -1, -1, 0, INT32_MAX, INT32_MAX, -1, -1, INT32_MAX, n_pts], np.int32)


def _bits(depth):
    return np.ascontiguousarray(depth, np.float32).view(np.uint32)


def instance_ranges(xyz, labels, foreign, inst):
    """[(k, P, visible)] -> the list in instances_model's form [(first, npts, P, visible)], with the layout it indexes."""
    static, pool, ranges = im.layout(xyz, labels, foreign)
    return static, pool, ranges, [(ranges[k - 1][0], ranges[k - 1][1], P, v) for k, P, v in inst]


def annotate(xyz, labels, foreign, inst, M0, W, H, idx, depth, values=None):
    """-> (obj (H,W) int32, inst (H,W) int32, stats (I,12) int32, unmatched int, won (H,W) int32 = the list POSITION behind inst)."""
    xyz = np.asarray(xyz, np.float32)
    N = xyz.shape[0]
    lab = np.zeros(N, np.int64) if labels is None else np.asarray(labels).astype(np.int64)
    K_own = int(lab.max()) if lab.size else 0
    _, pool, ranges, lst = instance_ranges(xyz, labels, foreign, inst)
    I = len(lst)
    values = np.arange(I, dtype=np.int32) if values is None else np.asarray(values, np.int32)
    idx = np.asarray(idx, np.int32).reshape(-1)
    dbits = _bits(depth).reshape(-1)
    P_ = W * H
    assert idx.size == P_ and dbits.size == P_
    obj = np.full(P_, -1, np.int32)
    won = np.full(P_, -1, np.int32)
    filled = ~((idx == 0) & (dbits == 0))
    # id -> (object, point)
    k_of = np.full(P_, -1, np.int64)
    pt = np.zeros((P_, 3), np.float32)
    own = filled & (idx >= 0) & (idx < N)
    k_of[own] = lab[idx[own]]
    pt[own] = xyz[idx[own]]
    base = N
    for f, fx in enumerate(foreign):
        fx = np.asarray(fx, np.float32)
        sel = filled & (idx >= base) & (idx < base + fx.shape[0])
        k_of[sel] = K_own + 1 + f
        pt[sel] = fx[idx[sel] - base]
        base += fx.shape[0]
    obj[filled & (k_of >= 0)] = k_of[filled & (k_of >= 0)]
    # the instance walk: list order, the first match stays
    M = [object_matrix(M0, P) for _, P, _ in inst]
    for i in range(I - 1, -1, -1):
        k, _, visible = inst[i]
        if not visible or lst[i][1] == 0:
            continue
        cand = np.flatnonzero(filled & (k_of == k))
        if cand.size == 0:
            continue
        pix, d = oracle.project_points(pt[cand], M[i], W, H)
        hit = (pix == cand) & (_bits(d) == dbits[cand])
        won[cand[hit]] = i
    unmatched = int((filled & ((k_of < 0) | ((k_of >= 1) & (won < 0)))).sum())
    stats = np.stack([empty_row(lst[i][1]) for i in range(I)]) if I else np.zeros((0, STATS), np.int32)
    ys, xs = np.divmod(np.arange(P_), W)
    for i in range(I):
        sel = won == i
        if sel.any():
            stats[i, VIS_PX:VY1 + 1] = (sel.sum(), xs[sel].min(), ys[sel].min(), xs[sel].max(), ys[sel].max())
        first, npts, _, visible = lst[i]
        if not visible or npts == 0:
            continue
        pix, d = oracle.project_points(pool[0][first:first + npts], M[i], W, H)
        ok = pix >= 0
        if ok.any():
            px, py = pix[ok] % W, pix[ok] // W
            stats[i, IN_PTS:NEAR_BITS + 1] = (ok.sum(), px.min(), py.min(), px.max(), py.max(), _bits(d[ok]).min())
    inst_img = np.where(won >= 0, values[np.clip(won, 0, max(I - 1, 0))] if I else -1, -1).astype(np.int32)
    return obj.reshape(H, W), inst_img.reshape(H, W), stats, unmatched, won.reshape(H, W)


def render(xyz, labels, foreign, inst, M0, W, H):
    """The level-0 frame of the model (instances_model.key_image): -> (idx (H,W) int32, depth (H,W) float32)."""
    static, pool, _, lst = instance_ranges(xyz, labels, foreign, inst)
    keys = im.key_image(static, pool, lst, M0, W, H)
    empty = keys == im.EMPTY
    idx = np.where(empty, 0, keys & np.uint64(0xFFFFFFFF)).astype(np.int32)
    dep = np.where(empty, 0, keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return idx.reshape(H, W), dep.reshape(H, W)


def key_matches(xyz, labels, foreign, inst, M0, W, H, i):
    """(H,W) bool: instance i drawn alone (visible or not) has, at the pixel, the key the whole frame has there."""
    static, pool, _, lst = instance_ranges(xyz, labels, foreign, inst)
    merged = im.key_image(static, pool, lst, M0, W, H)
    own = im.key_image(None, pool, [lst[i][:3] + (True,)], M0, W, H)
    return ((own == merged) & (merged != im.EMPTY)).reshape(H, W)


def first_instance_by_key_image(xyz, labels, foreign, inst, M0, W, H):
    """The cross-check: per pixel the first visible instance whose OWN key image has the merged key; -1 where the static part (or
    nothing) holds it.  -> (H,W) int32 list positions."""
    static, pool, _, lst = instance_ranges(xyz, labels, foreign, inst)
    merged = im.key_image(static, pool, lst, M0, W, H)
    won = np.full(W * H, -1, np.int32)
    for i in range(len(lst) - 1, -1, -1):
        if not lst[i][3] or lst[i][1] == 0:
            continue
        own = im.key_image(None, pool, [lst[i]], M0, W, H)
        won[(own == merged) & (merged != im.EMPTY)] = i
    return won.reshape(H, W)
