"""Scene editing, third verb (add): the NumPy model of the instance contract (include/read_hip.h, read_splat_forward_instances,
read_splat_forward_pano_instances, read_gather_forward_tables) and the per-instance oracle.  Used by tests/test_instances_cpu.py
(model against the oracle) and tests/test_gpu_instances.py (kernels against both).

A frame = the static part (points + ids, camera M_0) and a list of instances; instance i = (first, npts, P, visible) draws pool
points [first, first + npts) with object_matrix(M_0, P).  Per pixel the minimum of depth bits << 32 | id over every visible point
wins; empty pixels are (0, 0.0); level l + 1 is the 2x2 key minimum of level l."""
import numpy as np

import oracle
from read_amd import camera
from read_amd.raster import object_matrix
from tests import pano_model as pm

LEVELS = 5
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


# ---- raster model ------------------------------------------------------------------------------------------------------------
def _fold(keys, xyz, ids, pix, depth):
    ok = pix >= 0
    k = (np.ascontiguousarray(depth[ok], np.float32).view(np.uint32).astype(np.uint64) << np.uint64(32)) | \
        np.asarray(ids)[ok].astype(np.uint64)
    np.minimum.at(keys, pix[ok], k)


def key_image(static, pool, instances, M0, W, H, pano=False):
    """static = (xyz, ids) or None; pool = (xyz, ids); instances = [(first, npts, P, visible)] -> level-0 keys (W*H uint64).
    pano: M0 is a panorama camera (16 floats) and instance cameras are pano_model.object_camera(M0, P)."""
    keys = np.full(W * H, EMPTY, np.uint64)

    def draw(xyz, ids, P):
        if len(xyz) == 0:
            return
        if pano:
            pix, depth = pm.project(xyz, M0 if P is None else pm.object_camera(M0, P), W, H)
        else:
            pix, depth = oracle.project_points(np.ascontiguousarray(xyz, np.float32), object_matrix(M0, P), W, H)
        _fold(keys, xyz, ids, pix, depth)
    if static is not None:
        draw(static[0], static[1], None)
    for first, npts, P, visible in instances:
        if visible and npts > 0:
            draw(pool[0][first:first + npts], pool[1][first:first + npts], P)
    return keys


def frame(static, pool, instances, M0, W, H, levels=LEVELS, pano=False):
    """-> (idx levels int32, depth levels fp32)."""
    return pm.pyramid_of(key_image(static, pool, instances, M0, W, H, pano), W, H, levels)


# ---- the per-instance oracle: tests/test_gpu_objects.py::oracle_edit, per instance instead of per label ----------------------------
def oracle_frame(static, pool, instances, M0, W, H, levels=LEVELS):
    """oracle.raster_multiscale on every drawn range with its own matrix, local ids mapped to the range's ids, merged on the key."""
    sizes = camera.level_sizes(W, H, levels)
    keys = [np.full((h, w), EMPTY, np.uint64) for (w, h) in sizes]

    def draw(xyz, ids, P):
        if len(xyz) == 0:
            return
        ids = np.asarray(ids)
        oi, od = oracle.raster_multiscale(np.ascontiguousarray(xyz, np.float32), object_matrix(M0, P), W, H, levels, threads=16)
        for l in range(levels):
            bits = od[l].view(np.uint32)
            key = (bits.astype(np.uint64) << np.uint64(32)) | ids[oi[l]].astype(np.uint64)
            key[(oi[l] == 0) & (bits == 0)] = EMPTY
            keys[l] = np.minimum(keys[l], key)
    if static is not None:
        draw(static[0], static[1], None)
    for first, npts, P, visible in instances:
        if visible and npts > 0:
            draw(pool[0][first:first + npts], pool[1][first:first + npts], P)
    idx, dep = [], []
    for key in keys:
        empty = key == EMPTY
        idx.append(np.where(empty, 0, key & np.uint64(0xFFFFFFFF)).astype(np.int32))
        dep.append(np.where(empty, 0, key >> np.uint64(32)).astype(np.uint32).view(np.float32))
    return idx, dep


def layout(xyz, labels, foreign=()):
    """The rasteriser's split of a labelled cloud plus foreign objects: -> (static, pool, ranges); static = (xyz, ids) of label 0,
    pool = (xyz, ids) of the labelled points label after label (ascending ids) followed by the foreign objects' with ids N, N + 1,
    ..., ranges[k - 1] = (first, npts) of object k (labels 1..K, then the foreign objects)."""
    xyz = np.asarray(xyz, np.float32)
    labels = np.zeros(xyz.shape[0], np.int64) if labels is None else np.asarray(labels)
    K = int(labels.max()) if labels.size else 0
    sel0 = np.flatnonzero(labels == 0)
    px, pi, ranges, at = [], [], [], 0
    for k in range(1, K + 1):
        sel = np.flatnonzero(labels == k)
        px.append(xyz[sel]), pi.append(sel), ranges.append((at, sel.size))
        at += sel.size
    base = xyz.shape[0]
    for f in foreign:
        f = np.asarray(f, np.float32)
        px.append(f), pi.append(np.arange(base, base + f.shape[0])), ranges.append((at, f.shape[0]))
        at += f.shape[0]
        base += f.shape[0]
    pool = (np.concatenate(px) if px else np.zeros((0, 3), np.float32), np.concatenate(pi) if pi else np.zeros(0, np.int64))
    return (xyz[sel0], sel0), pool, ranges


# ---- the gather over several tables ------------------------------------------------------------------------------------------------
def _act(v, activation):
    v = np.asarray(v, np.float32)
    if activation == 'sigmoid':
        return (np.float32(1) / (np.float32(1) + np.exp(-v, dtype=np.float32))).astype(np.float32)
    if activation == 'tanh':
        return np.tanh(v, dtype=np.float32)
    return v


def select(tables, idx):
    """tables = [(rows (n_t, C), id_base_t, activation_t)] -> (table number, local id) per id: the last table whose base is <= id,
    the local id clamped to [0, n_t - 1]; an id below 0 is row 0 of table 0."""
    ids = np.asarray(idx).astype(np.int64)
    bases = np.array([b for _, b, _ in tables], np.int64)
    ns = np.array([r.shape[0] for r, _, _ in tables], np.int64)
    t = np.clip(np.searchsorted(bases, ids, side='right') - 1, 0, None)
    return t, np.clip(ids - bases[t], 0, ns[t] - 1)


def gather_tables(tables, idx):
    """-> feat (idx.shape + (C,)) float32: act_t(rows_t[local id])."""
    t, loc = select(tables, idx)
    out = np.empty(np.shape(idx) + (tables[0][0].shape[1],), np.float32)
    for s, (rows, _, activation) in enumerate(tables):
        sel = t == s
        out[sel] = _act(np.asarray(rows, np.float32)[loc[sel]], activation)
    return out
