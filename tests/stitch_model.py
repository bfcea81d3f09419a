"""Scene stitching: the NumPy model of the merge contract (include/read_hip.h, read_stitch_gather_forward) and the shared scene
of the union check.  Used by tests/test_stitch_cpu.py (against the oracle) and tests/test_gpu_stitch.py (against the kernel)."""
import functools

import numpy as np

import oracle
from read_amd import camera, synthetic

LEVELS = 5
W, H = 64, 48
COUNTS = (20_000, 15_000, 5_000)
DUPLICATES = 250


def merge(parts, visible=None):
    """parts: list of (idx_levels, depth_levels, id_base) with int32 / float32 arrays per level (local ids).
    -> (idx_levels, depth_levels, part_levels, local_levels): merged global ids (int32), merged depths (float32), winning part
    (uint8, 255 = no candidate) and the winner's local id (int32, 0 where no candidate), level by level.
    Candidates: visible parts whose pixel is not (idx == 0 and depth bits == 0); winner: smallest depth bit pattern as an unsigned
    number, ties to the lowest part; no candidate: idx 0, depth 0.0."""
    visible = [True] * len(parts) if visible is None else list(visible)
    levels = len(next(p for p in parts if p[0] is not None)[0])
    out_i, out_d, out_p, out_l = [], [], [], []
    for l in range(levels):
        shape = next(p for p in parts if p[0] is not None)[0][l].shape
        best = np.full(shape, 1 << 32, np.int64)             # above every 32-bit pattern
        idx = np.zeros(shape, np.int32)
        loc = np.zeros(shape, np.int32)
        part = np.full(shape, 255, np.uint8)
        for s, (pi, pd, base) in enumerate(parts):
            if not visible[s] or pi is None:
                continue
            bits = np.ascontiguousarray(pd[l], np.float32).view(np.uint32).astype(np.int64)
            cand = ~((pi[l] == 0) & (bits == 0))
            take = cand & (bits < best)                       # strict: a tie stays with the lower part
            best = np.where(take, bits, best)
            idx = np.where(take, pi[l].astype(np.int64) + base, idx).astype(np.int32)
            loc = np.where(take, pi[l], loc).astype(np.int32)
            part = np.where(take, s, part).astype(np.uint8)
        dep = np.where(part == 255, 0, best).astype(np.uint32).view(np.float32)
        out_i.append(idx), out_d.append(dep), out_p.append(part), out_l.append(loc)
    return out_i, out_d, out_p, out_l


def features(rows, part_levels, local_levels):
    """Activation 'none': feat[p] = rows[part][local id], no candidate -> rows[0][0].  rows: list of (n_s, C) float32 arrays."""
    out = []
    for part, loc in zip(part_levels, local_levels):
        f = np.broadcast_to(rows[0][0], part.shape + (rows[0].shape[1],)).copy()
        for s, r in enumerate(rows):
            sel = part == s
            f[sel] = r[loc[sel]]
        out.append(f)
    return out


def id_bases(counts):
    return [int(sum(counts[:s])) for s in range(len(counts))]


def union_camera(w=W, h=H):
    """The clouds of synthetic.make_cloud seen from 60 m behind their near face: a band across the middle of the image, empty
    rows above and below it at every level (16 rows of level 0 = one row of level 4)."""
    view = np.eye(4, dtype=np.float32)
    view[1, 3], view[2, 3] = 4.0, 60.0
    return camera.total_matrix(synthetic.make_proj(w, h, f=60.0 * w / W), view)[0]


@functools.lru_cache(maxsize=None)
def union_scene(counts=COUNTS, w=W, h=H):
    """-> (clouds, M): clouds of `counts` points from synthetic.make_cloud with seeds 1, 2, 3, ... in which DUPLICATES points that
    win pixels of the union — the winners of the coarsest level among them, so that every level has ties — also sit, at exactly
    their position, in the next part (they overwrite its last points)."""
    clouds = [synthetic.make_cloud(n, seed=s + 1).copy() for s, n in enumerate(counts)]
    M = union_camera(w, h)
    base = id_bases(counts)
    tail = DUPLICATES                                         # no source among the points that may be overwritten
    oi, od = oracle.raster_multiscale(np.concatenate(clouds), M, w, h, LEVELS)

    def winners(l):
        covered = ~((oi[l] == 0) & (od[l].view(np.uint32) == 0))
        ids = np.unique(oi[l][covered])
        part = np.searchsorted(np.asarray(base), ids, side='right') - 1
        keep = ids - np.asarray(base)[part] < np.asarray(counts)[part] - tail
        return ids[keep]
    coarse = winners(LEVELS - 1)
    fine = np.setdiff1d(winners(0), coarse)
    rng = np.random.default_rng(5)
    src = np.concatenate([coarse, rng.choice(fine, DUPLICATES - coarse.size, replace=False)])
    slot = [0] * len(counts)
    for g in src:
        a = int(np.searchsorted(np.asarray(base), g, side='right') - 1)
        b = (a + 1) % len(counts)
        slot[b] += 1
        clouds[b][counts[b] - slot[b]] = clouds[a][g - base[a]]
    return clouds, M


@functools.lru_cache(maxsize=None)
def union_oracle(counts=COUNTS, w=W, h=H):
    """The reference of the union check, computed once: the oracle on the concatenated cloud and on every part."""
    clouds, M = union_scene(counts, w, h)
    whole = oracle.raster_multiscale(np.concatenate(clouds), M, w, h, LEVELS)
    parts = [oracle.raster_multiscale(c, M, w, h, LEVELS) for c in clouds]
    return whole, parts


def tie_and_empty_counts(parts, visible=None):
    """Per level: (pixels where two or more visible candidates share the smallest depth bit pattern, pixels without a candidate)."""
    out = []
    visible = [True] * len(parts) if visible is None else visible
    for l in range(len(parts[0][0])):
        bits = np.stack([np.where((pi[l] == 0) & (pd[l].view(np.uint32) == 0), 1 << 32, pd[l].view(np.uint32).astype(np.int64))
                         for s, (pi, pd) in enumerate(parts) if visible[s]])
        lo = bits.min(0)
        out.append((int((((bits == lo).sum(0) >= 2) & (lo < (1 << 32))).sum()), int((lo == (1 << 32)).sum())))
    return out
