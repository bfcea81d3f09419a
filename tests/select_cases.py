"""Inputs the selection tests share (tests/test_select_cpu.py, tests/test_gpu_select.py): the posed-view vote case, whose
conditions the CPU test checks so that the GPU test cannot pass on a trivial case; random oriented boxes; the face-exact and
non-finite points; a small built scene with a car of known ids."""
import numpy as np

from read_amd import camera, synthetic
from read_amd.select import box_matrix

f32 = np.float32


# ---- the vote case -------------------------------------------------------------------------------------------------------------------
VOTE_N = 100_003
VOTE_W, VOTE_H = 64, 48
VOTE_REL, VOTE_SLACK = 0.05, 0.25
VOTE_MIN_HITS, VOTE_RATIO = 2, (1, 2)


def vote_case(W=VOTE_W, H=VOTE_H, n_views=4):
    """-> dict: xyz, W, H, totals (n_views x 16 floats), masks (n_views x (H,W) int32), rel, slack, min_hits, ratio.  The masks
    are given for 64 x 48 and scaled to other sizes by nearest pixel."""
    xyz = synthetic.make_street_cloud(VOTE_N)
    proj = synthetic.make_proj(W, H, f=48.0 * W / VOTE_W)
    totals = [camera.total_matrix(proj, synthetic.sweep_pose(8 * v))[0].reshape(16) for v in range(n_views)]
    masks = []
    for v in range(n_views):
        m = np.zeros((VOTE_H, VOTE_W), np.int32)
        if v == 3:
            m[10:40, 10:50] = 3
        else:
            m[8:30, 4:28] = 2 if v == 2 else 1
            m[20:44, 30:60] = 2
        if (W, H) != (VOTE_W, VOTE_H):
            m = m[(np.arange(H) * VOTE_H // H)[:, None], (np.arange(W) * VOTE_W // W)[None, :]]
        masks.append(np.ascontiguousarray(m))
    return {'xyz': xyz, 'W': W, 'H': H, 'totals': totals, 'masks': masks, 'rel': VOTE_REL, 'slack': VOTE_SLACK,
            'min_hits': VOTE_MIN_HITS, 'ratio': VOTE_RATIO}


# ---- boxes -----------------------------------------------------------------------------------------------------------------------------
CLOUD_LO = np.array([-60.0, -4.0, -120.0])
CLOUD_HI = np.array([60.0, 12.0, -1.0])
BOX_N = (0, 1, 255, 256, 257, 100_003)
BOX_K = (0, 1, 2, 33, 1024)


def _rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def random_boxes(K, seed):
    """K oriented boxes inside make_cloud's slab whose volumes add up to ~15 % of it (any yaw, tilt and roll up to 0.3 rad)
    -> ((K,12) float32, label_of (K,) int32 with repeated labels and, from K = 33 on, a few zeros)."""
    rng = np.random.default_rng([seed, K])
    vol = 0.15 * float(np.prod(CLOUD_HI - CLOUD_LO)) / max(K, 1)
    boxes = np.zeros((K, 12), f32)
    for k in range(K):
        u = (vol / 9.0) ** (1.0 / 3.0) * rng.uniform(0.8, 1.25)
        size = np.array([3.0 * u, min(u, 14.0), 3.0 * u]) * rng.uniform(0.8, 1.25, 3)
        lo, hi = CLOUD_LO + 0.3 * size, CLOUD_HI - 0.3 * size
        center = lo + rng.random(3) * np.maximum(hi - lo, 0.0)
        R = _rot(1, rng.uniform(0, 2 * np.pi)) @ _rot(0, rng.uniform(-0.3, 0.3)) @ _rot(2, rng.uniform(-0.3, 0.3))
        boxes[k] = box_matrix(center, size, R=R).reshape(12)
    label_of = (1 + rng.integers(0, max(K // 2, 1), K)).astype(np.int32)
    if K >= 33:
        label_of[rng.choice(K, K // 16, replace=False)] = 0
    return boxes, label_of


def face_points():
    """The axis-aligned box with centre 0 and half-size 2, and per axis and sign one point on the face (inside) and its fp32
    neighbour beyond (outside) -> (box (1,12), xyz (12,3), inside (12,) bool)."""
    two, beyond = f32(2), np.nextafter(f32(2), f32(3))
    pts, inside = [], []
    for axis in range(3):
        for sign in (1, -1):
            for v, ok in ((two, True), (beyond, False)):
                p = np.zeros(3, f32)
                p[axis] = f32(sign) * v
                pts.append(p)
                inside.append(ok)
    return box_matrix((0, 0, 0), (4, 4, 4)).reshape(1, 12), np.stack(pts), np.array(inside)


def nonfinite_points():
    """Points with a NaN or an infinity in one coordinate, all otherwise at the centre of face_points' box."""
    pts = []
    for axis in range(3):
        for v in (np.nan, np.inf, -np.inf):
            p = np.zeros(3, f32)
            p[axis] = v
            pts.append(p)
    return np.stack(pts)


# ---- a small built scene ----------------------------------------------------------------------------------------------------------------
CAR_CENTER = np.array([0.5, -0.8, -10.0])
CAR_HALF = np.array([0.9, 0.75, 2.1])


def car_scene(seed=21):
    """A ground plane, a wall across the street at z = -20 and a box-shaped car in front of it, shuffled
    -> (xyz (N,3) float32, is_car (N,) bool).  The car floats 15 cm above the ground, so its box (car_box) holds car points only."""
    rng = np.random.default_rng(seed)
    n_ground, n_wall, n_car = 12_000, 12_000, 6_000
    g = np.stack([rng.uniform(-8, 8, n_ground), np.full(n_ground, -1.7), rng.uniform(-30, -2, n_ground)], 1)
    w = np.stack([rng.uniform(-8, 8, n_wall), rng.uniform(-1.7, 4, n_wall), np.full(n_wall, -20.0)], 1)
    u = rng.uniform(-1, 1, (n_car, 3))
    face = rng.integers(0, 3, n_car)
    u[np.arange(n_car), face] = np.sign(u[np.arange(n_car), face])
    c = CAR_CENTER + u * CAR_HALF
    xyz = np.concatenate([g, w, c]).astype(f32)
    is_car = np.concatenate([np.zeros(n_ground + n_wall, bool), np.ones(n_car, bool)])
    order = rng.permutation(xyz.shape[0])
    return np.ascontiguousarray(xyz[order]), is_car[order]


def car_box():
    return box_matrix(CAR_CENTER, 2.0 * CAR_HALF + 0.1)
