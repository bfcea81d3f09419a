"""Clouds and cameras the panorama tests share (tests/test_pano_cpu.py, tests/test_gpu_pano.py): points all round the camera,
exact duplicates for ties, yawed / pitched / rolled poses, a projection with an off-centre principal row (ky != 0)."""
import numpy as np

from read_amd import camera


def ring_cloud(n, seed, dup=0):
    """n points in a 80 m x 16 m x 80 m box centred on the origin, the last ``dup`` of them exact copies of earlier ones."""
    rng = np.random.default_rng(seed)
    xyz = np.empty((n, 3), np.float32)
    m = n - dup
    xyz[:m, 0] = rng.uniform(-40, 40, m)
    xyz[:m, 1] = rng.uniform(-8, 8, m)
    xyz[:m, 2] = rng.uniform(-40, 40, m)
    if dup:
        xyz[m:] = xyz[rng.choice(m, dup, replace=False)]
    return xyz


def rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(4)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def pose(yaw=0.0, pitch=0.0, roll=0.0, t=(0.0, 0.0, 0.0)):
    """camera -> world: translate(t) o yaw(y) o pitch(x) o roll(z), degrees."""
    T = np.eye(4)
    T[:3, 3] = t
    return (T @ rot(1, yaw) @ rot(0, pitch) @ rot(2, roll)).astype(np.float32)


def proj(W, H, fy_scale=0.6, cy_shift=0.03):
    """get_proj_matrix with fy = fy_scale * H (vertical half-field atan(1 / (2 fy_scale))) and the principal row off the centre
    by cy_shift * H; the horizontal entries are not used by the panorama camera."""
    K = np.array([[fy_scale * H, 0, W / 2.0], [0, fy_scale * H, H * (0.5 + cy_shift)], [0, 0, 1.0]])
    return camera.get_proj_matrix(K, (W, H), 0.1, 1000.0).astype(np.float32)


def labels_for(n, seed, n_objects=3, share=0.1):
    """Random labels: ``share`` of the points to each of the objects 1..n_objects, the rest static."""
    rng = np.random.default_rng(seed)
    u = rng.random(n)
    lab = np.zeros(n, np.int32)
    for k in range(1, n_objects + 1):
        lab[(u >= share * (k - 1)) & (u < share * k)] = k
    return lab


def translation(t):
    P = np.eye(4, dtype=np.float32)
    P[:3, 3] = np.asarray(t, np.float32)
    return P
