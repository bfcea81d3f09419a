"""Clouds, projections and lenses the lens-camera tests share (tests/test_lens_cpu.py, tests/test_gpu_lens.py): the panorama
tests' ring cloud and poses, projections with the principal point off the centre on both axes, and coefficients of realistic
size — a wide forward camera (Brown-Conrady), a 200-degree surround fisheye (Kannala-Brandt), the equidistant fisheye."""
import numpy as np

from read_amd import camera
from tests.pano_cases import labels_for, pose, ring_cloud, rot, translation  # noqa: F401  (shared, not restated)

# name -> model, coeffs, horizontal focal length as a share of W, limit (None: camera.lens_camera's default)
LENSES = {
    "brown": (0, (-0.28, 0.07, 0.0006, -0.0004, -0.008), 0.5, None),
    "fisheye": (1, (-0.03, 0.002, -0.0005, 0.00003), 0.26, float(np.deg2rad(100.0))),           # a 200-degree field mask
    "equidistant": (1, (), 1.0 / np.pi, None),                                                  # 180 degrees over W
}
FOLDING = (0, (-0.3,), 0.5, None)          # r rad(r^2) turns at r^2 = 1 / 0.9: points beyond it would land in the image again


def proj(W, H, fx_share, cx_shift=0.02, cy_shift=0.03):
    """get_proj_matrix of K = [[fx, 0, cx], [0, fx, cy], [0, 0, 1]], fx = fx_share W, the principal point off the centre."""
    fx = fx_share * W
    K = np.array([[fx, 0, W * (0.5 + cx_shift)], [0, fx, H * (0.5 + cy_shift)], [0, 0, 1.0]])
    return camera.get_proj_matrix(K, (W, H), 0.1, 1000.0).astype(np.float32)


def intrinsics(P, W, H):
    """The documented K <-> P relation of camera.get_proj_matrix, solved for OpenCV's fx, fy, cx, cy (pixels, y down)."""
    P = np.asarray(P, np.float64)
    return P[0, 0] * W / 2.0, P[1, 1] * H / 2.0, (1.0 - P[0, 2]) * W / 2.0, (P[1, 2] + 1.0) * H / 2.0


def lens_cam(lens, W, H, view):
    model, coeffs, fx_share, limit = LENSES[lens] if isinstance(lens, str) else lens
    return camera.lens_camera(proj(W, H, fx_share), view, model, coeffs, limit)


def lens_args(lens):
    model, coeffs, _, limit = LENSES[lens]
    return model, coeffs, limit
