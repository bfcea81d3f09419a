"""Camera / clip-space conventions of READ's render path (host side, per frame: 16 floats).

``get_proj_matrix`` mirrors READ/gl/utils.py:123-150 (OpenGL-style projection from a
pinhole K; column-vector convention ``clip = P @ x_cam``; the camera looks down -z).
``total_matrix`` mirrors src/READ/gl/myrender.py:28-30 (``proj @ inv(view)``, fp32; the
result is an INPUT to the rasteriser — it is computed once on the host and the same 16
floats go to every consumer, never re-derived on the device).
"""
import numpy as np


def get_proj_matrix(K, image_size, znear=.01, zfar=1000.):
    """4x4 projection such that ``ndc = (P @ [x,y,z,1]) / w`` (READ/gl/utils.py:123-150)."""
    K = np.asarray(K)
    width, height = image_size
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    P = np.zeros((4, 4))
    P[0, 0] = 2.0 * fx / width
    P[1, 1] = 2.0 * fy / height
    P[0, 2] = 1.0 - 2.0 * cx / width
    P[1, 2] = 2.0 * cy / height - 1.0
    P[2, 2] = (zfar + znear) / (znear - zfar)
    P[2, 3] = 2.0 * zfar * znear / (znear - zfar)
    P[3, 2] = -1.0
    return P


def total_matrix(proj_matrix, view_matrix):
    """``proj @ inv(view)`` per batch item in the dtype of the inputs (myrender.py:28-30).

    ``view_matrix`` is camera->world.  Accepts (4,4) or (B,4,4); returns float32 (B,4,4)."""
    p = np.asarray(proj_matrix)
    v = np.asarray(view_matrix)
    if p.ndim == 2:
        p = p[None]
    if v.ndim == 2:
        v = v[None]
    return np.ascontiguousarray((p @ np.linalg.inv(v)).astype(np.float32))


def pano_camera(proj_matrix, view_matrix, hfov_deg):
    """The panorama (cylindrical) camera of ``PointCloudRasterizer.render_pano``: 16 float32 numbers, formed here in float64 and
    rounded once — like ``total_matrix`` an INPUT to the rasteriser, never re-derived on the device.

    [0:12]  three rows applied to (x, y, z, 1): c0 = x_c, c1 = P[1,1] * y_c, c3 = -z_c (the forward distance), with
            (x_c, y_c, z_c, 1) = inv(view) @ (x, y, z, 1); ``view_matrix`` is camera->world
    [12]    kx = 2 / hfov_rad: the column is W * (atan2(c0, c3) * kx + 1) / 2
    [13:16] ky = P[1,2], za = P[2,2], zb = P[2,3]: row and depth are the pinhole's of the same P at c0 = 0
    P[0,0] and P[0,2] are not used.  hfov_deg in (0, 360]."""
    P = np.asarray(proj_matrix, np.float64).reshape(4, 4)
    hfov = float(hfov_deg)
    if not 0.0 < hfov <= 360.0:
        raise ValueError(f"hfov_deg must lie in (0, 360], got {hfov_deg!r}")
    w2c = np.linalg.inv(np.asarray(view_matrix, np.float64).reshape(4, 4))
    cam = np.empty(16, np.float64)
    cam[0:4] = w2c[0]
    cam[4:8] = P[1, 1] * w2c[1]
    cam[8:12] = -w2c[2]
    cam[12] = 2.0 / (hfov * (np.pi / 180.0))
    cam[13], cam[14], cam[15] = P[1, 2], P[2, 2], P[2, 3]
    return np.ascontiguousarray(cam.astype(np.float32))


def level_sizes(W, H, levels=5):
    """Per-scale raster sizes, ``int(W*0.5**i), int(H*0.5**i)`` (myrender.py:33-34)."""
    return [(int(W * 0.5 ** i), int(H * 0.5 ** i)) for i in range(levels)]
