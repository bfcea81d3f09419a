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


def lidar_camera(view_matrix, hfov_deg=360., rmin=0.5, rmax=120., half_width=np.deg2rad(0.2)):
    """The sensor of ``PointCloudRasterizer.sweep_lidar``: 16 float32 numbers, formed here in float64 and rounded once — like
    ``total_matrix`` an INPUT to the kernels, never re-derived on the device.

    [0:12]  three UNSCALED rows applied to (x, y, z, 1): c0 = x_c, c1 = y_c, c3 = -z_c (forward), with (x_c, y_c, z_c, 1) =
            inv(view) @ (x, y, z, 1); ``view_matrix`` is sensor->world.  These are the lens camera's rows; no projection matrix
    [12]    kx = 2 / hfov_rad: the azimuth column is W * (atan2(c0, c3) * kx + 1) / 2;  hfov_deg in (0, 360]
    [13:15] rmin > 0 and rmax >= rmin: a return's metric range lies in [rmin, rmax]
    [15]    half_width >= 0: a beam accepts elevations within this many RADIANS of its own"""
    hfov = float(hfov_deg)
    if not 0.0 < hfov <= 360.0:
        raise ValueError(f"hfov_deg must lie in (0, 360], got {hfov_deg!r}")
    rmin, rmax, half_width = float(rmin), float(rmax), float(half_width)
    if not (0.0 < rmin <= rmax and np.isfinite(rmax)):
        raise ValueError(f"a LiDAR needs 0 < rmin <= rmax < inf, got rmin = {rmin!r}, rmax = {rmax!r}")
    if not (half_width >= 0.0 and np.isfinite(half_width)):
        raise ValueError(f"half_width must be a finite angle >= 0 (radians), got {half_width!r}")
    w2c = np.linalg.inv(np.asarray(view_matrix, np.float64).reshape(4, 4))
    cam = np.empty(16, np.float64)
    cam[0:4] = w2c[0]
    cam[4:8] = w2c[1]
    cam[8:12] = -w2c[2]
    cam[12] = 2.0 / (hfov * (np.pi / 180.0))
    cam[13], cam[14], cam[15] = rmin, rmax, half_width
    return np.ascontiguousarray(cam.astype(np.float32))


LENS_PINHOLE, LENS_FISHEYE = 0, 1      # model 0: Brown-Conrady (k1, k2, p1, p2, k3); model 1: Kannala-Brandt (k1, k2, k3, k4)
LENS_LIMIT_SHARE = 0.999               # the default limit, as a share of the radial profile's first stationary point


def lens_stationary_point(model, coeffs):
    """Where the radial profile of a lens first stops growing, in float64, in the unit the rasteriser compares with the limit:
    r^2 for model 0 (profile r rad(r^2), r the normalised radius), theta in radians for model 1 (profile theta_d(theta)).  None:
    the profile grows for ever.

    The derivative of either profile is a polynomial in s = r^2 (or theta^2) — 1 + 3 k1 s + 5 k2 s^2 + 7 k3 s^3 (+ 9 k4 s^4) —,
    so the first stationary point is its smallest positive real root: the roots come from ``numpy.roots`` (the companion
    matrix's eigenvalues), one is taken as real when |imag| <= 1e-9 max(1, |real|), and the smallest positive one is polished by
    two Newton steps on the polynomial.  A double root (the profile pauses and goes on growing) counts as stationary."""
    k = _lens_coeffs(model, coeffs)
    radial = (k[0], k[1], k[4]) if int(model) == LENS_PINHOLE else (k[0], k[1], k[2], k[3])
    d = np.array([(2 * i + 3) * c for i, c in enumerate(radial)][::-1] + [1.0])     # highest power first
    d = np.trim_zeros(d, 'f')
    if d.size <= 1:
        return None
    roots = np.roots(d)
    real = roots.real[(np.abs(roots.imag) <= 1e-9 * np.maximum(1.0, np.abs(roots.real))) & (roots.real > 0)]
    if real.size == 0:
        return None
    s = float(real.min())
    for _ in range(2):
        slope = np.polyval(np.polyder(d), s)
        if slope != 0:
            s = float(s - np.polyval(d, s) / slope)
    return s if int(model) == LENS_PINHOLE else float(np.sqrt(s))


def _lens_coeffs(model, coeffs):
    if model not in (LENS_PINHOLE, LENS_FISHEYE):
        raise ValueError(f"lens model must be 0 (distorted pinhole) or 1 (fisheye), got {model!r}")
    want = 5 if int(model) == LENS_PINHOLE else 4
    k = np.zeros(5, np.float64)
    c = np.asarray([] if coeffs is None else coeffs, np.float64).reshape(-1)
    if c.size > want or not np.isfinite(c).all():
        raise ValueError(f"lens model {int(model)} takes up to {want} finite coefficients, got {coeffs!r}")
    k[:c.size] = c
    return k


def lens_camera(proj_matrix, view_matrix, model, coeffs, limit=None):
    """The lens camera of ``PointCloudRasterizer.render_lens``: 32 float32 numbers, formed here in float64 and rounded once —
    like ``total_matrix`` an INPUT to the rasteriser, never re-derived on the device.

    model 0: a pinhole with Brown-Conrady distortion, coeffs = OpenCV's (k1, k2, p1, p2, k3); model 1: a Kannala-Brandt fisheye,
    coeffs = OpenCV's fisheye (k1, k2, k3, k4), the equidistant fisheye when all are 0.  Missing coefficients are 0.

    [0:12]   three UNSCALED rows applied to (x, y, z, 1): c0 = x_c, c1 = y_c (the axis P[1,1] multiplies), c3 = -z_c (the forward
             distance), with (x_c, y_c, z_c, 1) = inv(view) @ (x, y, z, 1); ``view_matrix`` is camera->world
    [12:16]  sx = P[0,0], ox = P[0,2], sy = P[1,1], oy = P[1,2]: nx = sx a' - ox, ny = sy b' - oy of the distorted (a', b')
    [16:18]  za = P[2,2], zb = P[2,3]: nz = (zb - za d) / d, d = c3 (model 0) or the range (model 1)
    [18]     the limit: a point is drawn only while r^2 = a^2 + b^2 <= limit (model 0, a = c0 / c3, b = c1 / c3) or
             theta <= limit (model 1, the angle off the axis in radians)
    [19]     the model, 0.0 or 1.0;  [20:25] the coefficients in the order given;  [25:32] zero

    limit None: 0.999 of ``lens_stationary_point`` (beyond it the distortion polynomial folds points far outside the field
    back into the image), at most pi for model 1, +inf for model 0 when the profile never turns.  A smaller limit may be passed
    (a field mask: 190 degrees = np.deg2rad(95)); a negative one, or one above the stationary point (or pi), raises ValueError."""
    P = np.asarray(proj_matrix, np.float64).reshape(4, 4)
    k = _lens_coeffs(model, coeffs)
    model = int(model)
    top = lens_stationary_point(model, k[:5] if model == LENS_PINHOLE else k[:4])
    if model == LENS_FISHEYE:
        top = np.pi if top is None else min(top, np.pi)
    if limit is None:
        limit = np.inf if top is None else (np.pi if top == np.pi else LENS_LIMIT_SHARE * top)
        if model == LENS_FISHEYE:
            limit = min(limit, np.pi)
    else:
        limit = float(limit)
        if not limit >= 0.0:
            raise ValueError(f"the lens limit must be >= 0, got {limit!r}")
        if top is not None and limit > top:
            what = "pi" if top == np.pi else f"the radial profile's first stationary point {top:.6g}"
            raise ValueError(f"the lens limit {limit!r} lies above {what}: beyond it points fold back into the image")
    w2c = np.linalg.inv(np.asarray(view_matrix, np.float64).reshape(4, 4))
    cam = np.zeros(32, np.float64)
    cam[0:4] = w2c[0]
    cam[4:8] = w2c[1]
    cam[8:12] = -w2c[2]
    cam[12], cam[13], cam[14], cam[15] = P[0, 0], P[0, 2], P[1, 1], P[1, 2]
    cam[16], cam[17] = P[2, 2], P[2, 3]
    cam[18], cam[19] = limit, float(model)
    cam[20:25] = k
    with np.errstate(over='ignore'):
        out = cam.astype(np.float32)
    bound = float(np.float32(np.pi)) if top == np.pi else top    # theta never exceeds the fp32 pi of the model's arctangent
    if bound is not None and float(out[18]) > bound:
        out[18] = np.nextafter(out[18], np.float32(0))            # rounding must not lift the limit over its bound
    return np.ascontiguousarray(out)


def level_sizes(W, H, levels=5):
    """Per-scale raster sizes, ``int(W*0.5**i), int(H*0.5**i)`` (myrender.py:33-34)."""
    return [(int(W * 0.5 ** i), int(H * 0.5 ** i)) for i in range(levels)]
