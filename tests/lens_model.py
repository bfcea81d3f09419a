"""The lens camera of the fast render path — a distorted pinhole and a fisheye — defined once in NumPy.

``project_lens_one`` in read_amd/csrc/project.h restates ``project``: fp32 throughout, no fused operations, sums left to right,
IEEE division, correctly rounded square root, polynomials by Horner with separate multiply and add.  The camera is the 32 fp32
numbers of ``read_amd.camera.lens_camera``: r[12] (three unscaled rows applied to (x, y, z, 1): c0 = x_c, c1 = y_c, c3 = -z_c),
sx, ox, sy, oy = P[0,0], P[0,2], P[1,1], P[1,2], za, zb = P[2,2], P[2,3], the limit, the model (0.0 / 1.0), five coefficients.

Model 0 (Brown-Conrady; k1, k2, p1, p2, k3 as OpenCV orders them):
    a = c0 / c3, b = c1 / c3, r2 = a a + b b;  kept iff c3 > 0 and r2 <= limit;  rad = ((k3 r2 + k2) r2 + k1) r2 + 1;
    OpenCV's tangential terms in OpenCV's axes x = a, y = -b (its y points down, b points up):
        xy2 = 2 (x y),  tx = p1 xy2 + p2 (r2 + 2 (x x)),  ty = p1 (r2 + 2 (y y)) + p2 xy2,
        a' = x rad + tx,  b' = -(y rad + ty);
    d = c3.
Model 1 (Kannala-Brandt; k1..k4):
    rho = sqrt(c0 c0 + c1 c1), theta = atan2_model(rho, c3) in [0, pi];  kept iff theta <= limit;  t2 = theta theta,
    theta_d = theta ((((k4 t2 + k3) t2 + k2) t2 + k1) t2 + 1);  q = theta_d / rho, 0 where rho == 0 (the axis point lands on the
    principal point);  a' = q c0, b' = q c1;  d = sqrt(c0 c0 + c1 c1 + c3 c3), the range (c3 is <= 0 past 180 degrees).
Both:  nx = sx a' - ox,  ny = sy b' - oy,  nz = (zb - za d) / d,  then the tail of the pinhole's project_one.  A point that is
not kept, or NaN / Inf anywhere, has no pixel.  Per pixel the minimum of (depth bits << 32 | id) wins; empty pixels are (0, 0.0);
level l is the same rule at int(W 0.5^l) x int(H 0.5^l) and equals level 0's keys min-reduced 2x2.

The limit.  A distortion polynomial folds back: past the first stationary point of the radial profile (r rad(r^2) for model 0,
theta_d(theta) for model 1) points far outside the field land inside the image again.  ``camera.lens_stationary_point`` finds
it in float64 as the smallest positive real root of the profile's derivative — a polynomial in s = r^2 or theta^2,
1 + 3 k1 s + 5 k2 s^2 + 7 k3 s^3 (+ 9 k4 s^4) — from numpy.roots (real when |imag| <= 1e-9 max(1, |real|)), polished by two
Newton steps; ``stationary_point`` below restates it by bracketing and bisection, and the tests compare the two.  The limit is
compared as r2 (model 0) or theta (model 1); the default is 0.999 of the stationary point, at most pi for model 1, +inf for
model 0 without one.
"""
import numpy as np

from tests.pano_model import EMPTY_KEY, atan2_model, level_size, pyramid_of, reduce2, tail, unpack  # noqa: F401  (shared, not restated)

f32 = np.float32


def _rows(xyz, cam):
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    c0 = cam[0] * x + cam[1] * y + cam[2] * z + cam[3] * f32(1)
    c1 = cam[4] * x + cam[5] * y + cam[6] * z + cam[7] * f32(1)
    c3 = cam[8] * x + cam[9] * y + cam[10] * z + cam[11] * f32(1)
    return c0, c1, c3


def ndc(xyz, cam):
    """(nx, ny, nz) fp32 of every point and ``keep``, the model's own accept test (c3 > 0 and r2 <= limit, or theta <= limit)."""
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    cam = np.asarray(cam, f32).reshape(32)
    sx, ox, sy, oy, za, zb, limit = cam[12:19]
    k = cam[20:25]
    with np.errstate(all='ignore'):
        c0, c1, c3 = _rows(xyz, cam)
        if cam[19] == f32(0):
            k1, k2, p1, p2, k3 = k
            a = c0 / c3
            b = c1 / c3
            r2 = a * a + b * b
            keep = (c3 > f32(0)) & (r2 <= limit)
            rad = ((k3 * r2 + k2) * r2 + k1) * r2 + f32(1)
            x, y = a, -b
            xy2 = f32(2) * (x * y)
            tx = p1 * xy2 + p2 * (r2 + f32(2) * (x * x))
            ty = p1 * (r2 + f32(2) * (y * y)) + p2 * xy2
            a2 = x * rad + tx
            b2 = -(y * rad + ty)
            d = c3
        else:
            k1, k2, k3, k4 = k[:4]
            rho = np.sqrt(c0 * c0 + c1 * c1)
            theta = atan2_model(rho, c3)
            keep = theta <= limit
            t2 = theta * theta
            theta_d = theta * ((((k4 * t2 + k3) * t2 + k2) * t2 + k1) * t2 + f32(1))
            q = np.where(rho == f32(0), f32(0), theta_d / np.where(rho == f32(0), f32(1), rho)).astype(f32)
            a2 = q * c0
            b2 = q * c1
            d = np.sqrt(c0 * c0 + c1 * c1 + c3 * c3)
        nx = sx * a2 - ox
        ny = sy * b2 - oy
        nz = (zb - za * d) / d
    return nx.astype(f32), ny.astype(f32), nz.astype(f32), keep


def project(xyz, cam, W, H):
    """-> (pixel or -1 (int32), depth (fp32, meaningful where pixel >= 0))."""
    nx, ny, nz, keep = ndc(xyz, cam)
    pix, depth, _, _ = tail(nx, ny, nz, W, H)
    return np.where(keep, pix, np.int32(-1)).astype(np.int32), depth


def project64(xyz, cam, W, H):
    """The same formulas in float64 with arctan2 in place of the polynomial (the fp32 camera and points, exactly converted).
    -> dict of nx, ny, nz, u, v, ok, pix and ``r``, the quantity compared with the limit (r2 or theta)."""
    p = np.asarray(xyz, f32).reshape(-1, 3).astype(np.float64)
    c = np.asarray(cam, f32).reshape(32).astype(np.float64)
    h = np.concatenate([p, np.ones((p.shape[0], 1))], 1)
    sx, ox, sy, oy, za, zb, limit = c[12:19]
    k = c[20:25]
    with np.errstate(all='ignore'):
        c0, c1, c3 = h @ c[0:4], h @ c[4:8], h @ c[8:12]
        if c[19] == 0:
            k1, k2, p1, p2, k3 = k
            a, b = c0 / c3, c1 / c3
            r = a * a + b * b
            keep = (c3 > 0) & (r <= limit)
            rad = 1 + r * (k1 + r * (k2 + r * k3))
            x, y = a, -b
            a2 = x * rad + 2 * p1 * x * y + p2 * (r + 2 * x * x)
            b2 = -(y * rad + p1 * (r + 2 * y * y) + 2 * p2 * x * y)
            d = c3
        else:
            k1, k2, k3, k4 = k[:4]
            rho = np.sqrt(c0 * c0 + c1 * c1)
            r = np.arctan2(rho, c3)
            keep = r <= limit
            t2 = r * r
            theta_d = r * (1 + t2 * (k1 + t2 * (k2 + t2 * (k3 + t2 * k4))))
            q = np.where(rho == 0, 0.0, theta_d / np.where(rho == 0, 1.0, rho))
            a2, b2 = q * c0, q * c1
            d = np.sqrt(c0 * c0 + c1 * c1 + c3 * c3)
        nx, ny, nz = sx * a2 - ox, sy * b2 - oy, (zb - za * d) / d
        inside = (nx >= -1) & (nx <= 1) & (ny >= -1) & (ny <= 1) & (nz >= -1) & (nz <= 1)
        u, v = W * (nx + 1) * 0.5, H * (1 - ny) * 0.5
        xx = np.where(inside, u, 0).astype(np.int64)
        yy = np.where(inside, v, 0).astype(np.int64)
    ok = keep & inside & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
    return {'nx': nx, 'ny': ny, 'nz': nz, 'u': u, 'v': v, 'ok': ok, 'pix': np.where(ok, yy * W + xx, -1), 'r': r, 'keep': keep,
            'inside': inside}


def stationary_point(model, coeffs):
    """``camera.lens_stationary_point`` restated without a root finder: the derivative polynomial in s is sampled on a fine
    geometric grid, its first sign change (or exact zero) bracketed, and the bracket bisected.  None when the grid sees none up
    to s = 1e4.  -> r^2 (model 0) or theta (model 1)."""
    k = np.zeros(5)
    k[:len(coeffs)] = coeffs
    radial = (k[0], k[1], k[4]) if model == 0 else (k[0], k[1], k[2], k[3])

    def deriv(s):
        out = np.ones_like(s)
        for i, c in enumerate(radial):
            out = out + (2 * i + 3) * c * s ** (i + 1)
        return out

    s = np.concatenate([[0.0], np.geomspace(1e-8, 1e4, 2_000_001)])
    neg = np.flatnonzero(deriv(s) <= 0)
    if neg.size == 0:
        return None
    lo, hi = s[neg[0] - 1], s[neg[0]]
    for _ in range(100):
        mid = 0.5 * (lo + hi)
        if deriv(np.float64(mid)) > 0:
            lo = mid
        else:
            hi = mid
    return float(hi) if model == 0 else float(np.sqrt(hi))


# ---- frames -------------------------------------------------------------------------------------------------------------------
def key_image(xyz, cam, W, H, ids=None, keys=None):
    """The W*H uint64 key image of one range of points under one camera, folded into ``keys`` when given."""
    if keys is None:
        keys = np.full(W * H, EMPTY_KEY, np.uint64)
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    if xyz.shape[0] == 0:
        return keys
    ids = np.arange(xyz.shape[0], dtype=np.uint64) if ids is None else np.asarray(ids).astype(np.uint64)
    pix, depth = project(xyz, cam, W, H)
    ok = pix >= 0
    k = (depth[ok].view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids[ok]
    np.minimum.at(keys, pix[ok], k)
    return keys


def frame(xyz, cam, W, H, levels=5, ids=None):
    """Every level rasterised on its own -> (idx levels, depth levels)."""
    out = [unpack(key_image(xyz, cam, *level_size(W, H, l), ids=ids), *level_size(W, H, l)) for l in range(levels)]
    return [o[0] for o in out], [o[1] for o in out]


def object_camera(cam, P):
    """The camera of an object placed by P (4x4 or None): rows object_matrix(R4, P)[:3], the twenty scalars unchanged."""
    from read_amd.raster import object_matrix
    cam = np.asarray(cam, f32).reshape(32)
    R4 = np.concatenate([cam[:12].reshape(3, 4), np.array([[0, 0, 0, 1]], f32)], 0)
    out = cam.copy()
    out[:12] = object_matrix(R4, P)[:3].reshape(12)
    return out


def labelled_keys(xyz, labels, cam, poses, hidden, W, H):
    """Level-0 key image of a labelled cloud: label 0 under ``cam``, label k under object_camera(cam, poses.get(k)), hidden
    labels left out; ids are the points' indices in the whole cloud."""
    xyz = np.asarray(xyz, f32)
    labels = np.asarray(labels)
    keys = np.full(W * H, EMPTY_KEY, np.uint64)
    for k in np.unique(labels):
        if int(k) in hidden:
            continue
        sel = np.nonzero(labels == k)[0]
        key_image(xyz[sel], cam if k == 0 else object_camera(cam, poses.get(int(k))), W, H, ids=sel, keys=keys)
    return keys
