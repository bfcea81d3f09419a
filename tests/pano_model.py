"""The panorama (cylindrical) camera of the fast render path, defined once in NumPy.

``project_pano_one`` in read_amd/csrc/project.h restates ``project``: fp32 throughout, no fused operations, sums left to
right, IEEE division and correctly rounded square root.  The camera is the 16 fp32 numbers of ``read_amd.camera.pano_camera``:
r[12] (three rows applied to (x, y, z, 1): c0 = x_c, c1 = P[1,1] y_c, c3 = -z_c), kx = 2 / hfov_rad, ky = P[1,2], za = P[2,2],
zb = P[2,3].

Per point:  rho = sqrt(c0 c0 + c3 c3),  theta = atan2_model(c0, c3),  nx = theta kx,  ny = c1 / rho - ky,
nz = (zb - za rho) / rho,  then the tail of the pinhole's project_one (inside test, u, v, depth, integer conversion, range).
Per pixel the minimum of (depth bits << 32 | id) wins; empty pixels are (0, 0.0); level l is the same rule at
int(W 0.5^l) x int(H 0.5^l) and equals level 0's keys min-reduced 2x2.
"""
import numpy as np

f32 = np.float32
EMPTY_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)

# Abramowitz & Stegun 4.4.49: arctan(t) / t = 1 + a2 t^2 + ... + a16 t^16 on [0, 1], |error| <= 2e-8 before rounding.
# Highest power first (Horner in s = t^2); the constant term 1 closes the chain.  The kernel holds the same bit patterns.
ATAN_COEFFS = tuple(f32(c) for c in (0.0028662257, -0.0161657367, 0.0429096138, -0.0752896400, 0.1065626393, -0.1420889944,
                                     0.1999355085, -0.3333314528))
ATAN_COEFF_BITS = tuple(int(np.asarray(c, f32).view(np.uint32)) for c in ATAN_COEFFS)
PI_F = f32(3.14159265358979323846)
HALF_PI_F = f32(1.57079632679489661923)


def atan2_model(a, b):
    """fp32 arctangent of a / b in (-pi, pi], as the kernel computes it."""
    a = np.asarray(a, f32)
    b = np.asarray(b, f32)
    with np.errstate(all='ignore'):
        ax, az = np.abs(a), np.abs(b)
        swap = ax > az                                  # compare-and-select, not fmax / fmin: NaN takes the 'false' side
        large = np.where(swap, ax, az)
        small = np.where(swap, az, ax)
        t = np.where(large == f32(0), f32(0), small / np.where(large == f32(0), f32(1), large)).astype(f32)
        s = t * t
        p = np.full(s.shape, ATAN_COEFFS[0], f32)
        for c in ATAN_COEFFS[1:]:
            p = p * s + c
        p = p * s + f32(1)
        r = p * t
        r = np.where(swap, HALF_PI_F - r, r)
        r = np.where(b < f32(0), PI_F - r, r)
        return np.copysign(r, a).astype(f32)


def ndc(xyz, cam):
    """(nx, ny, nz) fp32 of every point."""
    xyz = np.asarray(xyz, f32)
    cam = np.asarray(cam, f32).reshape(16)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(all='ignore'):
        c0 = cam[0] * x + cam[1] * y + cam[2] * z + cam[3] * f32(1)
        c1 = cam[4] * x + cam[5] * y + cam[6] * z + cam[7] * f32(1)
        c3 = cam[8] * x + cam[9] * y + cam[10] * z + cam[11] * f32(1)
        kx, ky, za, zb = cam[12], cam[13], cam[14], cam[15]
        rho = np.sqrt(c0 * c0 + c3 * c3)
        theta = atan2_model(c0, c3)
        nx = theta * kx
        ny = c1 / rho - ky
        nz = (zb - za * rho) / rho
    return nx.astype(f32), ny.astype(f32), nz.astype(f32)


def tail(nx, ny, nz, W, H):
    """ndc_pixel, which project_one ends with: -> (pixel or -1 (int32), depth fp32, u, v)."""
    with np.errstate(all='ignore'):
        inside = (nx >= f32(-1)) & (nx <= f32(1)) & (ny >= f32(-1)) & (ny <= f32(1)) & (nz >= f32(-1)) & (nz <= f32(1))
        u = (f32(W) * (nx + f32(1))) * f32(0.5)
        v = (f32(H) * (f32(1) - ny)) * f32(0.5)
        depth = (nz + f32(1)) * f32(0.5)
        xx = np.where(inside, u, f32(0)).astype(np.int32)          # (int) truncates; only inside values are converted
        yy = np.where(inside, v, f32(0)).astype(np.int32)
    ok = inside & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
    pix = np.where(ok, yy * np.int32(W) + xx, np.int32(-1)).astype(np.int32)
    return pix, depth.astype(f32), u, v


def project(xyz, cam, W, H):
    """-> (pixel or -1 (int32), depth (fp32, meaningful where pixel >= 0))."""
    nx, ny, nz = ndc(xyz, cam)
    pix, depth, _, _ = tail(nx, ny, nz, W, H)
    return pix, depth


def project64(xyz, cam, W, H):
    """The same formulas in float64 with arctan2 in place of the polynomial (the fp32 camera and points, exactly converted).
    -> dict of nx, ny, nz, u, v, ok, pix."""
    p = np.asarray(xyz, f32).astype(np.float64)
    c = np.asarray(cam, f32).reshape(16).astype(np.float64)
    h = np.concatenate([p, np.ones((p.shape[0], 1))], 1)
    with np.errstate(all='ignore'):
        c0, c1, c3 = h @ c[0:4], h @ c[4:8], h @ c[8:12]
        rho = np.sqrt(c0 * c0 + c3 * c3)
        nx = np.arctan2(c0, c3) * c[12]
        ny = c1 / rho - c[13]
        nz = (c[15] - c[14] * rho) / rho
        inside = (nx >= -1) & (nx <= 1) & (ny >= -1) & (ny <= 1) & (nz >= -1) & (nz <= 1)
        u, v = W * (nx + 1) * 0.5, H * (1 - ny) * 0.5
        xx = np.where(inside, u, 0).astype(np.int64)
        yy = np.where(inside, v, 0).astype(np.int64)
    ok = inside & (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
    return {'nx': nx, 'ny': ny, 'nz': nz, 'u': u, 'v': v, 'ok': ok, 'pix': np.where(ok, yy * W + xx, -1)}


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


def unpack(keys, W, H):
    """-> (idx int32 (H, W), depth fp32 (H, W)); empty pixels are (0, 0.0)."""
    empty = keys == EMPTY_KEY
    idx = np.where(empty, 0, keys & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32).reshape(H, W)
    dep = np.where(empty, 0, keys >> np.uint64(32)).astype(np.uint32).view(f32).reshape(H, W)
    return idx, dep


def reduce2(keys, W, H):
    """2x2 key-min of a W x H key image (W, H even) -> (W/2) x (H/2)."""
    k = keys.reshape(H // 2, 2, W // 2, 2)
    return k.min(axis=(1, 3)).reshape(-1)


def level_size(W, H, l):
    return int(W * 0.5 ** l), int(H * 0.5 ** l)


def frame(xyz, cam, W, H, levels=5, ids=None):
    """Every level rasterised on its own -> (idx levels, depth levels)."""
    out = [unpack(key_image(xyz, cam, *level_size(W, H, l), ids=ids), *level_size(W, H, l)) for l in range(levels)]
    return [o[0] for o in out], [o[1] for o in out]


def pyramid_of(keys, W, H, levels=5):
    """Level 0's keys min-reduced 2x2, level after level -> (idx levels, depth levels)."""
    idx, dep = [], []
    for l in range(levels):
        w, h = level_size(W, H, l)
        i, d = unpack(keys, w, h)
        idx.append(i)
        dep.append(d)
        if l + 1 < levels:
            keys = reduce2(keys, w, h)
    return idx, dep


def object_camera(cam, P):
    """The camera of an object placed by P (4x4 or None): rows object_matrix(R4, P)[:3], the scalars unchanged."""
    from read_amd.raster import object_matrix
    cam = np.asarray(cam, f32).reshape(16)
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
