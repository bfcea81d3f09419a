"""The spinning LiDAR of the fitted scene, defined once in NumPy.  read_amd/csrc/lidar.hip restates it bit for
bit: fp32 throughout, nothing fused, sums left to right, IEEE division, correctly rounded square root — the rules of
``project_pano_one`` — and the arctangent is ``pano_model.atan2_model``.

Sensor.  ``cam`` = the 16 fp32 numbers of ``read_amd.camera.lidar_camera``: cam[0:12] three UNSCALED rows applied to (x, y, z, 1)
giving c0 = x_c, c1 = y_c, c3 = -z_c (forward); cam[12] = kx = 2 / hfov_rad; cam[13] = rmin > 0; cam[14] = rmax >= rmin;
cam[15] = delta >= 0, a beam's acceptance half-width in radians.  ``elev`` = B fp32 beam elevations in radians, finite, strictly
ascending, 1 <= B <= 128; row b of every image is beam b (row 0 the lowest beam); W azimuth columns.

Per point.  q = c0 c0 + c3 c3, rho = sqrt(q), theta = atan2_model(c0, c3), phi = atan2_model(c1, rho), r = sqrt(q + c1 c1),
nx = theta kx.  Column: -1 <= nx <= 1, u = (W (nx + 1)) 0.5, col = (int)u, accepted iff 0 <= col < W (theta = +pi falls on column
W and is dropped).  Beam: d_b = |phi - elev[b]|; the beam is the b of the smallest d_b, ties to the lower b; accepted iff
d_b <= delta.  Range: accepted iff rmin <= r and r <= rmax.  A comparison with a NaN is false.  The cell is b W + col.

Per cell the minimum of (range bits << 32 | id) wins; r >= rmin > 0, so the empty cell (id 0, range 0.0) is never ambiguous.

See-through filter, on the COMPLETE key image, never in place: for a cell with a return of range r, near = the smallest range over
the returns of the cells with |db| <= wb, |dc| <= wc (rows clipped at the table's ends; columns modulo W iff wrap, else clipped;
the cell itself counts), lim = near scale + slack (a product, then a sum), kept iff r <= lim, else the cell becomes empty.

Return list, in ascending cell order: count (all kept returns, also beyond the capacity) and, for the first min(count, capacity)
of them, cell, id and xyz in the sensor frame ALONG THE BEAM: x = (r ce_b) st_c, y = r se_b, z = -((r ce_b) ct_c) with the host
tables beam_dir[b] = (cos, sin) of the fp32 elev[b] and col_dir[c] = (sin, cos) of theta_c = ((c + 0.5) / W 2 - 1) / kx, each
computed in float64 and rounded once.
"""
import numpy as np

from tests import pano_model as pm

f32 = np.float32
EMPTY_KEY = pm.EMPTY_KEY
MAX_BEAMS = 128
MAX_WINDOW = 4


# ---- the host tables ----------------------------------------------------------------------------------------------------------
def beam_dir(elev):
    """(B, 2) fp32: (cos, sin) of the fp32 elevations, in float64, rounded once."""
    e = np.asarray(elev, f32).astype(np.float64)
    return np.stack([np.cos(e), np.sin(e)], 1).astype(f32)


def col_dir(W, kx):
    """(W, 2) fp32: (sin, cos) of the centre azimuth of every column under the fp32 kx, in float64, rounded once."""
    th = ((np.arange(W, dtype=np.float64) + 0.5) / W * 2.0 - 1.0) / float(f32(kx))
    return np.stack([np.sin(th), np.cos(th)], 1).astype(f32)


# ---- per point ----------------------------------------------------------------------------------------------------------------
def beam_linear(phi, elev):
    """The definition: -> (b int32, d fp32), b the first index of the smallest |phi - elev[b]| by a scan that replaces its
    candidate only when strictly below it (so a NaN phi stays at b = 0 with d = NaN)."""
    phi = np.asarray(phi, f32).reshape(-1)
    elev = np.asarray(elev, f32).reshape(-1)
    with np.errstate(all='ignore'):
        best = np.zeros(phi.shape[0], np.int32)
        d = np.abs(phi - elev[0]).astype(f32)
        for b in range(1, elev.shape[0]):
            db = np.abs(phi - elev[b]).astype(f32)
            lower = db < d
            best = np.where(lower, np.int32(b), best)
            d = np.where(lower, db, d)
    return best, d.astype(f32)


def beam_search(phi, elev):
    """What the kernel does: lo = the number of table entries below phi by a branch-free binary search, the two neighbours
    lo - 1 and lo compared (the tie to the lower one), then a walk down a plateau.  fp32 subtraction is monotone, so d_b does not
    rise up to lo - 1 and does not fall from lo on: the smallest d is at one of the two, and entries that round to the SAME d sit
    directly below lo - 1 — the walk takes the first of them, which is the scan's tie rule.  -> (b int32, d fp32)."""
    phi = np.asarray(phi, f32).reshape(-1)
    elev = np.asarray(elev, f32).reshape(-1)
    B = elev.shape[0]
    with np.errstate(all='ignore'):
        lo = np.zeros(phi.shape[0], np.int64)
        step = 128
        while step >= 1:
            t = lo + step
            take = (t <= B) & (elev[np.minimum(t, B) - 1] < phi)
            lo = np.where(take, t, lo)
            step //= 2
        a, b = np.maximum(lo - 1, 0), np.minimum(lo, B - 1)
        da, db = np.abs(phi - elev[a]).astype(f32), np.abs(phi - elev[b]).astype(f32)
        low = da <= db
        best = np.where(low, a, b)
        d = np.where(low, da, db).astype(f32)
        while True:
            down = (best > 0) & (np.abs(phi - elev[np.maximum(best - 1, 0)]).astype(f32) == d)
            if not down.any():
                break
            best = np.where(down, best - 1, best)
    return best.astype(np.int32), d


def rows(xyz, cam):
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    cam = np.asarray(cam, f32).reshape(16)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(all='ignore'):
        c0 = cam[0] * x + cam[1] * y + cam[2] * z + cam[3] * f32(1)
        c1 = cam[4] * x + cam[5] * y + cam[6] * z + cam[7] * f32(1)
        c3 = cam[8] * x + cam[9] * y + cam[10] * z + cam[11] * f32(1)
    return c0.astype(f32), c1.astype(f32), c3.astype(f32)


def angles(xyz, cam):
    """-> (theta, phi, r) fp32 of every point."""
    c0, c1, c3 = rows(xyz, cam)
    with np.errstate(all='ignore'):
        q = c0 * c0 + c3 * c3
        rho = np.sqrt(q)
        theta = pm.atan2_model(c0, c3)
        phi = pm.atan2_model(c1, rho)
        r = np.sqrt(q + c1 * c1)
    return theta.astype(f32), phi.astype(f32), r.astype(f32)


def project(xyz, cam, elev, W, beam=beam_linear):
    """-> (cell or -1 (int32), range fp32: r where the point is accepted, 0.0 elsewhere)."""
    cam = np.asarray(cam, f32).reshape(16)
    elev = np.asarray(elev, f32).reshape(-1)
    theta, phi, r = angles(xyz, cam)
    with np.errstate(all='ignore'):
        nx = theta * cam[12]
        inside = (nx >= f32(-1)) & (nx <= f32(1))
        u = (f32(W) * (nx + f32(1))) * f32(0.5)
        col = np.where(inside, u, f32(0)).astype(np.int32)           # (int) truncates; only inside values are converted
        b, d = beam(phi, elev)
        ok = inside & (col >= 0) & (col < W) & (d <= cam[15]) & (cam[13] <= r) & (r <= cam[14])
    cell = np.where(ok, b.astype(np.int64) * W + col, -1).astype(np.int32)
    return cell, np.where(ok, r, f32(0)).astype(f32)


def project64(xyz, cam, elev, W):
    """The same formulas in float64 with arctan2 (the fp32 camera, table and points, exactly converted).
    -> dict of nx, u, phi, r, d (B smallest first two distances), b, col, ok, cell."""
    p = np.asarray(xyz, f32).astype(np.float64)
    c = np.asarray(cam, f32).reshape(16).astype(np.float64)
    e = np.asarray(elev, f32).astype(np.float64)
    h = np.concatenate([p, np.ones((p.shape[0], 1))], 1)
    with np.errstate(all='ignore'):
        c0, c1, c3 = h @ c[0:4], h @ c[4:8], h @ c[8:12]
        q = c0 * c0 + c3 * c3
        nx = np.arctan2(c0, c3) * c[12]
        phi = np.arctan2(c1, np.sqrt(q))
        r = np.sqrt(q + c1 * c1)
        inside = (nx >= -1) & (nx <= 1)
        u = W * (nx + 1) * 0.5
        col = np.where(inside, u, 0).astype(np.int64)
        # nearest and second nearest beam through the sorted table
        j = np.searchsorted(e, phi)
        a, bb = np.clip(j - 1, 0, e.size - 1), np.clip(j, 0, e.size - 1)
        da, db = np.abs(phi - e[a]), np.abs(phi - e[bb])
        low = da <= db
        b = np.where(low, a, bb)
        d1 = np.where(low, da, db)
        d2 = np.where(a == bb, np.inf, np.where(low, db, da))
        # the runner-up may also lie one further out on the winner's side
        o = np.where(low, a - 1, bb + 1)
        d2 = np.minimum(d2, np.where((o >= 0) & (o < e.size), np.abs(phi - e[np.clip(o, 0, e.size - 1)]), np.inf))
        ok = inside & (col >= 0) & (col < W) & (d1 <= c[15]) & (c[13] <= r) & (r <= c[14])
    return {'nx': nx, 'u': u, 'phi': phi, 'r': r, 'd1': d1, 'd2': d2, 'b': b, 'col': col, 'inside': inside, 'ok': ok,
            'cell': np.where(ok, b * W + col, -1)}


# ---- per cell -----------------------------------------------------------------------------------------------------------------
def key_image(xyz, cam, elev, W, ids=None, keys=None):
    """The B*W uint64 key image of one range of points under one camera, folded into ``keys`` when given."""
    B = np.asarray(elev).reshape(-1).shape[0]
    if keys is None:
        keys = np.full(B * W, EMPTY_KEY, np.uint64)
    xyz = np.asarray(xyz, f32).reshape(-1, 3)
    if xyz.shape[0] == 0:
        return keys
    ids = np.arange(xyz.shape[0], dtype=np.uint64) if ids is None else np.asarray(ids).astype(np.uint64)
    cell, r = project(xyz, cam, elev, W)
    ok = cell >= 0
    k = (r[ok].view(np.uint32).astype(np.uint64) << np.uint64(32)) | ids[ok]
    np.minimum.at(keys, cell[ok], k)
    return keys


def object_camera(cam, P):
    """The camera of an object placed by P: rows object_matrix(R4, P)[:3], the four scalars unchanged (as the panorama's)."""
    return pm.object_camera(cam, P)


def labelled_keys(xyz, labels, cam, elev, W, poses, hidden, extra=()):
    """Key image of a labelled cloud: label 0 under ``cam``, label k under object_camera(cam, poses.get(k)), hidden labels left
    out; ``extra`` = [(k, P)]: further copies of label k placed by P.  ids are the points' indices in the whole cloud."""
    xyz = np.asarray(xyz, f32)
    labels = np.asarray(labels)
    B = np.asarray(elev).reshape(-1).shape[0]
    keys = np.full(B * W, EMPTY_KEY, np.uint64)
    for k in np.unique(labels):
        if int(k) in hidden:
            continue
        sel = np.nonzero(labels == k)[0]
        key_image(xyz[sel], cam if k == 0 else object_camera(cam, poses.get(int(k))), elev, W, ids=sel, keys=keys)
    for k, P in extra:
        sel = np.nonzero(labels == k)[0]
        key_image(xyz[sel], object_camera(cam, P), elev, W, ids=sel, keys=keys)
    return keys


def scale_of(rel):
    return f32(1.0 + rel)


def see_through(keys, B, W, wb, wc, wrap, scale, slack):
    """The filtered key image (a new array)."""
    keys = np.asarray(keys, np.uint64).reshape(B, W)
    bits = (keys >> np.uint64(32)).astype(np.uint32)                 # EMPTY: 0xFFFFFFFF, above every range's bits
    near = bits.copy()
    for db in range(-wb, wb + 1):
        for dc in range(-wc, wc + 1):
            sh = np.full((B, W), np.uint32(0xFFFFFFFF), np.uint32)
            b0, b1 = max(0, -db), min(B, B - db)                       # rows b in [b0, b1) have b + db inside the table
            if b0 >= b1:
                continue
            src = bits[b0 + db:b1 + db]
            if wrap:
                sh[b0:b1] = np.roll(src, -dc, axis=1)
            else:
                c0, c1 = max(0, -dc), min(W, W - dc)
                if c0 < c1:
                    sh[b0:b1, c0:c1] = src[:, c0 + dc:c1 + dc]
            near = np.minimum(near, sh)
    has = keys != EMPTY_KEY
    with np.errstate(all='ignore'):
        lim = near.view(f32) * f32(scale) + f32(slack)
        keep = has & (bits.view(f32) <= lim)
    return np.where(keep, keys, EMPTY_KEY).reshape(-1)


def unpack(keys, B, W):
    """-> (range fp32 (B, W), idx int32 (B, W)); empty cells are (0.0, 0)."""
    idx, rng = pm.unpack(keys, W, B)
    return rng, idx


def returns(keys, elev, W, kx, capacity):
    """The return list of a (filtered) key image -> (count, cell int32 (m,), id int32 (m,), xyz fp32 (m, 3)), m = min(count,
    capacity)."""
    keys = np.asarray(keys, np.uint64).reshape(-1)
    cells = np.flatnonzero(keys != EMPTY_KEY)
    count = int(cells.size)
    cells = cells[:max(0, min(count, int(capacity)))]
    k = keys[cells]
    ids = (k & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    r = (k >> np.uint64(32)).astype(np.uint32).view(f32)
    bd, cd = beam_dir(elev), col_dir(W, kx)
    b, c = cells // W, cells % W
    with np.errstate(all='ignore'):
        h = r * bd[b, 0]
        xyz = np.stack([h * cd[c, 0], r * bd[b, 1], -(h * cd[c, 1])], 1).astype(f32)
    return count, cells.astype(np.int32), ids, xyz


def sweep(xyz, cam, elev, W, window=(0, 0), wrap=False, scale=1.0, slack=0.0, capacity=None, ids=None, keys=None):
    """One whole sweep -> dict(range, idx, count, cell, id, xyz, keys (filtered))."""
    elev = np.asarray(elev, f32).reshape(-1)
    B = elev.shape[0]
    if keys is None:
        keys = key_image(xyz, cam, elev, W, ids=ids)
    kept = see_through(keys, B, W, window[0], window[1], wrap, f32(scale), f32(slack))
    rng, idx = unpack(kept, B, W)
    count, cell, rid, pts = returns(kept, elev, W, np.asarray(cam, f32).reshape(16)[12], B * W if capacity is None else capacity)
    return {'range': rng, 'idx': idx, 'count': count, 'cell': cell, 'id': rid, 'xyz': pts, 'keys': kept}
