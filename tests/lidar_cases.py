"""Sensors, clouds and poses the LiDAR tests share (tests/test_lidar_cpu.py, tests/test_gpu_lidar.py)."""
import numpy as np

from read_amd import camera
from tests import pano_cases as pc

f32 = np.float32


def uniform_table(B, lo_deg, hi_deg):
    """B fp32 elevations (radians) evenly spaced over [lo_deg, hi_deg]."""
    return np.deg2rad(np.linspace(lo_deg, hi_deg, B)).astype(f32)


def nonuniform_table(B, lo_deg, hi_deg, seed=0):
    """B fp32 elevations over [lo_deg, hi_deg] with random spacings between 0.7 and 1.3 (before normalisation).  The float64
    comparison accepts a point within delta = a share of the SMALLEST spacing of a beam and sets aside those within 1e-5 rad of
    d = delta, a share 2e-5 / (2 delta) of the accepted ones on either side: a table whose smallest spacing is far below its mean
    would spend the 2 % the comparison allows on that margin alone (128 beams over 40 degrees: mean 5.5e-3 rad)."""
    rng = np.random.default_rng(seed)
    steps = rng.uniform(0.7, 1.3, B - 1)
    e = lo_deg + np.concatenate([[0.0], np.cumsum(steps)]) / steps.sum() * (hi_deg - lo_deg)
    return np.deg2rad(e).astype(f32)


def spacing(elev):
    return float(np.diff(np.asarray(elev, np.float64)).min())


# (name, table, W, hfov, delta as a share of the smallest spacing): the four rows of the float64 comparison
ROWS = [
    ("64 uniform", uniform_table(64, -24.8, 2.0), 2048, 360.0, 0.5),
    ("16 uniform", uniform_table(16, -15.0, 15.0), 512, 360.0, 0.25),
    ("128 non-uniform", nonuniform_table(128, -25.0, 15.0), 4096, 360.0, 0.5),
    ("32 at 120 degrees", uniform_table(32, -10.0, 10.0), 1024, 120.0, 0.4),
]


def sensor_cam(elev, hfov, share, view=None, rmin=0.5, rmax=120.0):
    """camera.lidar_camera with delta = share of the table's smallest spacing (a single beam: share is delta in radians)."""
    elev = np.asarray(elev)
    delta = share * spacing(elev) if elev.size > 1 else share
    return camera.lidar_camera(np.eye(4) if view is None else view, hfov, rmin, rmax, delta)


def gauss_cloud(n, seed, sigma=(30.0, 3.0, 30.0)):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, 3)) * np.asarray(sigma)).astype(f32)


def street_cloud(n, seed, dup=0):
    """A cloud a sweep fills well: a ground plane 1.8 m under the origin, walls to both sides and scattered clutter, the last
    ``dup`` points exact copies of earlier ones (ties)."""
    rng = np.random.default_rng(seed)
    m = n - dup
    xyz = np.empty((n, 3), f32)
    g, w = int(0.6 * m), int(0.36 * m)
    xyz[:g] = np.stack([rng.uniform(-40, 40, g), np.full(g, -1.8) + rng.normal(0, 0.02, g), rng.uniform(-40, 40, g)], 1)
    side = rng.choice([-1.0, 1.0], w)
    xyz[g:g + w] = np.stack([side * (9.0 + rng.normal(0, 0.05, w)), rng.uniform(-1.8, 6.0, w), rng.uniform(-40, 40, w)], 1)
    c = m - g - w
    xyz[g + w:m] = np.stack([rng.uniform(-30, 30, c), rng.uniform(-1.8, 3.0, c), rng.uniform(-30, 30, c)], 1)
    if dup:
        xyz[m:] = xyz[rng.choice(m, dup, replace=False)]
    return xyz


def edge_catalogue(cam):
    """Points in the SENSOR frame of an upright sensor at the origin (view = identity) that sit on the contract's edges: the axis
    rho = 0, the plane c1 = 0, ranges on rmin / rmax and one ulp either side, exactly backwards (theta = +-pi), NaN / Inf
    coordinates, and points 10^5 apart in scale."""
    rmin, rmax = float(cam[13]), float(cam[14])
    pts = [[0, 0, 0], [0, 5, 0], [0, -5, 0], [0, 1e-3, 0],                                    # the axis
           [3, 0, -4], [-3, 0, -4], [0, 0, -7], [1, 0, 0], [-1, 0, 0],                         # c1 = 0
           [0, 0, 5], [-0.0, 0, 5], [1e-6, 0, 5], [-1e-6, 0, 5]]                               # backwards: theta = +pi / -pi
    for r in (rmin, rmax):
        for rr in (np.nextafter(f32(r), f32(0)), f32(r), np.nextafter(f32(r), f32(np.inf))):
            pts += [[0, 0, -float(rr)], [float(rr), 0, 0], [0.6 * float(rr), 0, -0.8 * float(rr)]]
    for s in (1e-5, 1e-3, 1.0, 1e2, 1e5):
        pts += [[0.3 * s, -0.05 * s, -0.9 * s], [-0.7 * s, 0.02 * s, 0.2 * s]]
    inf, nan = np.inf, np.nan
    pts += [[nan, 0, -1], [0, nan, -1], [0, 0, nan], [inf, 0, -1], [0, inf, -1], [0, 0, -inf], [-inf, inf, inf], [nan, nan, nan]]
    return np.array(pts, f32)


pose, rot, translation, labels_for = pc.pose, pc.rot, pc.translation, pc.labels_for
