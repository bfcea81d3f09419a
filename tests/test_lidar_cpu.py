"""CPU: the LiDAR sweep's contract (tests/lidar_model.py) — the fp32 model against the same formulas in float64,
the beam search against the linear definition, the seam, the see-through filter's properties, the return list — and the C ABI of
read_lidar_sweep / read_lidar_project_points (exported, bound, refusing bad arguments before any device work).  Sweeps are checked
on the GPU (tests/test_gpu_lidar.py)."""
import ctypes as C
import os

import numpy as np
import pytest

from read_amd import _lib, camera, lidar
from tests import lidar_cases as lc
from tests import lidar_model as lm
from tests import pano_model as pm

f32 = np.float32


# ---- the fp32 model against float64 ------------------------------------------------------------------------------------------------
# The margins are the issue's and follow atan2_model's bound of 4e-6 rad against arctan2 (tests/test_pano_cpu.py): a distance
# |phi - e_b| moves by at most that plus an ulp of phi, the difference of two distances by at most twice it — 2e-5 rad between
# the two nearest beams and 1e-5 rad round d = delta cover both; a column edge is set aside at 1e-3 column as in the panorama's
# comparison; |nx| = 1 and the two ends of the range gate at a relative 1e-5, some hundred fp32 ulps.  A candidate is a point the
# float64 formulas accept or miss by no more than a margin.
@pytest.mark.parametrize("name,elev,W,hfov,share", lc.ROWS, ids=[r[0] for r in lc.ROWS])
def test_fp32_model_against_float64(name, elev, W, hfov, share):
    n = 400_000
    xyz = lc.gauss_cloud(n, 17)
    cam = lc.sensor_cam(elev, hfov, share, view=lc.pose(yaw=25.0, t=(0.7, 0.2, -1.1)))
    cell, _ = lm.project(xyz, cam, elev, W)
    ref = lm.project64(xyz, cam, elev, W)
    delta, rmin, rmax = float(cam[15]), float(cam[13]), float(cam[14])
    with np.errstate(invalid='ignore'):
        near = (np.abs(ref['d2'] - ref['d1']) < 2e-5) | (np.abs(ref['d1'] - delta) < 1e-5) | \
               (np.abs(ref['u'] - np.round(ref['u'])) < 1e-3) | (np.abs(np.abs(ref['nx']) - 1) < 1e-5) | \
               (np.abs(ref['r'] - rmin) < 1e-5 * rmin) | (np.abs(ref['r'] - rmax) < 1e-5 * rmax)
        # a candidate: a point in the field and the range gate whose elevation is within reach of a beam
        cand = ref['inside'] & (ref['r'] >= rmin * (1 - 1e-5)) & (ref['r'] <= rmax * (1 + 1e-5)) & (ref['d1'] <= delta + 1e-5)
    clear = ~near
    mism_out = int((cell[clear] != ref['cell'][clear]).sum())
    mism_in = int((cell[near] != ref['cell'][near]).sum())
    share_in = float((near & cand).sum()) / float(cand.sum())
    print(f"{name}: W {W} hfov {hfov}: candidates {int(cand.sum())}, accepted {int(ref['ok'].sum())}, inside the margins "
          f"{100.0 * share_in:.2f} %, mismatches outside {mism_out}, inside {mism_in}")
    assert ref['ok'].sum() > 20_000
    assert mism_out == 0
    assert share_in <= 0.02


# ---- the beam: binary search + neighbours + plateau walk == the linear scan ---------------------------------------------------
def _adversarial_phi(elev):
    e = np.asarray(elev, f32)
    up = lambda x, k=1: x if k == 0 else up(np.nextafter(x, f32(np.inf)), k - 1)
    down = lambda x, k=1: x if k == 0 else down(np.nextafter(x, f32(-np.inf)), k - 1)
    mid = ((e[:-1].astype(np.float64) + e[1:].astype(np.float64)) / 2).astype(f32)
    vals = [e, up(e), down(e), up(e, 2), down(e, 2), mid, up(mid), down(mid), up(mid, 2), down(mid, 2),
            np.array([e[0] - 1, e[0] - 1e-3, e[-1] + 1e-3, e[-1] + 1, -np.pi / 2, np.pi / 2, 0.0, -0.0, np.nan, np.inf, -np.inf,
                      1e-30, -1e-30, 1e30], f32)]
    rng = np.random.default_rng(3)
    vals.append(rng.uniform(float(e[0]) - 0.1, float(e[-1]) + 0.1, 20_000).astype(f32))
    return np.concatenate([np.asarray(v, f32).reshape(-1) for v in vals])


TABLES = {r[0]: r[1] for r in lc.ROWS}
TABLES.update({
    "one beam": np.array([0.1], f32),
    "two beams": np.array([-0.2, 0.3], f32),
    # exact midpoints: entries k / 8 have midpoints that are fp32 numbers, so the tie (to the lower beam) is hit exactly
    "eighths": (np.arange(-8, 9) / 8.0).astype(f32),
    # entries far below phi = 1 round to the SAME distance (1 - 1e-10 = 1 - 2e-10 = 1 in fp32): the plateau the walk handles
    "plateau": np.array([1e-10, 2e-10, 3e-10, 1e-9, 3.0], f32),
    "plateau about zero": np.array([-3e-10, -2e-10, -1e-10, 0.0, 1e-10, 2e-10, 2.5], f32),
    "128 uniform": lc.uniform_table(128, -25.0, 15.0),
})


@pytest.mark.parametrize("t", list(TABLES))
def test_beam_search_equals_the_linear_definition(t):
    elev = TABLES[t]
    assert (np.diff(elev) > 0).all()
    phi = _adversarial_phi(elev) if elev.size > 1 else np.concatenate([_adversarial_phi(np.array([0.1, 0.2], f32)), elev])
    if t.startswith("plateau"):
        phi = np.concatenate([phi, np.array([1.0, 0.5, 2.0, -1.0, 1.5, 1.25], f32)])
    b_lin, d_lin = lm.beam_linear(phi, elev)
    b_bin, d_bin = lm.beam_search(phi, elev)
    assert np.array_equal(b_lin, b_bin), f"{int((b_lin != b_bin).sum())} beams differ"
    assert np.array_equal(d_lin.view(np.uint32), d_bin.view(np.uint32))
    # the definition itself against a plain loop, on a sample
    for i in range(0, phi.size, max(1, phi.size // 300)):
        with np.errstate(all='ignore'):
            d = np.abs(phi[i] - elev).astype(f32)
        want = 0
        for b in range(1, elev.size):
            if d[b] < d[want]:
                want = b
        assert b_lin[i] == want
    if t == "eighths":                                                           # midpoints tie, the lower beam wins
        mid = ((elev[:-1] + elev[1:]) / 2).astype(f32)
        b, d = lm.beam_search(mid, elev)
        assert np.array_equal(b, np.arange(16)) and np.all(d == f32(1 / 16))
    if t == "plateau":                                                           # phi = 1 is 1.0 from the first four entries
        b, d = lm.beam_search(np.array([1.0], f32), elev)
        assert b[0] == 0 and d[0] == f32(1.0)


def test_the_seam_and_rejected_points():
    elev = lc.uniform_table(17, -16.0, 16.0)
    W = 64
    cam = lc.sensor_cam(elev, 360.0, 0.5)
    # exactly backwards: theta = +pi falls on column W and is dropped; theta = -pi lands on column 0
    # (a -0.0 coordinate does not survive the row sum: c0 = -0 + 0 + 0 + 0 = +0, so -pi is reached from just left of the axis)
    pts = np.array([[0.0, 0, 5], [-1e-8, 0, 5], [-1e-6, 0, 5], [0, 0, -5], [5, 0, 0], [-5, 0, 0]], f32)
    theta, phi, r = lm.angles(pts, cam)
    assert theta[0] == pm.PI_F and theta[1] == -pm.PI_F and -pm.PI_F < theta[2] < -3.14159
    cell, rng = lm.project(pts, cam, elev, W)
    b0, d0 = lm.beam_linear(np.zeros(1, f32), elev)                              # elevation 0 is beam 8 itself
    assert int(b0[0]) == 8 and d0[0] == 0
    row = 8 * W
    assert cell.tolist() == [-1, row + 0, row + 0, row + W // 2, row + 3 * W // 4, row + W // 4]
    assert rng[0] == 0 and np.all(rng[1:] == f32(5))
    # the edge catalogue: the axis (elevation +-90 degrees: no beam), the origin, NaN / Inf, the range gate's ends
    cat = lc.edge_catalogue(cam)
    cell, rng = lm.project(cat, cam, elev, W)
    assert (cell[:4] == -1).all() and (cell[-8:] == -1).all() and (rng[cell < 0] == 0).all()
    rmin, rmax = cam[13], cam[14]
    on = lm.project(np.array([[0, 0, -float(rmin)], [0, 0, -float(rmax)]], f32), cam, elev, W)
    assert (on[0] >= 0).all() and on[1].tolist() == [float(rmin), float(rmax)]          # both ends are inclusive
    off = lm.project(np.array([[0, 0, -float(np.nextafter(rmin, f32(0)))], [0, 0, -float(np.nextafter(rmax, f32(np.inf)))]], f32),
                     cam, elev, W)
    assert (off[0] == -1).all()
    # a narrow field: |nx| > 1 is outside
    cam120 = lc.sensor_cam(elev, 120.0, 0.5)
    c, _ = lm.project(np.array([[0, 0, -5], [5, 0, -5], [5, 0, -2.5], [-5, 0, 5]], f32), cam120, elev, W)
    assert c[0] == row + W // 2 and c[1] >= 0 and c[2] == -1 and c[3] == -1


def test_lidar_camera_layout():
    view = lc.pose(yaw=37.0, pitch=-8.0, roll=3.0, t=(1.5, -0.5, 2.0))
    cam = camera.lidar_camera(view, 200.0, 0.7, 90.0, 0.003)
    assert cam.dtype == np.float32 and cam.shape == (16,)
    lens = camera.lens_camera(np.eye(4), view, 0, None)
    assert np.array_equal(cam[:12], lens[:12])                                   # the lens camera's rows
    assert cam[12] == f32(2.0 / np.deg2rad(200.0)) and cam[12] == camera.pano_camera(np.eye(4), view, 200.0)[12]
    assert (cam[13], cam[14], cam[15]) == (f32(0.7), f32(90.0), f32(0.003))
    assert camera.lidar_camera(view)[12] == f32(1.0 / np.pi)
    for kw in (dict(hfov_deg=0.0), dict(hfov_deg=361.0), dict(rmin=0.0), dict(rmin=-1.0), dict(rmin=5.0, rmax=4.0),
               dict(rmax=np.inf), dict(half_width=-1e-3), dict(half_width=np.nan)):
        with pytest.raises(ValueError):
            camera.lidar_camera(view, **kw)
    # the product's host tables are the model's
    elev = lc.nonuniform_table(128, -25.0, 15.0)
    assert np.array_equal(lidar.beam_table(elev).view(np.uint32), lm.beam_dir(elev).view(np.uint32))
    for W, kx in ((1, cam[12]), (7, cam[12]), (2048, f32(1.0 / np.pi))):
        assert np.array_equal(lidar.column_table(W, kx).view(np.uint32), lm.col_dir(W, kx).view(np.uint32))


# ---- the see-through filter -------------------------------------------------------------------------------------------------------
def _image(B, W, cells):
    """A key image from {(b, c): (range, id)}."""
    keys = np.full(B * W, lm.EMPTY_KEY, np.uint64)
    for (b, c), (r, i) in cells.items():
        keys[b * W + c] = (np.uint64(f32(r).view(np.uint32)) << np.uint64(32)) | np.uint64(i)
    return keys


def _kept(keys):
    return set(np.flatnonzero(keys != lm.EMPTY_KEY).tolist())


def test_filter_on_a_hand_built_image():
    """scale = 1 + 1 / 16 is exact in fp32, so "exactly on the limit" can be written down."""
    B, W = 4, 8
    cells = {(0, 0): (10.0, 1), (0, 7): (10.625, 2),     # neighbours only through the seam; 10.625 = 10 * 1.0625: on the limit
             (1, 3): (5.0, 3), (1, 4): (5.3125, 4),      # 5.3125 = 5 * 1.0625: on the limit, kept
             (1, 5): (5.5, 5),                           # within the limit of 5.3125 beside it; 5.0 is two columns away
             (2, 4): (30.0, 6),                          # a row under 5.0, a column off: seen through
             (3, 0): (20.0, 7), (3, 7): (22.0, 8),       # 22 > 21.25 through the seam
             (3, 3): (8.0, 9), (3, 5): (8.0, 10)}        # two rows under the 5 m returns
    keys = _image(B, W, cells)
    scale = lm.scale_of(0.0625)
    assert scale == f32(1.0625)
    at = lambda *bc: {b * W + c for b, c in bc}
    everything = _kept(keys)
    kept = lambda *a: _kept(lm.see_through(keys, B, W, *a))
    assert kept(0, 0, True, scale, 0.0) == everything                                          # a zero window keeps everything
    assert kept(1, 1, False, scale, 0.0) == everything - at((2, 4))
    assert kept(1, 1, True, scale, 0.0) == everything - at((2, 4), (3, 7))                      # (0, 7) is on the limit: kept
    assert kept(1, 1, True, scale, 1.0) == everything - at((2, 4))                              # slack lifts 22.0 back in
    assert kept(0, 1, True, scale, 0.0) == everything - at((3, 7))                              # rows beyond wb are not seen
    # two columns: (1, 5) now sees 5.0; (0, 7) sees 5.5 a row down; (3, 7) sees 8.0 without the seam
    assert kept(1, 2, False, scale, 0.0) == everything - at((0, 7), (1, 5), (2, 4), (3, 7))
    # two rows: the 8 m returns see the 5 m ones; (3, 7) and (0, 7) see nothing without the seam
    assert kept(2, 1, False, scale, 0.0) == everything - at((2, 4), (3, 3), (3, 5))
    # the input is never modified, and a kept cell keeps its whole key
    before = keys.copy()
    out = lm.see_through(keys, B, W, 4, 4, True, scale, 0.0)
    assert np.array_equal(keys, before) and np.all((out == keys) | (out == lm.EMPTY_KEY))
    # the window may be wider than the image (W = 2 < 2 * 4 + 1): a true modulo
    tiny = _image(1, 2, {(0, 0): (1.0, 1), (0, 1): (2.0, 2)})
    assert _kept(lm.see_through(tiny, 1, 2, 4, 4, True, scale, 0.0)) == {0}
    assert _kept(lm.see_through(tiny, 1, 2, 4, 0, True, scale, 0.0)) == {0, 1}


def _filter_loop(keys, B, W, wb, wc, wrap, scale, slack):
    """The rule cell by cell, as the kernel walks it."""
    keys = keys.reshape(B, W)
    out = np.full((B, W), lm.EMPTY_KEY, np.uint64)
    for b in range(B):
        for c in range(W):
            if keys[b, c] == lm.EMPTY_KEY:
                continue
            near = None
            for bb in range(max(b - wb, 0), min(b + wb, B - 1) + 1):
                for dc in range(-wc, wc + 1):
                    cc = c + dc
                    if wrap:
                        cc %= W
                    elif cc < 0 or cc >= W:
                        continue
                    if keys[bb, cc] != lm.EMPTY_KEY:
                        r = np.uint32(keys[bb, cc] >> np.uint64(32)).view(f32)
                        near = r if near is None or r < near else near
            r = np.uint32(keys[b, c] >> np.uint64(32)).view(f32)
            if r <= f32(f32(near * f32(scale)) + f32(slack)):
                out[b, c] = keys[b, c]
    return out.reshape(-1)


def test_filter_properties():
    elev = lc.uniform_table(16, -15.0, 15.0)
    B, W = 16, 96
    cam = lc.sensor_cam(elev, 360.0, 0.5, view=lc.pose(yaw=12.0, t=(0.3, 0.0, 0.2)))
    keys = lm.key_image(lc.street_cloud(30_000, 5, dup=300), cam, elev, W)
    assert (keys != lm.EMPTY_KEY).sum() > 0.3 * B * W
    for wb, wc, wrap in ((1, 2, True), (4, 4, False), (0, 3, True), (2, 0, False)):
        got = lm.see_through(keys, B, W, wb, wc, wrap, lm.scale_of(0.05), 0.0)
        assert np.array_equal(got, _filter_loop(keys, B, W, wb, wc, wrap, lm.scale_of(0.05), 0.0)), (wb, wc, wrap)
    assert np.array_equal(lm.see_through(keys, B, W, 0, 0, False, lm.scale_of(0.05), 0.0), keys)
    # the kept set grows with rel and with slack
    sets = [_kept(lm.see_through(keys, B, W, 1, 2, True, lm.scale_of(rel), slack))
            for rel, slack in ((0.0, 0.0), (0.05, 0.0), (0.05, 0.5), (0.5, 0.5), (0.5, 5.0))]
    assert all(a <= b for a, b in zip(sets, sets[1:])) and len(sets[0]) < len(sets[-1]) <= len(_kept(keys))
    assert len(sets[1]) < len(_kept(keys))                                       # the default filter does drop something here
    # wrap and clip differ only in the wc columns next to the seam
    for wc in (1, 2, 4):
        a = lm.see_through(keys, B, W, 1, wc, True, lm.scale_of(0.05), 0.0).reshape(B, W)
        b = lm.see_through(keys, B, W, 1, wc, False, lm.scale_of(0.05), 0.0).reshape(B, W)
        assert np.array_equal(a[:, wc:W - wc], b[:, wc:W - wc])
        assert _kept(a.reshape(-1)) <= _kept(b.reshape(-1))                      # wrapping only adds neighbours
    assert not np.array_equal(lm.see_through(keys, B, W, 1, 4, True, lm.scale_of(0.0), 0.0),
                              lm.see_through(keys, B, W, 1, 4, False, lm.scale_of(0.0), 0.0))


def test_return_list():
    elev = lc.nonuniform_table(24, -20.0, 10.0)
    B, W = 24, 80
    cam = lc.sensor_cam(elev, 200.0, 0.5, view=lc.pose(yaw=-30.0, pitch=2.0, t=(0.1, 0.2, 0.3)))
    xyz = lc.street_cloud(20_000, 6)
    full = lm.sweep(xyz, cam, elev, W, window=(1, 2), wrap=False, scale=lm.scale_of(0.05))
    count = full['count']
    assert count == int((full['keys'] != lm.EMPTY_KEY).sum()) > 150
    assert np.all(np.diff(full['cell']) > 0) and full['cell'].size == count                  # ascending cells, all of them
    assert np.array_equal(full['id'], full['idx'].reshape(-1)[full['cell']])
    r = full['range'].reshape(-1)[full['cell']]
    # xyz from the two tables, bit for bit, by a scalar loop
    bd, cd = lm.beam_dir(elev), lm.col_dir(W, cam[12])
    for j in range(0, count, 37):
        b, c = divmod(int(full['cell'][j]), W)
        h = f32(r[j] * bd[b, 0])
        want = np.array([f32(h * cd[c, 0]), f32(r[j] * bd[b, 1]), -f32(h * cd[c, 1])], f32)
        assert np.array_equal(full['xyz'][j].view(np.uint32), want.view(np.uint32))
    # a return lies along its beam at its range: close to the point that made it (within the cell's angular size)
    err = np.linalg.norm(full['xyz'].astype(np.float64) - (np.linalg.inv(lc.pose(yaw=-30.0, pitch=2.0, t=(0.1, 0.2, 0.3)).astype(np.float64))
                                                           @ np.c_[xyz[full['id']], np.ones(count)].T).T[:, :3], axis=1)
    assert np.all(err <= r * (np.deg2rad(200.0) / W + 2 * float(cam[15])) + 1e-3)
    assert np.allclose(np.linalg.norm(full['xyz'].astype(np.float64), axis=1), r, rtol=1e-6)
    # count goes beyond the capacity; the list is a prefix
    for cap in (0, 1, count - 1, count, count + 5):
        part = lm.sweep(xyz, cam, elev, W, window=(1, 2), wrap=False, scale=lm.scale_of(0.05), capacity=cap)
        m = min(cap, count)
        assert part['count'] == count and part['cell'].size == m and part['xyz'].shape == (m, 3)
        assert np.array_equal(part['cell'], full['cell'][:m]) and np.array_equal(part['id'], full['id'][:m])
        assert np.array_equal(part['xyz'].view(np.uint32), full['xyz'][:m].view(np.uint32))


def test_labelled_model():
    elev = lc.uniform_table(16, -15.0, 15.0)
    W, n = 64, 8000
    cam = lc.sensor_cam(elev, 360.0, 0.5)
    xyz = lc.street_cloud(n, 8)
    labels = lc.labels_for(n, 3)
    assert np.array_equal(lm.labelled_keys(xyz, labels, cam, elev, W, {}, set()), lm.key_image(xyz, cam, elev, W))
    moved = lm.labelled_keys(xyz, labels, cam, elev, W, {1: lc.translation((2.0, 0.5, -1.0))}, {2})
    ids = (moved[moved != lm.EMPTY_KEY] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert not np.isin(ids, np.flatnonzero(labels == 2)).any() and np.isin(ids, np.flatnonzero(labels == 1)).any()
    twice = lm.labelled_keys(xyz, labels, cam, elev, W, {}, set(), extra=[(3, lc.translation((0.0, 0.0, 6.0)))])
    assert np.all(twice <= lm.key_image(xyz, cam, elev, W)) and not np.array_equal(twice, lm.key_image(xyz, cam, elev, W))


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------
FAKE = 1 << 20          # a 256-byte aligned non-null address: the calls below fail on their arguments and never touch it
NEW = ("read_lidar_workspace_bytes", "read_lidar_workspace_init", "read_lidar_sweep", "read_lidar_project_points")
ELEV = lc.uniform_table(16, -15.0, 15.0)


def test_symbols_are_exported_and_declared():
    L = C.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "read_hip.h")).read()
    for name in NEW:
        assert hasattr(L, name) and name in _lib.SIGNATURES and f" {name}(" in hdr, name
    assert "typedef struct read_lidar_args" in hdr
    assert _lib.lib().read_abi_version() == 3
    # the workspace: two key images and the tile counts and offsets, rounded to 256 bytes; 0 for sizes the sweep refuses
    L = _lib.lib()
    assert L.read_lidar_workspace_bytes(64, 2048) == 2 * 64 * 2048 * 8 + 2 * 512 * 4
    assert L.read_lidar_workspace_bytes(1, 1) == 256
    assert L.read_lidar_workspace_bytes(0, 8) == 0 and L.read_lidar_workspace_bytes(129, 8) == 0 and L.read_lidar_workspace_bytes(128, 1 << 24) == 0


def _cam(**kw):
    return lc.sensor_cam(ELEV, kw.pop('hfov', 360.0), 0.5, **kw)


def _inst(first=(0, 10), npts=(10, 20), n=30, M=True, visible=None):
    first, npts = np.asarray(first, np.int64), np.asarray(npts, np.int64)
    Ms = np.tile(_cam(), (max(len(first), 1), 1)) if M else None
    vis = None if visible is None else np.asarray(visible, np.uint8)
    s = _lib.SplatInstances(FAKE, FAKE, n, len(first), first.ctypes.data, npts.ctypes.data, None if Ms is None else Ms.ctypes.data,
                            None if vis is None else vis.ctypes.data)
    s.keep = (first, npts, Ms, vis)
    return s


def _sweep(cam=None, elev=ELEV, B=None, W=64, inst=None, **kw):
    """read_lidar_sweep with sound arguments except for what ``kw`` overrides -> (rc, message)."""
    cam = _cam() if cam is None else np.ascontiguousarray(cam, f32)
    elev = None if elev is None else np.ascontiguousarray(elev, f32)
    a = dict(xyz=FAKE, ids=None, n=100, inst=None if inst is None else C.pointer(inst), cam_host=cam.ctypes.data,
             elev_host=None if elev is None else elev.ctypes.data, B=(0 if elev is None else elev.size) if B is None else B, W=W,
             beam_dir=FAKE, col_dir=FAKE, wb=1, wc=2, wrap=1, scale=1.05, slack=0.0, range=FAKE, idx=FAKE, count=FAKE, cell=FAKE,
             ret_id=FAKE, ret_xyz=FAKE, capacity=100, workspace=FAKE, workspace_bytes=1 << 40)
    a.update(kw)
    args = _lib.LidarArgs(**a)
    L = _lib.lib()
    rc = L.read_lidar_sweep(C.byref(args), None)
    return rc, L.read_last_error().decode()


def _refused(msg_part, **kw):
    rc, msg = _sweep(**kw)
    assert rc == -22 and "read_lidar_sweep" in msg and msg_part in msg, (kw, rc, msg)


def test_sweep_refuses_null_pointers():
    L = _lib.lib()
    assert L.read_lidar_sweep(None, None) == -22 and "read_lidar_sweep" in L.read_last_error().decode()
    _refused("null", xyz=None)
    _refused("null", cam_host=None)
    _refused("null", elev=None, B=16)
    _refused("null", workspace=None)
    _refused("beam_dir", beam_dir=None)
    _refused("col_dir", col_dir=None)
    for field in ("first", "npts", "M", "xyz", "ids"):
        inst = _inst()
        setattr(inst, field, None)
        _refused("null", inst=inst)
    # nothing to do for a pointer: no refusal on its account (the calls stop at the workspace size: nothing is launched)
    for kw in (dict(xyz=None, n=0), dict(beam_dir=None, col_dir=None, ret_xyz=None), dict(beam_dir=None, col_dir=None, capacity=0),
               dict(range=None, idx=None, count=None, cell=None, ret_id=None, ret_xyz=None)):
        rc, msg = _sweep(workspace_bytes=1024, **kw)
        assert rc == -12 and "workspace" in msg, (kw, msg)


def test_sweep_refuses_bad_sizes_and_tables():
    _refused("B = 0", elev=ELEV, B=0)
    _refused("B = 129", elev=np.arange(129, dtype=f32) * 1e-3, B=129)
    _refused("bad size", W=0)
    _refused("bad size", W=-5)
    _refused("bad size", elev=np.arange(128, dtype=f32) * 1e-3, W=1 << 24)
    for bad in (np.nan, np.inf, -np.inf):
        e = ELEV.copy()
        e[5] = bad
        _refused("elev_host[5] is not finite", elev=e)
    e = ELEV.copy()
    e[7] = e[6]
    _refused("not strictly ascending at 7", elev=e)
    _refused("not strictly ascending at 1", elev=ELEV[::-1].copy())
    # the largest table and a single beam pass (and stop at the workspace size)
    for e in (np.arange(128, dtype=f32) * 1e-3, np.array([0.0], f32)):
        rc, msg = _sweep(elev=e, workspace_bytes=128)
        assert rc == -12, msg


def test_sweep_refuses_bad_cameras():
    for i in range(16):
        for bad in (np.nan, np.inf, -np.inf):
            cam = _cam()
            cam[i] = bad
            _refused("not finite", cam=cam)
    for kx in (0.0, -1.0, f32(1.0 / np.pi) - f32(1e-7), 0.3):
        cam = _cam()
        cam[12] = kx
        _refused("1 / pi", cam=cam)
    for i, vals, part in ((13, (0.0, -1.0), "rmin"), (14, (0.4,), "rmax"), (15, (-1e-6,), "delta")):
        for v in vals:
            cam = _cam()
            cam[i] = v
            _refused(part, cam=cam)
    # rmax = rmin and delta = 0 are sound
    cam = _cam()
    cam[14], cam[15] = cam[13], 0.0
    assert _sweep(cam=cam, workspace_bytes=128)[0] == -12
    # a drawn instance's camera is held to finiteness; a hidden or empty one is not looked at
    inst = _inst()
    inst.keep[2][1, 3] = np.nan
    _refused("instance 1", inst=inst)
    inst = _inst(visible=[1, 0])
    inst.keep[2][1, 3] = np.nan
    assert _sweep(inst=inst, workspace_bytes=128)[0] == -12
    inst = _inst(npts=(10, 0))
    inst.keep[2][1, 3] = np.inf
    assert _sweep(inst=inst, workspace_bytes=128)[0] == -12


def test_sweep_refuses_bad_filters_capacity_workspace_and_lists():
    for kw in (dict(wb=-1), dict(wb=5), dict(wc=-1), dict(wc=5)):
        _refused("window", **kw)
    for s in (0.999, 0.0, -1.0, np.nan, np.inf):
        _refused("scale", scale=s)
    for s in (-1e-6, np.nan, np.inf):
        _refused("slack", slack=s)
    _refused("capacity", capacity=-1)
    _refused("n out of range", n=-1)
    _refused("aligned", workspace=FAKE + 8)
    need = _lib.lib().read_lidar_workspace_bytes(16, 64)
    rc, msg = _sweep(workspace_bytes=need - 1)
    assert rc == -12 and "read_lidar_sweep" in msg and f"{need - 1} < {need}" in msg, msg
    # a malformed instance list: the checks of read_splat_forward_pano_instances
    inst = _inst()
    inst.count = -1
    _refused("inst->count", inst=inst)
    _refused("negative", inst=_inst(first=(0, -1)))
    _refused("negative", inst=_inst(npts=(10, -2)))
    _refused("first + npts", inst=_inst(first=(0, 25), npts=(10, 6)))
    _refused("inst->n", inst=_inst(n=-1))


def test_project_points_refuses_bad_arguments():
    L = _lib.lib()
    cam, elev = _cam(), ELEV.copy()
    call = lambda xyz=FAKE, n=10, c=cam, e=elev, B=16, W=64, cell=FAKE: (
        L.read_lidar_project_points(xyz, n, None if c is None else c.ctypes.data, None if e is None else e.ctypes.data, B, W, cell, None, None),
        L.read_last_error().decode())
    for kw in (dict(xyz=None), dict(cell=None), dict(c=None), dict(e=None), dict(n=-1), dict(B=0), dict(B=129), dict(W=0)):
        rc, msg = call(**kw)
        assert rc == -22 and "read_lidar_project_points" in msg, (kw, msg)
    bad = elev.copy()
    bad[3] = bad[2]
    rc, msg = call(e=bad)
    assert rc == -22 and "ascending at 3" in msg
    for i, v, part in ((12, 0.1, "1 / pi"), (5, np.nan, "not finite"), (13, 0.0, "rmin"), (14, 0.1, "rmax"), (15, -1.0, "delta")):
        c = cam.copy()
        c[i] = v
        rc, msg = call(c=c)
        assert rc == -22 and part in msg, (i, msg)
    assert call(xyz=None, n=0, cell=None)[0] == 0                                # nothing to do


def test_refusals_by_name():
    from read_amd.render import Scene, StitchedScene
    xyz = lc.street_cloud(100, 0)
    st = StitchedScene([Scene(xyz), Scene(xyz)])
    with pytest.raises(NotImplementedError, match="lidar_sweep.*StitchedScene"):
        st.lidar_sweep(None)
    scene = Scene(xyz)
    scene.set_point_discard(np.zeros(100, bool))
    with pytest.raises(NotImplementedError, match="augmentation.*lidar_sweep"):
        scene.lidar_sweep(None)
    scene.set_point_discard(None)
    scene.set_point_sizes(np.ones(100, f32))
    with pytest.raises(NotImplementedError, match="augmentation.*lidar_sweep"):
        scene.lidar_sweep(None)
    with pytest.raises(ValueError, match="set_vertices"):
        Scene().lidar_sweep(None)
