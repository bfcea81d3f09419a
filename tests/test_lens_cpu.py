"""CPU: the lens camera's contract (tests/lens_model.py) — the fp32 model against the same formulas in float64
and against an independent statement in OpenCV's axes, agreement with the pinhole where the lens is none, the limit, the
arctangent near the axis and behind the camera plane — and the C ABI of read_splat_forward_lens, read_splat_forward_lens_instances
and read_splat_lens_project_points (exported, bound as declared, refusing bad arguments before any device work).  Frames are
checked on the GPU (tests/test_gpu_lens.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle
from read_amd import _lib, camera
from tests import lens_cases as lc
from tests import lens_model as lm

f32 = np.float32


def _frac(x):
    return np.abs(x - np.round(x))


# ---- the camera ------------------------------------------------------------------------------------------------------------------
def test_lens_camera_layout():
    W, H = 512, 128
    P = lc.proj(W, H, 0.5)
    view = lc.pose(yaw=37.0, pitch=-8.0, roll=3.0, t=(1.5, -0.5, 2.0))
    k = (-0.28, 0.07, 0.0006, -0.0004, -0.008)
    cam = camera.lens_camera(P, view, 0, k, 1.5)
    assert cam.dtype == np.float32 and cam.shape == (32,)
    w2c = np.linalg.inv(view.astype(np.float64))
    p = np.array([3.0, 1.0, -7.0, 1.0])
    xc = w2c @ p
    assert np.allclose(cam[:12].reshape(3, 4).astype(np.float64) @ p, [xc[0], xc[1], -xc[2]], rtol=1e-6, atol=1e-6)    # unscaled
    assert tuple(cam[12:18]) == (P[0, 0], P[0, 2], P[1, 1], P[1, 2], P[2, 2], P[2, 3])
    assert cam[18] == f32(1.5) and cam[19] == 0.0 and np.array_equal(cam[20:25], np.asarray(k, f32)) and not cam[25:].any()
    fish = camera.lens_camera(P, view, 1, (0.01, -0.002))
    assert fish[19] == 1.0 and np.array_equal(fish[20:25], np.asarray((0.01, -0.002, 0, 0, 0), f32)) and np.array_equal(fish[:18], cam[:18])
    for model, coeffs in ((2, ()), (-1, ()), (0.5, ()), (0, (1, 2, 3, 4, 5, 6)), (1, (1, 2, 3, 4, 5)), (0, (np.nan,))):
        with pytest.raises(ValueError):
            camera.lens_camera(P, view, model, coeffs)


@pytest.mark.parametrize("model,coeffs", [(0, (-0.3,)), (0, (-0.28, 0.07, 0.0006, -0.0004, -0.008)), (0, (0.1, 0.01)), (0, ()),
                                          (1, (-0.03, 0.002, -0.0005, 0.00003)), (1, (-0.2,)), (1, (0.05, -0.03)), (1, ())])
def test_default_limit_and_stationary_point(model, coeffs):
    P, view = lc.proj(64, 48, 0.5), np.eye(4)
    got, want = camera.lens_stationary_point(model, coeffs), lm.stationary_point(model, coeffs)
    print(f"model {model} {coeffs}: stationary point {got} (root finder), {want} (bisection)")
    assert (got is None) == (want is None)
    cam = camera.lens_camera(P, view, model, coeffs)
    if got is None:
        assert cam[18] == (f32(np.inf) if model == 0 else f32(np.pi))
        if model == 1:
            with pytest.raises(ValueError, match="pi"):
                camera.lens_camera(P, view, 1, coeffs, 3.2)
        return
    assert abs(got - want) <= 1e-9 * want
    top = min(got, np.pi) if model == 1 else got
    assert cam[18] == (f32(np.pi) if top == np.pi else f32(0.999 * top))
    assert camera.lens_camera(P, view, model, coeffs, 0.5 * top)[18] == f32(0.5 * top)       # a smaller limit is the caller's
    assert float(camera.lens_camera(P, view, model, coeffs, top)[18]) <= top                 # the bound itself: never rounded over it
    with pytest.raises(ValueError, match="stationary point|pi"):
        camera.lens_camera(P, view, model, coeffs, top * 1.001)
    for bad in (-0.1, np.nan):
        with pytest.raises(ValueError):
            camera.lens_camera(P, view, model, coeffs, bad)


# ---- where the lens is none ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [True, False])
def test_zero_coefficients_model0_is_the_pinhole(exact):
    """Model 0 without coefficients is the pinhole of M = P @ inv(view): the same pixel except within 1e-3 px of a pixel boundary
    (the lens divides before it scales, the pinhole after).  Under a view whose entries are 0 and +-1 every row sum has one term
    and is exact, and then the depth is the pinhole's bit for bit: both compute fl(fl(P22 z_c) + P23) / -z_c.  Under a general
    view the pinhole rounds P22 into its matrix row before the sum and the lens multiplies the rounded sum, so the two depths are
    the same number rounded in two places: with |p|, |t| <= 60 m each four-term sum is off by <= 4 * 60 * 2^-24 = 1.4e-5 m, and
    d depth = (|zb| / 2 c3^2) d c3 <= 0.1 * 2.8e-5 = 2.8e-6 at c3 >= 1 m; the bound below is 4e-6 there."""
    W, H = 512, 128
    xyz = lc.ring_cloud(200_000, 5)
    view = np.round(lc.rot(1, 90.0)).astype(np.float32) if exact else \
        lc.pose(yaw=25.0, pitch=-6.0, roll=3.0, t=(0.7, 0.2, -1.1))
    P = lc.proj(W, H, 0.5)
    cam = camera.lens_camera(P, view, 0, ())
    assert cam[18] == np.inf
    M = camera.total_matrix(P, view)[0]
    pix_o, dep_o = oracle.project_points(xyz, M, W, H)
    pix_l, dep_l = lm.project(xyz, cam, W, H)
    ref = lm.project64(xyz, cam, W, H)
    with np.errstate(invalid='ignore'):
        clear = (_frac(ref['u']) > 1e-3) & (_frac(ref['v']) > 1e-3) & (np.abs(np.abs(ref['nx']) - 1) > 1e-5) & \
                (np.abs(np.abs(ref['ny']) - 1) > 1e-5) & (np.abs(np.abs(ref['nz']) - 1) > 1e-5)
    accepted = int((pix_o >= 0).sum())
    print(f"exact {exact}: accepted {accepted}, inside the margins {int((~clear & (pix_o >= 0)).sum())}, "
          f"differing pixels outside {int((pix_o[clear] != pix_l[clear]).sum())}")
    assert accepted > 20_000
    assert np.array_equal(pix_o[clear], pix_l[clear])
    both = (pix_o >= 0) & (pix_l >= 0)
    if exact:
        assert np.array_equal(dep_o[both].view(np.uint32), dep_l[both].view(np.uint32))
    else:
        far = both & (ref['nz'] > -1) & ((cam[8:12].astype(np.float64) * np.c_[xyz, np.ones(len(xyz))]).sum(1) >= 1.0)
        dd = float(np.abs(dep_o[far].astype(np.float64) - dep_l[far]).max())
        print(f"general view: max |depth - pinhole depth| at c3 >= 1 m = {dd:.2e}")
        assert far.sum() > 20_000 and dd <= 4e-6


def test_on_the_axis_model1_lands_on_the_principal_point():
    W, H = 512, 128
    P = lc.proj(W, H, 0.26)
    cam = camera.lens_camera(P, np.eye(4), 1, lc.LENSES["fisheye"][1], lc.LENSES["fisheye"][3])
    d = np.exp(np.random.default_rng(3).uniform(np.log(0.11), np.log(990.0), 5000)).astype(f32)
    xyz = np.zeros((5000, 3), f32)
    xyz[:, 2] = -d
    pix, dep = lm.project(xyz, cam, W, H)
    pp, _, _, _ = lm.tail(np.array([-cam[13]]), np.array([-cam[15]]), np.zeros(1, f32), W, H)
    assert (pix == pp[0]).all() and pp[0] >= 0                                  # rho = 0 is NOT rejected, unlike the panorama's
    pix_o, dep_o = oracle.project_points(xyz, camera.total_matrix(P, np.eye(4, dtype=np.float32))[0], W, H)
    assert np.array_equal(pix_o, pix) and np.array_equal(dep_o.view(np.uint32), dep.view(np.uint32))
    # the axis point behind the camera: theta = pi, kept only by a limit of pi, and then it too lands on the principal point
    back = np.array([[0, 0, 5.0]], f32)
    assert lm.project(back, cam, W, H)[0][0] == -1
    eq = camera.lens_camera(P, np.eye(4), 1, ())
    assert eq[18] == f32(np.pi) and lm.project(back, eq, W, H)[0][0] == pp[0]


# ---- against float64 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", ["brown", "fisheye", "equidistant"])
@pytest.mark.parametrize("W,H", [(64, 48), (512, 128), (1024, 352)])
def test_fp32_model_against_float64(W, H, lens):
    xyz = lc.ring_cloud(200_000, 5)
    cam = lc.lens_cam(lens, W, H, lc.pose(yaw=25.0, pitch=-6.0, roll=4.0, t=(0.7, 0.2, -1.1)))
    pix, _ = lm.project(xyz, cam, W, H)
    nx, ny, nz, _ = lm.ndc(xyz, cam)
    _, _, u, v = lm.tail(nx, ny, nz, W, H)
    ref = lm.project64(xyz, cam, W, H)
    with np.errstate(invalid='ignore'):
        clear = (_frac(ref['u']) > 1e-3) & (_frac(ref['v']) > 1e-3) & (np.abs(np.abs(ref['nx']) - 1) > 1e-5) & \
                (np.abs(np.abs(ref['ny']) - 1) > 1e-5) & (np.abs(np.abs(ref['nz']) - 1) > 1e-5) & \
                (np.abs(ref['r'] - float(cam[18])) > 1e-5)
    accepted = int(ref['ok'].sum())
    excluded = int((~clear & ref['ok']).sum())
    mism = int((pix[clear] != ref['pix'][clear]).sum())
    both = ref['ok'] & (pix >= 0)
    du = float(np.abs(u[both] - ref['u'][both]).max())
    print(f"{lens} {W}x{H}: accepted {accepted}, excluded {excluded} ({100.0 * excluded / accepted:.2f} %), mismatches {mism}, "
          f"max |u - U| = {du:.2e}")
    assert accepted > 20_000
    assert excluded <= 0.01 * accepted
    assert mism == 0


# ---- OpenCV's own axes -----------------------------------------------------------------------------------------------------------
def _opencv_pixels(xyz, view, K, model, coeffs):
    """cv::projectPoints / cv::fisheye::projectPoints as their documentation states them: camera axes X right, Y DOWN, Z forward,
    pixel units, float64.  -> (u, v) with v counted from the image top; only points with Z > 0 are meaningful."""
    fx, fy, cx, cy = K
    p = np.concatenate([np.asarray(xyz, np.float64), np.ones((len(xyz), 1))], 1) @ np.linalg.inv(np.asarray(view, np.float64)).T
    X, Y, Z = p[:, 0], -p[:, 1], -p[:, 2]                  # the GL camera looks down -z with y up
    x, y = X / Z, Y / Z
    r2 = x * x + y * y
    if model == 0:
        k1, k2, p1, p2, k3 = coeffs
        rad = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
        xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    else:
        k1, k2, k3, k4 = coeffs
        r = np.sqrt(r2)
        th = np.arctan(r)
        thd = th * (1 + k1 * th ** 2 + k2 * th ** 4 + k3 * th ** 6 + k4 * th ** 8)
        s = np.where(r == 0, 1.0, thd / np.where(r == 0, 1.0, r))
        xd, yd = x * s, y * s
    return fx * xd + cx, fy * yd + cy


@pytest.mark.parametrize("lens", ["brown", "fisheye"])
def test_opencv_axes(lens):
    """Pins the tangential signs and the K <-> P relation: u = fx x' + cx, v = fy y' + cy in OpenCV's frame."""
    W, H = 512, 128
    model, coeffs, fx_share, _ = lc.LENSES[lens]
    if model == 0:
        coeffs = (-0.28, 0.07, 0.02, -0.015, -0.008)       # tangential terms large enough that a wrong sign moves pixels
    view = lc.pose(yaw=25.0, pitch=-6.0, roll=4.0, t=(0.7, 0.2, -1.1))
    P = lc.proj(W, H, fx_share)
    cam = camera.lens_camera(P, view, model, coeffs)
    xyz = lc.ring_cloud(50_000, 9)
    ref = lm.project64(xyz, cam, W, H)
    view32 = np.linalg.inv(np.concatenate([cam[:12].reshape(3, 4).astype(np.float64) * [[1], [1], [-1]], [[0, 0, 0, 1]]], 0))
    u, v = _opencv_pixels(xyz, view32, lc.intrinsics(P, W, H), model, cam[20:25 if model == 0 else 24].astype(np.float64))
    ok = ref['ok'] & (np.c_[xyz, np.ones(len(xyz))] @ cam[8:12].astype(np.float64) > 0)      # OpenCV's form divides by Z
    assert ok.sum() > 5000
    assert np.abs(u[ok] - ref['u'][ok]).max() <= 1e-8 * W and np.abs(v[ok] - ref['v'][ok]).max() <= 1e-8 * W
    # and the signs matter: flipping p1 moves the image by more than a pixel somewhere
    if model == 0:
        flipped = lm.project64(xyz, camera.lens_camera(P, view, 0, (coeffs[0], coeffs[1], -coeffs[2], coeffs[3], coeffs[4])), W, H)
        assert np.abs(flipped['v'][ok] - ref['v'][ok]).max() > 1.0


# ---- the limit -------------------------------------------------------------------------------------------------------------------
def test_limit_keeps_inside_and_drops_outside():
    W, H = 512, 128
    for lens, at in (("fisheye", lambda t: (np.sin(t), 0.0, -np.cos(t))), ("brown", lambda r2: (np.sqrt(r2), 0.0, -1.0))):
        model, coeffs, fx_share, limit = lc.LENSES[lens]
        limit = 1.0 if limit is None else limit
        cam = camera.lens_camera(lc.proj(W, H, fx_share), np.eye(4), model, coeffs, limit)
        pts = 5.0 * np.array([at(limit - 1e-4), at(limit + 1e-4), at(0.5 * limit)], np.float64)
        pix, _ = lm.project(pts.astype(f32), cam, W, H)
        assert pix[0] >= 0 and pix[1] == -1 and pix[2] >= 0, (lens, pix)
        assert lens != "fisheye" or pts[0][2] > 0        # 100 degrees off the axis is behind the camera plane, and is drawn


def test_no_point_beyond_the_stationary_point_is_drawn():
    W, H = 256, 128
    model, coeffs, fx_share, _ = lc.FOLDING
    xyz = lc.ring_cloud(200_000, 6)
    view = lc.pose(yaw=-15.0, pitch=3.0)
    cam = camera.lens_camera(lc.proj(W, H, fx_share), view, model, coeffs)
    top = camera.lens_stationary_point(model, coeffs)
    assert top == pytest.approx(1.0 / 0.9, rel=1e-12) and cam[18] == f32(0.999 * top)
    pix, _ = lm.project(xyz, cam, W, H)
    r2 = lm.project64(xyz, cam, W, H)['r']
    assert (pix >= 0).sum() > 20_000 and r2[pix >= 0].max() <= top
    # what the limit is for: without it, points beyond the turn land inside the image again
    loose = cam.copy()
    loose[18] = np.inf
    folded = (lm.project(xyz, loose, W, H)[0] >= 0) & (r2 > top)
    print(f"folding lens: {int((pix >= 0).sum())} drawn, {int(folded.sum())} more would fold back into the image")
    assert folded.sum() > 1000


# ---- the arctangent where the fisheye uses it ------------------------------------------------------------------------------------
def test_atan2_near_the_axis_and_behind_the_plane():
    rng = np.random.default_rng(2)
    n = 2_000_000
    c3 = np.exp(rng.uniform(np.log(0.01), np.log(3000.0), n)).astype(f32)
    rho = (c3 * np.exp(rng.uniform(np.log(1e-8), 0.0, n))).astype(f32)
    rho = np.minimum(rho, c3)
    want = np.arctan2(rho.astype(np.float64), c3.astype(np.float64))
    rel = float((np.abs(lm.atan2_model(rho, c3).astype(np.float64) - want) / want).max())
    print(f"atan2_model(rho, c3), rho / c3 in [1e-8, 1]: max relative error {rel:.3e}")
    assert rel <= 2e-7
    rho = np.exp(rng.uniform(np.log(1e-6), np.log(3000.0), n)).astype(f32)
    c3 = -np.exp(rng.uniform(np.log(1e-6), np.log(3000.0), n)).astype(f32)
    err = float(np.abs(lm.atan2_model(rho, c3).astype(np.float64) - np.arctan2(rho.astype(np.float64), c3.astype(np.float64))).max())
    print(f"atan2_model(rho, c3), c3 < 0: max |error| {err:.3e} rad")
    assert err <= 4e-6
    th = lm.atan2_model(np.array([0.0, 0.0, 1.0, np.nan], f32), np.array([2.0, -2.0, 0.0, 1.0], f32))
    assert th[0] == 0 and th[1] == f32(np.pi) and th[2] == f32(np.pi / 2) and np.isnan(th[3])


def test_rejected_points():
    W, H = 256, 64
    inf, nan = np.inf, np.nan
    bad = np.array([[nan, 0, -1], [0, nan, -1], [0, 0, nan], [inf, 0, -1], [0, inf, -1], [0, 0, -inf], [-inf, inf, inf],
                    [0, 0, 0],                                       # the camera centre
                    [0, 0, -0.05], [0, 0, -2000]], f32)              # nearer than znear, beyond zfar
    for lens in ("brown", "fisheye", "equidistant"):
        cam = lc.lens_cam(lens, W, H, np.eye(4))
        assert (lm.project(bad, cam, W, H)[0] == -1).all(), lens
    # model 0 draws nothing at or behind the camera plane, whatever its limit
    cam = camera.lens_camera(lc.proj(W, H, 0.5), np.eye(4), 0, ())
    assert (lm.project(np.array([[1, 0, 0], [0.1, 0, 1], [0, 0, 1]], f32), cam, W, H)[0] == -1).all()


@pytest.mark.parametrize("lens", ["brown", "fisheye"])
def test_frame_model_pyramid_and_labels(lens):
    W, H = 64, 48
    xyz = lc.ring_cloud(20_000, 11, dup=500)
    cam = lc.lens_cam(lens, W, H, lc.pose(yaw=12.0, pitch=4.0, roll=-7.0, t=(0.3, 0.1, 0.2)))
    keys = lm.key_image(xyz, cam, W, H)
    idx0, _ = lm.unpack(keys, W, H)
    assert not np.isin(idx0, np.arange(19_500, 20_000)).any() and (keys != lm.EMPTY_KEY).sum() > 0.25 * W * H
    direct = lm.frame(xyz, cam, W, H, 5)
    reduced = lm.pyramid_of(keys, W, H, 5)
    for l in range(5):
        assert np.array_equal(direct[0][l], reduced[0][l]), f"index level {l}"
        assert np.array_equal(direct[1][l].view(np.uint32), reduced[1][l].view(np.uint32)), f"depth level {l}"
    labels = lc.labels_for(20_000, 3)
    poses = {1: lc.translation((2.0, 0.5, -1.0)), 3: (lc.rot(1, 30.0) @ lc.translation((0.0, 0.0, 4.0))).astype(f32)}
    assert np.array_equal(lm.labelled_keys(xyz, labels, cam, {}, set(), W, H), keys)         # identity poses: the unlabelled frame
    moved = lm.labelled_keys(xyz, labels, cam, poses, set(), W, H)
    assert not np.array_equal(moved, keys)
    hid = lm.labelled_keys(xyz, labels, cam, poses, {1}, W, H)
    assert not np.isin((hid[hid != lm.EMPTY_KEY] & np.uint64(0xFFFFFFFF)).astype(np.int64), np.flatnonzero(labels == 1)).any()
    oc = lm.object_camera(cam, poses[1])
    x = np.array([1.0, 2.0, -3.0, 1.0])
    assert np.allclose(oc[:12].reshape(3, 4) @ x, cam[:12].reshape(3, 4) @ (poses[1] @ x), atol=1e-4) and np.array_equal(oc[12:], cam[12:])


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------
FAKE = 1 << 20          # a 256-byte aligned non-null address: the calls below fail on their arguments and never touch it
NEW = ("read_splat_forward_lens", "read_splat_forward_lens_instances", "read_splat_lens_project_points")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ctype(decl):
    decl = decl.strip()
    if decl.startswith("const float *cam_host"):
        return C.POINTER(C.c_float)
    if "*const *" in decl:
        return C.POINTER(C.c_void_p)
    if "*" in decl:
        return C.c_void_p
    return {"int": C.c_int, "int64_t": C.c_int64, "size_t": C.c_size_t}[decl.rsplit(" ", 1)[0]]


def test_symbols_are_exported_and_bound_as_declared():
    L = C.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(ROOT, "include", "read_hip.h")).read()
    for name in NEW:
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
        m = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert m, f"{name} is not declared"
        want = [_ctype(a) for a in m.group(1).replace("\n", " ").split(",")]
        assert _lib.SIGNATURES[name] == (C.c_int, want), name
    assert _lib.lib().read_abi_version() == 3


def _cam(lens="fisheye"):
    return lc.lens_cam(lens, 64, 48, np.eye(4))


def _objs(begin, n=None, visible=None):
    begin = np.asarray(begin, np.int64)
    count = len(begin) - 1
    Ms = np.tile(_cam()[:16], (max(count, 1), 1))
    vis = None if visible is None else np.asarray(visible, np.uint8)
    s = _lib.SplatObjects(FAKE, FAKE, int(begin[-1]) if n is None else n, count, begin.ctypes.data, Ms.ctypes.data,
                          None if vis is None else vis.ctypes.data)
    s.keep = (begin, Ms, vis)
    return s


def _inst(first, npts, n=100, visible=None):
    first, npts = np.asarray(first, np.int64), np.asarray(npts, np.int64)
    Ms = np.tile(_cam()[:16], (max(len(first), 1), 1))
    vis = None if visible is None else np.asarray(visible, np.uint8)
    s = _lib.SplatInstances(FAKE, FAKE, n, len(first), first.ctypes.data, npts.ctypes.data, Ms.ctypes.data,
                            None if vis is None else vis.ctypes.data)
    s.keep = (first, npts, Ms, vis)
    return s


def _forward(cam=None, W=64, H=48, levels=5, xyz=FAKE, ids=None, n=100, ws=FAKE, outs=True, objs=None, inst=None, cam_null=False,
             ws_bytes=1 << 40):
    L = _lib.lib()
    cam = _cam() if cam is None else np.ascontiguousarray(cam, f32)
    idx = _lib.ptr_array([FAKE] * min(levels, 5)) if outs else None
    cp = None if cam_null else cam.ctypes.data_as(C.POINTER(C.c_float))
    if inst is not None:
        rc = L.read_splat_forward_lens_instances(xyz, ids, n, cp, W, H, levels, C.byref(inst) if inst != "null" else None, idx, None,
                                                 ws, ws_bytes, None)
    else:
        rc = L.read_splat_forward_lens(xyz, ids, n, cp, W, H, levels, None if objs is None else C.byref(objs), idx, None, ws,
                                       ws_bytes, None)
    return rc, L.read_last_error().decode()


@pytest.mark.parametrize("case", ["cam", "ws", "outputs", "xyz", "obj_begin", "obj_M", "obj_xyz", "obj_ids", "inst", "inst_first",
                                  "inst_npts", "inst_M", "inst_xyz"])
def test_forward_lens_refuses_null_pointers(case):
    objs = inst = None
    if case.startswith("obj_"):
        objs = _objs([0, 10, 30])
        setattr(objs, case[4:], None)
    elif case == "inst":
        inst = "null"
    elif case.startswith("inst_"):
        inst = _inst([0, 10], [10, 20])
        setattr(inst, case[5:], None)
    rc, msg = _forward(cam_null=case == "cam", ws=None if case == "ws" else FAKE, outs=case != "outputs",
                       xyz=None if case == "xyz" else FAKE, objs=objs, inst=inst)
    assert rc == -22 and "read_splat_forward_lens" in msg, (case, msg)
    assert ("no outputs" in msg) if case == "outputs" else ("null" in msg), (case, msg)


@pytest.mark.parametrize("W,H,levels", [(64, 40, 5), (40, 64, 5), (65, 48, 2), (1216, 352, 6)])
def test_forward_lens_refuses_sizes_off_the_pyramid(W, H, levels):
    for inst in (None, _inst([0], [10])):
        rc, msg = _forward(W=W, H=H, levels=levels, inst=inst)
        assert rc == -22 and "read_splat_forward_lens" in msg, msg
        assert ("multiples of 2^(levels-1)" in msg) if levels <= 5 else ("levels" in msg), msg


def test_forward_lens_refuses_bad_cameras():
    for lens in ("brown", "fisheye"):
        for i in range(32):
            for bad in (np.nan, np.inf, -np.inf):
                cam = _cam(lens)
                cam[i] = bad
                rc, msg = _forward(cam=cam, ws_bytes=1024)
                if i == 18 and bad == np.inf and lens == "brown":            # model 0 may have no limit
                    assert rc == -12 and "workspace" in msg, msg
                    continue
                assert rc == -22 and "read_splat_forward_lens" in msg and "cam_host" in msg, (lens, i, bad, msg)
                assert ("limit" in msg) if i == 18 else ("not finite" in msg), (lens, i, bad, msg)
    for model in (2.0, -1.0, 0.5):
        cam = _cam()
        cam[19] = model
        rc, msg = _forward(cam=cam)
        assert rc == -22 and "model must be 0" in msg, (model, msg)
    for lens, limit in (("brown", -1.0), ("fisheye", -1e-6), ("fisheye", 3.2), ("fisheye", np.nextafter(f32(np.pi), f32(4)))):
        cam = _cam(lens)
        cam[18] = limit
        rc, msg = _forward(cam=cam)
        assert rc == -22 and "limit" in msg, (lens, limit, msg)
    # a range's rows are held to finiteness, its 4 trailing floats are ignored — unless the range is hidden or empty
    objs = _objs([0, 10, 30])
    objs.keep[1][1, 3] = np.nan
    rc, msg = _forward(objs=objs)
    assert rc == -22 and "object 1" in msg and "not finite" in msg, msg
    inst = _inst([0, 10], [10, 20])
    inst.keep[2][0, 11] = np.inf
    rc, msg = _forward(inst=inst)
    assert rc == -22 and "instance 0" in msg and "not finite" in msg, msg
    # what passes the camera checks stops at the workspace size: nothing is launched
    for cam in (_cam("brown"), _cam("fisheye"), _cam("equidistant"), camera.lens_camera(lc.proj(64, 48, 0.5), np.eye(4), 0, ())):
        rc, msg = _forward(cam=cam, ws_bytes=1024)
        assert rc == -12 and "workspace" in msg, msg
    objs = _objs([0, 10, 30], visible=[1, 0])
    objs.keep[1][1, 3] = np.nan
    objs.keep[1][0, 12:] = np.nan
    rc, msg = _forward(objs=objs, ws_bytes=1024)
    assert rc == -12 and "workspace" in msg, msg


def test_forward_lens_refuses_bad_ranges():
    rc, msg = _forward(objs=_objs([0, 10, 5, 30]))
    assert rc == -22 and "read_splat_forward_lens" in msg and "not monotone at 1" in msg, msg
    rc, msg = _forward(objs=_objs([0, 10, 30], n=31))
    assert rc == -22 and "begin[count] = 30 != objs->n = 31" in msg, msg
    rc, msg = _forward(objs=_objs([3, 10, 30]))
    assert rc == -22 and "begin[0]" in msg, msg
    rc, msg = _forward(n=-1)
    assert rc == -22 and "n out of range" in msg, msg
    rc, msg = _forward(inst=_inst([0, -1], [10, 5]))
    assert rc == -22 and "read_splat_forward_lens_instances" in msg and "instance 1" in msg and "negative" in msg, msg
    rc, msg = _forward(inst=_inst([0, 10], [10, -5]))
    assert rc == -22 and "instance 1" in msg and "negative" in msg, msg
    rc, msg = _forward(inst=_inst([0, 95], [10, 6]))
    assert rc == -22 and "first + npts = 95 + 6 > inst->n = 100" in msg, msg


def test_lens_project_points_refuses_bad_arguments():
    L = _lib.lib()
    cam = _cam()
    cp = cam.ctypes.data_as(C.POINTER(C.c_float))
    for args in ((None, 10, cp, 64, 48, FAKE), (FAKE, 10, cp, 64, 48, None), (FAKE, 10, None, 64, 48, FAKE), (FAKE, 10, cp, 0, 48, FAKE)):
        rc = L.read_splat_lens_project_points(args[0], args[1], args[2], args[3], args[4], args[5], None, None)
        assert rc == -22 and "read_splat_lens_project_points" in L.read_last_error().decode(), args
    cam[19] = 3.0
    rc = L.read_splat_lens_project_points(FAKE, 10, cp, 64, 48, FAKE, None, None)
    assert rc == -22 and "model" in L.read_last_error().decode()
    cam[19], cam[18] = 1.0, 3.5
    rc = L.read_splat_lens_project_points(FAKE, 10, cp, 64, 48, FAKE, None, None)
    assert rc == -22 and "limit" in L.read_last_error().decode()
    cam[18], cam[5] = 1.0, np.nan
    rc = L.read_splat_lens_project_points(FAKE, 10, cp, 64, 48, FAKE, None, None)
    assert rc == -22 and "not finite" in L.read_last_error().decode()
    assert L.read_splat_lens_project_points(None, 0, _cam().ctypes.data_as(C.POINTER(C.c_float)), 64, 48, None, None, None) == 0


# ---- Python: one camera per scene, refusals by name ------------------------------------------------------------------------------
def test_scene_lens_is_exclusive_and_refusals_by_name():
    from read_amd.raster import PointCloudRasterizer
    from read_amd.render import MultiscaleRender, Scene, StitchedScene
    xyz = lc.ring_cloud(100, 0)
    scene = Scene(xyz)
    with pytest.raises(ValueError, match="set_lens"):
        scene.lens_camera()
    for model, coeffs, limit in ((2, (), None), (0, (1, 2, 3, 4, 5, 6), None), (1, (), 3.5), (0, (-0.3,), 2.0)):
        with pytest.raises(ValueError):
            scene.set_lens(model, coeffs, limit)
    assert scene.lens is None
    P, view = lc.proj(64, 64, 0.26), lc.pose(yaw=10.0)
    scene.set_proj_matrix(P)
    scene.set_camera_view(view)
    model, coeffs, limit = lc.lens_args("fisheye")
    scene.set_lens(model, coeffs, limit)
    assert np.array_equal(scene.lens_camera(), camera.lens_camera(P, view, model, coeffs, limit))
    with pytest.raises(ValueError, match="set_panorama.*lens"):
        scene.set_panorama(180.0)
    scene.set_lens(None)
    scene.set_panorama(180.0)
    with pytest.raises(ValueError, match="set_lens.*panorama"):
        scene.set_lens(model, coeffs, limit)
    scene.set_panorama(None)
    scene.set_lens(model, coeffs, limit)
    fmt = "uv_1d_p1, uv_1d_p1_ds1, uv_1d_p1_ds2, uv_1d_p1_ds3"
    with pytest.raises(NotImplementedError, match="xyz_p1_ds1.*lens"):
        MultiscaleRender(scene, "uv_1d_p1, xyz_p1_ds1", (64, 64), out_buffer_location='torch').render()
    with pytest.raises(NotImplementedError, match="supersampling 2.*lens"):
        MultiscaleRender(scene, fmt, (64, 64), out_buffer_location='torch', supersampling=2).render()
    with pytest.raises(NotImplementedError, match="lens.*68x64"):
        MultiscaleRender(scene, fmt, (68, 64), out_buffer_location='torch').render()
    scene.set_point_discard(np.zeros(100, bool))
    with pytest.raises(NotImplementedError, match="augmentation.*lens"):
        MultiscaleRender(scene, fmt, (64, 64), out_buffer_location='torch').render()
    scene.set_point_discard(None)
    with pytest.raises(NotImplementedError, match="lens.*select_masks"):
        scene.select_masks([], [], (64, 64))
    with pytest.raises(NotImplementedError, match="lens.*annotate_frame"):
        scene.annotate_frame((64, 64))
    st = StitchedScene([Scene(xyz), Scene(xyz)])
    with pytest.raises(NotImplementedError, match="lens.*StitchedScene"):
        st.set_lens(model, coeffs)
    st.set_lens(None)
    st.scenes[1].set_lens(model, coeffs, limit)                                # set on a part behind the stitched scene's back
    with pytest.raises(NotImplementedError, match="lens.*StitchedScene"):
        MultiscaleRender(st, fmt, (64, 64), out_buffer_location='torch').render()
    r = PointCloudRasterizer.__new__(PointCloudRasterizer)
    r.labels = None
    with pytest.raises(NotImplementedError, match="render_gl.*lens"):
        r.render_gl(np.eye(4), 64, 64, lens=scene.lens_camera())
