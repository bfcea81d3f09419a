"""CPU: the panorama camera's contract (tests/pano_model.py) — the arctangent's accuracy, the fp32 model against
the same formulas in float64, agreement with the pinhole at the image centre, the pyramid and label identities of the frame model —
and the C ABI of read_splat_forward_pano / read_splat_pano_project_points (exported, bound, refusing bad arguments before any
device work).  Frames are checked on the GPU (tests/test_gpu_pano.py)."""
import ctypes as C

import numpy as np
import pytest

import oracle
from read_amd import _lib, camera
from tests import pano_cases as pc
from tests import pano_model as pm

ATAN_BOUND = 4e-6           # rad: 0.005 pixel at W = 8192 over 360 degrees


def _atan_err(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(pm.atan2_model(a, b).astype(np.float64) - np.arctan2(a.astype(np.float64), b.astype(np.float64)))


def test_atan2_model_accuracy():
    rng = np.random.default_rng(0)
    n = 2_000_000
    a, b = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    err = _atan_err(a, b).max()
    print(f"atan2_model: max |error| over {n} random pairs = {err:.3e} rad")
    assert err <= ATAN_BOUND
    # axes, both diagonals, every sign
    one = np.float32(1)
    spec = [(s * x, t * y) for x, y in ((0, 1), (1, 0), (1, 1), (3, 3), (1e-30, 1e-30), (1e30, 1e30)) for s in (1, -1) for t in (1, -1)]
    # a zero of either sign against a non-zero operand, and (+-0, +0)
    spec += [(z, y) for z in (0.0, -0.0) for y in (1.0, -1.0, 1e-38, -1e-38, 1e38, -1e38)]
    spec += [(y, z) for z in (0.0, -0.0) for y in (1.0, -1.0, 1e-38, -1e-38, 1e38, -1e38)]
    spec += [(0.0, 0.0), (-0.0, 0.0)]
    # operands 2^-100 .. 2^100 apart, in every quadrant
    for e in range(-100, 101):
        for s in (1, -1):
            for t in (1, -1):
                spec.append((s * 2.0 ** e, t * 1.0))
                spec.append((s * 2.0 ** (e / 2 if e % 2 == 0 else 0), t * 2.0 ** (-e / 2 if e % 2 == 0 else 0)))
    sa, sb = np.array([p[0] for p in spec], np.float32), np.array([p[1] for p in spec], np.float32)
    got, want = pm.atan2_model(sa, sb), np.arctan2(sa.astype(np.float64), sb.astype(np.float64))
    assert np.abs(got - want).max() <= ATAN_BOUND
    assert np.array_equal(np.signbit(got), np.signbit(want))                    # the sign of a zero result included
    assert float(pm.atan2_model(one, one)) == pytest.approx(np.pi / 4, abs=ATAN_BOUND)
    # exactly backwards: +pi for c0 = +0, -pi for c0 = -0 (the model's step 8 then 9)
    assert pm.atan2_model(np.float32(0.0), np.float32(-2.0)) == pm.PI_F and pm.atan2_model(np.float32(-0.0), np.float32(-2.0)) == -pm.PI_F
    # (+-0, -0): the model tests b < 0, so a negative ZERO is not "behind" and the result is +-0 where arctan2 says +-pi; such a
    # point has rho = 0 and is rejected whatever the angle (test_rejected_points)
    z = pm.atan2_model(np.float32([0.0, -0.0]), np.float32([-0.0, -0.0]))
    assert np.array_equal(z, np.float32([0.0, -0.0])) and np.array_equal(np.signbit(z), [False, True])
    # NaN in, NaN out (compare-and-select, so NumPy and the device agree)
    assert np.isnan(pm.atan2_model(np.float32([np.nan, 1.0, np.nan]), np.float32([1.0, np.nan, np.nan]))).all()


def test_coefficients_are_fp32_literals():
    assert len(pm.ATAN_COEFFS) == 8 and all(np.asarray(c).dtype == np.float32 for c in pm.ATAN_COEFFS)
    assert pm.ATAN_COEFF_BITS == (0x3b3bd74a, 0xbc846e02, 0x3d2fc1fe, 0xbd9a3174, 0x3dda3d83, 0xbe117fc7, 0x3e4cbbe5, 0xbeaaaa6c)
    assert int(pm.PI_F.view(np.uint32)) == 0x40490fdb and int(pm.HALF_PI_F.view(np.uint32)) == 0x3fc90fdb


def test_pano_camera_layout():
    W, H = 512, 128
    P = pc.proj(W, H)
    view = pc.pose(yaw=37.0, pitch=-8.0, roll=3.0, t=(1.5, -0.5, 2.0))
    cam = camera.pano_camera(P, view, 200.0)
    assert cam.dtype == np.float32 and cam.shape == (16,)
    w2c = np.linalg.inv(view.astype(np.float64))
    p = np.array([3.0, 1.0, -7.0, 1.0])
    xc = w2c @ p
    rows = cam[:12].reshape(3, 4).astype(np.float64) @ p
    assert np.allclose(rows, [xc[0], float(P[1, 1]) * xc[1], -xc[2]], rtol=1e-6, atol=1e-6)
    assert cam[12] == np.float32(2.0 / np.deg2rad(200.0))
    assert (cam[13], cam[14], cam[15]) == (P[1, 2], P[2, 2], P[2, 3])
    # P[0,0] and P[0,2] are ignored
    P2 = P.copy()
    P2[0, 0], P2[0, 2] = 9.0, -0.4
    assert np.array_equal(camera.pano_camera(P2, view, 200.0), cam)
    # 360 degrees is the largest field and passes the library's kx >= 1 / pi check (test_forward_pano_refuses_bad_cameras)
    assert camera.pano_camera(P, view, 360.0)[12] == np.float32(1.0 / np.pi)
    for bad in (0.0, -10.0, 360.5, float('nan')):
        with pytest.raises(ValueError):
            camera.pano_camera(P, view, bad)


@pytest.mark.parametrize("W,H,hfov", [(512, 128, 360.0), (256, 64, 200.0), (1024, 64, 360.0)])
def test_fp32_model_against_float64(W, H, hfov):
    xyz = pc.ring_cloud(200_000, 5)
    cam = camera.pano_camera(pc.proj(W, H), pc.pose(yaw=25.0, pitch=-6.0, t=(0.7, 0.2, -1.1)), hfov)
    pix, _ = pm.project(xyz, cam, W, H)
    nx, ny, nz = pm.ndc(xyz, cam)
    _, _, u, v = pm.tail(nx, ny, nz, W, H)
    ref = pm.project64(xyz, cam, W, H)
    frac = lambda x: np.abs(x - np.round(x))
    with np.errstate(invalid='ignore'):
        clear = (frac(ref['u']) > 1e-3) & (frac(ref['v']) > 1e-3) & (np.abs(np.abs(ref['nx']) - 1) > 1e-5) & \
                (np.abs(np.abs(ref['ny']) - 1) > 1e-5)
    accepted = int(ref['ok'].sum())
    excluded = int((~clear & ref['ok']).sum())
    mism = int((pix[clear] != ref['pix'][clear]).sum())
    both = ref['ok'] & (pix >= 0)
    du = float(np.abs(u[both] - ref['u'][both]).max())
    print(f"{W}x{H} hfov {hfov}: accepted {accepted}, excluded {excluded} ({100.0 * excluded / accepted:.2f} %), mismatches {mism}, "
          f"max |u - U| = {du:.2e}")
    assert accepted > 20_000
    assert excluded <= 0.01 * accepted
    assert mism == 0


@pytest.mark.parametrize("yaw", [0, 90, 180])
def test_centre_column_is_the_pinhole(yaw):
    """c0 = 0: rho = |c3| exactly, so depth is the pinhole's bit for bit; so is the row when P[1,2] = 0 (then both compute
    fl(P11 y) / rho), and with P[1,2] != 0 the pinhole divides fl(fl(P11 y) + fl(P12 z)) where the panorama subtracts ky after
    the division — the same number rounded in two places, equal as a ROW away from row boundaries (1e-3 px, as above)."""
    W, H = 512, 128
    rng = np.random.default_rng(7)
    n = 20_000
    local = np.zeros((n, 4))
    local[:, 1] = rng.uniform(-30, 30, n)
    local[:, 2] = -np.exp(rng.uniform(np.log(0.05), np.log(2000.0), n))           # in front, beyond both clip planes too
    local[:, 3] = 1
    view = pc.rot(1, yaw)                                                        # entries 0 / +-1: every product below is exact
    view = np.round(view).astype(np.float32)
    xyz = (local @ view.astype(np.float64).T)[:, :3].astype(np.float32)
    for cy_shift in (0.0, 0.03):
        P = pc.proj(W, H, cy_shift=cy_shift)
        cam = camera.pano_camera(P, view, 360.0)
        M = camera.total_matrix(P, view)[0]
        pix_o, dep_o = oracle.project_points(xyz, M, W, H)
        pix_p, dep_p = pm.project(xyz, cam, W, H)
        nx, ny, nz = pm.ndc(xyz, cam)
        assert np.all(nx == 0)
        ok_o, ok_p = pix_o >= 0, pix_p >= 0
        if cy_shift == 0.0:
            assert P[1, 2] == 0
            assert np.array_equal(ok_o, ok_p)
            assert np.array_equal(pix_o[ok_o] // W, pix_p[ok_p] // W)
            assert np.all(pix_p[ok_p] % W == W // 2)
            sel = ok_o
        else:
            v64 = pm.project64(xyz, cam, W, H)
            with np.errstate(invalid='ignore'):
                clear = (np.abs(v64['v'] - np.round(v64['v'])) > 1e-3) & (np.abs(np.abs(v64['ny']) - 1) > 1e-5)
            assert np.array_equal(ok_o[clear], ok_p[clear])
            sel = ok_o & ok_p
            assert np.array_equal((pix_o[sel & clear] // W), (pix_p[sel & clear] // W))
        assert sel.sum() > 5000
        assert np.array_equal(dep_o[sel].view(np.uint32), dep_p[sel].view(np.uint32))


def test_rejected_points():
    W, H = 256, 64
    cam = camera.pano_camera(pc.proj(W, H), np.eye(4), 360.0)
    inf, nan = np.inf, np.nan
    pts = np.array([[0, 0, 0], [0, 5, 0], [0, -5, 0],                # rho = 0: the camera's vertical axis
                    [nan, 0, -1], [0, nan, -1], [0, 0, nan], [inf, 0, -1], [0, inf, -1], [0, 0, -inf], [-inf, inf, inf],
                    [0, 0, 1],                                       # exactly backwards: theta = +pi -> column W
                    [0, 0, -0.05], [0, 0, -2000]], np.float32)       # nearer than znear, beyond zfar
    pix, _ = pm.project(pts, cam, W, H)
    assert (pix == -1).all()
    pix, _ = pm.project(np.array([[0, 0, -1], [-1e-5, 0, 1], [1, 0, 0], [-1, 0, 0]], np.float32), cam, W, H)
    row = pix[0] // W
    assert pix.tolist() == [row * W + W // 2, row * W + 0, row * W + 3 * W // 4, row * W + W // 4]


@pytest.mark.parametrize("W,H", [(96, 48), (256, 64)])
def test_frame_model_pyramid_and_labels(W, H):
    xyz = pc.ring_cloud(20_000, 11, dup=500)
    cam = camera.pano_camera(pc.proj(W, H), pc.pose(yaw=12.0, pitch=4.0, roll=-7.0, t=(0.3, 0.1, 0.2)), 360.0)
    keys = pm.key_image(xyz, cam, W, H)
    # the duplicates tie exactly and the smaller id wins
    idx0, _ = pm.unpack(keys, W, H)
    assert not np.isin(idx0, np.arange(19_500, 20_000)).any() and (keys != pm.EMPTY_KEY).sum() > 0.25 * W * H
    direct = pm.frame(xyz, cam, W, H, 5)
    reduced = pm.pyramid_of(keys, W, H, 5)
    for l in range(5):
        assert np.array_equal(direct[0][l], reduced[0][l]), f"index level {l}"
        assert np.array_equal(direct[1][l].view(np.uint32), reduced[1][l].view(np.uint32)), f"depth level {l}"
    # labels: the whole-cloud model equals the merge of the per-label models under object_matrix cameras
    labels = pc.labels_for(20_000, 3)
    poses = {1: pc.translation((2.0, 0.5, -1.0)), 2: None, 3: (pc.rot(1, 30.0) @ pc.translation((0.0, 0.0, 4.0))).astype(np.float32)}
    merged = np.full(W * H, pm.EMPTY_KEY, np.uint64)
    for k in range(4):
        sel = np.flatnonzero(labels == k)
        ck = cam if k == 0 else pm.object_camera(cam, poses[k])
        part = pm.key_image(xyz[sel], ck, W, H)                                  # local ids
        glob = np.where(part == pm.EMPTY_KEY, pm.EMPTY_KEY,
                        (part & np.uint64(0xFFFFFFFF00000000)) | sel[(part & np.uint64(0xFFFFFFFF)).astype(np.int64) % sel.size].astype(np.uint64))
        merged = np.minimum(merged, glob)
    assert np.array_equal(pm.labelled_keys(xyz, labels, cam, poses, set(), W, H), merged)
    assert np.array_equal(pm.labelled_keys(xyz, np.zeros(20_000, np.int32), cam, {}, set(), W, H), keys)
    # identity poses: the unlabelled frame; a moved object changes it; a hidden one drops its ids
    assert np.array_equal(pm.labelled_keys(xyz, labels, cam, {}, set(), W, H), keys)
    assert not np.array_equal(merged, keys)
    hid = pm.labelled_keys(xyz, labels, cam, poses, {1}, W, H)
    assert not np.isin((hid[hid != pm.EMPTY_KEY] & np.uint64(0xFFFFFFFF)).astype(np.int64), np.flatnonzero(labels == 1)).any()
    # the object camera moves points: rows (R4 @ P)[:3] applied to x equal the camera's rows applied to P x
    oc = pm.object_camera(cam, poses[1])
    x = np.array([1.0, 2.0, -3.0, 1.0])
    assert np.allclose(oc[:12].reshape(3, 4) @ x, cam[:12].reshape(3, 4) @ (poses[1] @ x), atol=1e-4) and np.array_equal(oc[12:], cam[12:])


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------
FAKE = 1 << 20          # a 256-byte aligned non-null address: the calls below fail on their arguments and never touch it
NEW = ("read_splat_forward_pano", "read_splat_pano_project_points")


def test_symbols_are_exported_and_declared():
    L = C.CDLL(_lib.LIB_PATH)
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "read_hip.h")).read()
    for name in NEW:
        assert hasattr(L, name) and name in _lib.SIGNATURES and f"int {name}(" in hdr, name
    assert _lib.lib().read_abi_version() == 3


def _cam(hfov=360.0):
    return camera.pano_camera(pc.proj(64, 48), np.eye(4), hfov)


def _objs(begin, n=None, M=True, visible=None):
    begin = np.asarray(begin, np.int64)
    count = len(begin) - 1
    Ms = np.tile(_cam(), (max(count, 1), 1)) if M else None
    vis = None if visible is None else np.asarray(visible, np.uint8)
    s = _lib.SplatObjects(FAKE, FAKE, int(begin[-1]) if n is None else n, count, begin.ctypes.data, None if Ms is None else Ms.ctypes.data,
                          None if vis is None else vis.ctypes.data)
    s.keep = (begin, Ms, vis)
    return s


def _forward(cam=None, W=64, H=48, levels=5, xyz=FAKE, ids=None, n=100, ws=FAKE, outs=True, objs=None, cam_null=False, ws_bytes=1 << 40):
    L = _lib.lib()
    cam = _cam() if cam is None else np.ascontiguousarray(cam, np.float32)
    idx = _lib.ptr_array([FAKE] * min(levels, 5)) if outs else None
    rc = L.read_splat_forward_pano(xyz, ids, n, None if cam_null else cam.ctypes.data_as(C.POINTER(C.c_float)), W, H, levels,
                                   None if objs is None else C.byref(objs), idx, None, ws, ws_bytes, None)
    return rc, L.read_last_error().decode()


@pytest.mark.parametrize("case", ["cam", "ws", "outputs", "xyz", "obj_begin", "obj_M", "obj_xyz", "obj_ids"])
def test_forward_pano_refuses_null_pointers(case):
    objs = None
    if case.startswith("obj_"):
        objs = _objs([0, 10, 30])
        if case == "obj_begin":
            objs.begin = None
        elif case == "obj_M":
            objs.M = None
        else:
            setattr(objs, case[4:], None)
    rc, msg = _forward(cam_null=case == "cam", ws=None if case == "ws" else FAKE, outs=case != "outputs",
                       xyz=None if case == "xyz" else FAKE, objs=objs)
    assert rc == -22 and "read_splat_forward_pano" in msg, (case, msg)
    assert ("no outputs" in msg) if case == "outputs" else ("null" in msg), (case, msg)


@pytest.mark.parametrize("W,H,levels", [(64, 40, 5), (40, 64, 5), (65, 48, 2), (1216, 352, 6)])
def test_forward_pano_refuses_sizes_off_the_pyramid(W, H, levels):
    rc, msg = _forward(W=W, H=H, levels=levels)
    assert rc == -22 and "read_splat_forward_pano" in msg, msg
    assert ("multiples of 2^(levels-1)" in msg) if levels <= 5 else ("levels" in msg), msg


def test_forward_pano_refuses_bad_cameras():
    for i in range(16):
        for bad in (np.nan, np.inf, -np.inf):
            cam = _cam()
            cam[i] = bad
            rc, msg = _forward(cam=cam)
            assert rc == -22 and "read_splat_forward_pano" in msg and "cam_host" in msg and "not finite" in msg, (i, bad, msg)
    for kx in (0.0, -1.0, np.float32(1.0 / np.pi) - np.float32(1e-7), 0.3):
        cam = _cam()
        cam[12] = kx
        rc, msg = _forward(cam=cam)
        assert rc == -22 and "kx" in msg and "1 / pi" in msg, (kx, msg)
    # an object's camera is held to the same conditions, unless the object is hidden or empty
    objs = _objs([0, 10, 30])
    objs.keep[1][1, 3] = np.nan
    rc, msg = _forward(objs=objs)
    assert rc == -22 and "object 1" in msg and "not finite" in msg, msg
    # the largest field and a narrow one pass the camera checks (and stop at the workspace size: nothing is launched)
    for hfov in (360.0, 45.0, 0.5):
        rc, msg = _forward(cam=_cam(hfov), ws_bytes=1024)
        assert rc == -12 and "workspace" in msg, (hfov, msg)
    objs = _objs([0, 10, 30], visible=[1, 0])
    objs.keep[1][1, 3] = np.nan
    rc, msg = _forward(objs=objs, ws_bytes=1024)
    assert rc == -12 and "workspace" in msg, msg


def test_forward_pano_refuses_bad_ranges():
    rc, msg = _forward(objs=_objs([0, 10, 5, 30]))
    assert rc == -22 and "read_splat_forward_pano" in msg and "not monotone at 1" in msg, msg
    rc, msg = _forward(objs=_objs([0, 10, 30], n=31))
    assert rc == -22 and "begin[count] = 30 != objs->n = 31" in msg, msg
    rc, msg = _forward(objs=_objs([3, 10, 30]))
    assert rc == -22 and "begin[0]" in msg, msg
    rc, msg = _forward(n=-1)
    assert rc == -22 and "n out of range" in msg, msg


def test_pano_project_points_refuses_bad_arguments():
    L = _lib.lib()
    cam = _cam()
    cp = cam.ctypes.data_as(C.POINTER(C.c_float))
    for args in ((None, 10, cp, 64, 48, FAKE), (FAKE, 10, cp, 64, 48, None), (FAKE, 10, None, 64, 48, FAKE), (FAKE, 10, cp, 0, 48, FAKE)):
        rc = L.read_splat_pano_project_points(args[0], args[1], args[2], args[3], args[4], args[5], None, None)
        assert rc == -22 and "read_splat_pano_project_points" in L.read_last_error().decode(), args
    cam[12] = 0.1
    rc = L.read_splat_pano_project_points(FAKE, 10, cp, 64, 48, FAKE, None, None)
    assert rc == -22 and "kx" in L.read_last_error().decode()
    cam[12], cam[5] = 1.0, np.nan
    rc = L.read_splat_pano_project_points(FAKE, 10, cp, 64, 48, FAKE, None, None)
    assert rc == -22 and "not finite" in L.read_last_error().decode()
    assert L.read_splat_pano_project_points(None, 0, _cam().ctypes.data_as(C.POINTER(C.c_float)), 64, 48, None, None, None) == 0


def test_scene_panorama_refusals_by_name():
    from read_amd.raster import PointCloudRasterizer
    from read_amd.render import MultiscaleRender, Scene, StitchedScene
    xyz = pc.ring_cloud(100, 0)
    scene = Scene(xyz)
    for bad in (0.0, 361.0, -5.0):
        with pytest.raises(ValueError):
            scene.set_panorama(bad)
    with pytest.raises(ValueError, match="set_panorama"):
        scene.pano_camera()
    scene.set_proj_matrix(pc.proj(64, 64))
    scene.set_camera_view(pc.pose(yaw=10.0))
    scene.set_panorama(360.0)
    assert np.array_equal(scene.pano_camera(), camera.pano_camera(pc.proj(64, 64), pc.pose(yaw=10.0), 360.0))
    fmt = "uv_1d_p1, uv_1d_p1_ds1, uv_1d_p1_ds2, uv_1d_p1_ds3"
    with pytest.raises(NotImplementedError, match="panorama.*MultiscaleRender"):
        MultiscaleRender(scene, fmt, (64, 64), out_buffer_location='torch').render()
    with pytest.raises(NotImplementedError, match="panorama.*MultiscaleRender"):
        MultiscaleRender(scene, "uv_1d_p1, xyz_p1_ds1", (64, 64), out_buffer_location='torch').render()
    st = StitchedScene([Scene(xyz), Scene(xyz)])
    with pytest.raises(NotImplementedError, match="panorama.*StitchedScene"):
        st.set_panorama(180.0)
    st.set_panorama(None)
    st.scenes[1].set_panorama(180.0)                                           # set on a part behind the stitched scene's back
    with pytest.raises(NotImplementedError, match="panorama.*StitchedScene"):
        MultiscaleRender(st, fmt, (64, 64), out_buffer_location='torch').render()
    scene.set_panorama(None)
    assert scene.panorama is None
    # render_gl names its refusal before it touches a device
    r = PointCloudRasterizer.__new__(PointCloudRasterizer)
    r.labels = None
    with pytest.raises(NotImplementedError, match="render_gl.*panorama"):
        r.render_gl(np.eye(4), 64, 64, pano=camera.pano_camera(np.eye(4), np.eye(4), 90.0))
