"""GPU: the panorama (cylindrical) camera on the fast render path against its NumPy definition, tests/pano_model.py
(DESIGN.md §10.3).  Every rasteriser comparison is exact: pixel per point, index and depth bit patterns on all five levels."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import oracle
from oracle import unet_torch
from read_amd import _lib, camera, synthetic
from read_amd.frame import FrameRenderer
from read_amd.ogl import OGL
from read_amd.raster import PointCloudRasterizer, label_layout, object_matrix
from read_amd.render import MultiscaleRender, Scene, StitchedScene
from read_amd.unet import weight_spec
from tests import pano_cases as pc
from tests import pano_model as pm

pytestmark = pytest.mark.gpu

LEVELS = 5
FMT = "uv_1d_p1, uv_1d_p1_ds1, uv_1d_p1_ds2, uv_1d_p1_ds3, uv_1d_p1_ds4"
MIN_PSNR, MAX_REL_RMS = 120.0, 1e-4          # the standing frame guards


def assert_frame(idx, dep, ref_idx, ref_dep, what=""):
    for l in range(len(ref_idx)):
        ri = torch.as_tensor(np.ascontiguousarray(ref_idx[l])).reshape(idx[l].shape).to(idx[l].device)
        assert torch.equal(idx[l], ri), f"{what}: index level {l}: {int((idx[l] != ri).sum())} pixels differ"
        if dep is not None:
            rd = torch.as_tensor(np.ascontiguousarray(ref_dep[l])).reshape(dep[l].shape).to(dep[l].device)
            assert torch.equal(dep[l].view(torch.int32), rd.view(torch.int32)), f"{what}: depth level {l}"


def copy(frame):
    return [t.clone() for t in frame[0]], [t.clone() for t in frame[1]]


# ---- the projection entry --------------------------------------------------------------------------------------------------------
OFFSET = np.array([5000.0, -5000.0, 5000.0])


@functools.lru_cache(maxsize=None)
def _operands():
    """2e6 points: random ones all round the camera (near the origin, and 5 km away for the second camera), the four axis
    directions and the camera's vertical axis at many distances, NaN and Inf coordinates."""
    rng = np.random.default_rng(21)
    n = 2_000_000
    xyz = np.empty((n, 3), np.float32)
    m = 1_200_000
    r = np.exp(rng.uniform(np.log(0.02), np.log(3000.0), m))
    th = rng.uniform(-np.pi, np.pi, m)
    xyz[:m, 0], xyz[:m, 2] = r * np.sin(th), -r * np.cos(th)
    xyz[:m, 1] = r * rng.uniform(-1.2, 1.2, m)
    k = 700_000                                                  # the same kind of cloud, 5 km from the origin
    r = np.exp(rng.uniform(np.log(0.5), np.log(500.0), k))
    th = rng.uniform(-np.pi, np.pi, k)
    xyz[m:m + k] = (np.stack([r * np.sin(th), r * rng.uniform(-1.0, 1.0, k), -r * np.cos(th)], 1) + OFFSET).astype(np.float32)
    a = m + k
    d = np.exp(rng.uniform(np.log(0.01), np.log(5000.0), 20_000)).astype(np.float32)
    for j, (ax, sg) in enumerate(((0, 1), (0, -1), (2, 1), (2, -1), (1, 1))):      # +-x, +-z; then +-y: rho = 0
        blk = np.zeros((20_000, 3), np.float32)
        blk[:, ax] = sg * d
        if ax == 1:
            blk[10_000:, 1] *= -1
        xyz[a + 20_000 * j:a + 20_000 * (j + 1)] = blk
    xyz[a + 80_000] = 0.0                                        # the camera centre itself
    bad = xyz[n - 1000:]
    bad[:] = rng.uniform(-10, 10, (1000, 3))
    vals = np.array([np.nan, np.inf, -np.inf], np.float32)
    bad[np.arange(1000), rng.integers(0, 3, 1000)] = vals[rng.integers(0, 3, 1000)]
    bad[:100, :] = vals[rng.integers(0, 3, (100, 3))]
    return xyz


@pytest.mark.parametrize("hfov", [360.0, 200.0, 45.0])
def test_projection_entry_equals_the_model(hip, hfov):
    W, H = 2432, 352
    xyz = _operands()
    dev = torch.from_numpy(xyz).cuda()
    pix = torch.empty(xyz.shape[0], dtype=torch.int32, device='cuda')
    dep = torch.empty(xyz.shape[0], dtype=torch.float32, device='cuda')
    views = (pc.pose(), pc.pose(yaw=140.0, pitch=9.0, roll=-4.0, t=(0.4, -0.3, 0.8)), pc.pose(yaw=-33.0, pitch=2.0, t=OFFSET))
    for v, view in enumerate(views):
        cam = camera.pano_camera(pc.proj(W, H), view, hfov)
        _lib.check(hip.read_splat_pano_project_points(dev.data_ptr(), xyz.shape[0], cam.ctypes.data_as(C.POINTER(C.c_float)), W, H,
                                                      pix.data_ptr(), dep.data_ptr(), _lib.stream_ptr()), "read_splat_pano_project_points")
        want_pix, want_dep = pm.project(xyz, cam, W, H)
        got_pix, got_dep = pix.cpu().numpy(), dep.cpu().numpy()
        ok = want_pix >= 0
        print(f"hfov {hfov} view {v}: {int(ok.sum())} of {ok.size} accepted, {int((got_pix != want_pix).sum())} pixels differ")
        assert np.array_equal(got_pix, want_pix), f"view {v}: {int((got_pix != want_pix).sum())} pixels differ"
        assert np.array_equal(got_dep[ok].view(np.uint32), want_dep[ok].view(np.uint32)), f"view {v}: depth bits"
        assert ok.sum() > 20_000
        assert (want_pix[-1000:] == -1).all()                                       # NaN / Inf
        assert v > 0 or (want_pix[1_980_000:1_999_000] == -1).all()                 # rho = 0 under the upright camera


# ---- frames ----------------------------------------------------------------------------------------------------------------------
def _poses(kind):
    if kind == "upright":
        return [pc.pose(yaw=10.0 * k, t=(0.2 * k, 0.0, -0.3 * k)) for k in range(3)]
    return [pc.pose(yaw=-25.0 + 8.0 * k, pitch=7.0, roll=-12.0 + k, t=(0.1, 0.2 * k, 0.3 * k)) for k in range(3)]


@pytest.mark.parametrize("hfov", [360.0, 120.0])
@pytest.mark.parametrize("kind", ["upright", "rolled"])
@pytest.mark.parametrize("W,H", [(96, 48), (256, 64)])
def test_frames_equal_the_model_and_alternate_with_the_pinhole(hip, W, H, kind, hfov):
    xyz = pc.ring_cloud(20_000, 11, dup=500)
    P = pc.proj(W, H)
    r = PointCloudRasterizer(xyz)
    views = _poses(kind)
    for k, view in enumerate(views):                                 # one workspace: frames 1 and 2 start from seeds
        cam = camera.pano_camera(P, view, hfov)
        got = r.render_pano(cam, W, H, LEVELS)
        assert_frame(*got, *pm.frame(xyz, cam, W, H, LEVELS), f"pose {k}")
    assert len(r._workspaces) == 1
    M = camera.total_matrix(P, views[0])[0]
    got = r.render(M, W, H, LEVELS)                                 # the pinhole, warm-started from a panorama's winners
    assert_frame(*got, *oracle.raster_multiscale(xyz, M, W, H, LEVELS), "pinhole after panorama")
    cam = camera.pano_camera(P, views[1], hfov)
    got = r.render_pano(cam, W, H, LEVELS, want_depth=False)        # and back, from the pinhole's winners; ids only
    assert got[1] is None
    assert_frame(got[0], None, *pm.frame(xyz, cam, W, H, LEVELS), "panorama after pinhole")
    assert len(r._workspaces) == 1
    with pytest.raises(ValueError, match="one camera"):
        r.render_pano(np.stack([cam, cam]), W, H, LEVELS)


def test_panorama_alternates_with_the_cell_path(hip):
    """>= 2^20 points and W % 16 == 0: the pinhole frames take the cell-ordered path (hi-z, bins, an announced next camera);
    panorama frames in between use the same workspace and leave it EMPTY."""
    W, H = 256, 64
    xyz = pc.ring_cloud((1 << 20) + 4096, 12, dup=2000)
    P = pc.proj(W, H)
    r = PointCloudRasterizer(xyz)
    assert r.cells is not None
    views = _poses("rolled")
    totals = [camera.total_matrix(P, v)[0] for v in views]
    cams = [camera.pano_camera(P, v, 360.0) for v in views]
    want_pano = [pm.pyramid_of(pm.key_image(xyz, c, W, H), W, H, LEVELS) for c in cams[:2]]
    want_pin = [oracle.raster_multiscale(xyz, M, W, H, LEVELS, threads=16) for M in totals]
    assert_frame(*r.render_pano(cams[0], W, H, LEVELS), *want_pano[0], "panorama on a fresh workspace")
    assert_frame(*r.render(totals[0], W, H, LEVELS, next_total=totals[1]), *want_pin[0], "cell path after panorama")
    assert_frame(*r.render_pano(cams[1], W, H, LEVELS), *want_pano[1], "panorama over a pending announcement")
    assert_frame(*r.render(totals[1], W, H, LEVELS, next_total=totals[2]), *want_pin[1], "cell path again")
    assert_frame(*r.render(totals[2], W, H, LEVELS), *want_pin[2], "cell path, announced")
    assert_frame(*r.render_pano(cams[0], W, H, LEVELS), *want_pano[0], "panorama after two cell frames")


def test_labels_moved_hidden_and_empty(hip):
    W, H = 96, 48
    n = 5000
    xyz = pc.ring_cloud(n, 13, dup=200)
    labels = pc.labels_for(n, 4, n_objects=3, share=0.15)
    labels[labels == 2] = 0                                          # object 2 has no points
    assert set(np.unique(labels)) == {0, 1, 3}
    r = PointCloudRasterizer(xyz, labels=labels)
    assert r.n_objects == 3
    cam = camera.pano_camera(pc.proj(W, H), pc.pose(yaw=20.0, pitch=-5.0, roll=6.0), 360.0)
    poses = {1: (pc.translation((3.0, 1.0, -2.0)) @ pc.rot(1, 40.0)).astype(np.float32), 2: pc.translation((1.0, 1.0, 1.0))}
    for k, Pk in poses.items():
        r.set_object_pose(k, Pk)
    first = copy(r.render_pano(cam, W, H, LEVELS))
    keys = pm.labelled_keys(xyz, labels, cam, poses, set(), W, H)
    assert_frame(*first, *pm.pyramid_of(keys, W, H, LEVELS), "moved")
    assert not np.array_equal(keys, pm.labelled_keys(xyz, labels, cam, {}, set(), W, H))          # the move shows
    r.set_object_visible(3, False)
    hidden = r.render_pano(cam, W, H, LEVELS)
    assert_frame(*hidden, *pm.pyramid_of(pm.labelled_keys(xyz, labels, cam, poses, {3}, W, H), W, H, LEVELS), "hidden")
    assert not torch.equal(hidden[0][0], first[0][0])
    r.set_object_visible(3, True)
    again = r.render_pano(cam, W, H, LEVELS)
    assert_frame(*again, [t.cpu().numpy() for t in first[0]], [t.cpu().numpy() for t in first[1]], "shown again")
    # identity poses: the unlabelled rasteriser's frame
    r.set_object_pose(1, None)
    r.set_object_pose(2, None)
    plain = PointCloudRasterizer(xyz).render_pano(cam, W, H, LEVELS)
    assert_frame(*r.render_pano(cam, W, H, LEVELS), [t.cpu().numpy() for t in plain[0]], [t.cpu().numpy() for t in plain[1]], "identity")


def test_forward_pano_partition_equals_the_rasteriser(hip):
    """read_splat_forward_pano with a hand-built read_splat_objects (the partition of ``label_layout``), as a C caller would
    pass it, against the rasteriser's own frame of the same labelled cloud (a range list through
    read_splat_forward_pano_instances) and against the model: one object moved, one hidden."""
    W, H, n = 256, 64, 200_000
    xyz = pc.ring_cloud(n, 15, dup=1000)
    labels = pc.labels_for(n, 5, n_objects=3, share=0.1)
    cam = camera.pano_camera(pc.proj(W, H), pc.pose(yaw=-15.0, pitch=4.0, roll=-7.0, t=(0.2, 0.1, -0.3)), 360.0)
    poses = {2: (pc.translation((2.0, -0.5, 1.5)) @ pc.rot(1, -25.0)).astype(np.float32)}
    r = PointCloudRasterizer(xyz, labels=labels)
    assert r._inst is not None and len(r._inst) == 3
    r.set_object_pose(2, poses[2])
    r.set_object_visible(3, False)
    got = r.render_pano(cam, W, H, LEVELS)
    # the C caller's side: static part, compacted objects, begin, one panorama camera per object, flags; a workspace of its own
    dev = torch.device("cuda")
    pts = torch.from_numpy(xyz).to(dev)
    static_ids, obj_ids, begin = label_layout(torch.from_numpy(labels).to(dev))
    static_xyz, obj_xyz = pts[static_ids.long()].contiguous(), pts[obj_ids.long()].contiguous()
    R4 = np.concatenate([cam[:12].reshape(3, 4), np.array([[0, 0, 0, 1]], np.float32)], 0)
    Ms = np.empty((3, 16), np.float32)
    for k in range(1, 4):
        Ms[k - 1, :12] = object_matrix(R4, poses.get(k))[:3].reshape(12)
        Ms[k - 1, 12:] = cam[12:]
    visible = np.array([1, 1, 0], np.uint8)
    objs = _lib.SplatObjects(obj_xyz.data_ptr(), obj_ids.data_ptr(), int(obj_ids.numel()), 3, begin.ctypes.data, Ms.ctypes.data,
                             visible.ctypes.data)
    ws = torch.empty(hip.read_splat_workspace_bytes(1, W, H), dtype=torch.uint8, device=dev)
    _lib.check(hip.read_splat_workspace_init(ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "read_splat_workspace_init")
    idx = [torch.empty_like(t) for t in got[0]]
    dep = [torch.empty_like(t) for t in got[1]]
    _lib.check(hip.read_splat_forward_pano(
        static_xyz.data_ptr(), static_ids.data_ptr(), int(static_ids.numel()), cam.ctypes.data_as(C.POINTER(C.c_float)), W, H, LEVELS,
        C.byref(objs), _lib.ptr_array([t.data_ptr() for t in idx]), _lib.ptr_array([t.data_ptr() for t in dep]), ws.data_ptr(),
        ws.numel(), _lib.stream_ptr()), "read_splat_forward_pano")
    assert_frame(idx, dep, [t.cpu().numpy() for t in got[0]], [t.cpu().numpy() for t in got[1]], "partition vs range list")
    keys = pm.labelled_keys(xyz, labels, cam, poses, {3}, W, H)
    assert_frame(idx, dep, *pm.pyramid_of(keys, W, H, LEVELS), "model")
    assert not np.array_equal(keys, pm.labelled_keys(xyz, labels, cam, {}, set(), W, H))          # the move and the hiding show


def test_thirty_three_instances_cross_the_flush(hip):
    """33 copies of object 1 beside the object itself: 34 ranges, two launches of range_splat_kernel under the panorama camera (32
    ranges each at most), one copy hidden."""
    W, H = 128, 48
    n = 5000
    xyz = pc.ring_cloud(n, 17)
    labels = pc.labels_for(n, 5, n_objects=1, share=0.04)
    sel = np.flatnonzero(labels == 1)
    assert 100 < sel.size < 1000
    r = PointCloudRasterizer(xyz, labels=labels)
    rng = np.random.default_rng(8)
    poses = [pc.translation(rng.uniform(-6.0, 6.0, 3)) for _ in range(33)]
    hs = [r.add_instance(1, P) for P in poses]
    r.set_instance_visible(hs[31], False)
    cam = camera.pano_camera(pc.proj(W, H), pc.pose(yaw=20.0, pitch=-5.0, roll=6.0), 360.0)
    assert r.pano_instance_cameras(cam).shape == (34, 16)
    keys = pm.labelled_keys(xyz, labels, cam, {}, set(), W, H)
    before = keys.copy()
    for i, P in enumerate(poses):
        if i != 31:
            pm.key_image(xyz[sel], pm.object_camera(cam, P), W, H, ids=sel, keys=keys)
    assert (keys != before).sum() > 30                               # the copies show
    last = pm.key_image(xyz[sel], pm.object_camera(cam, poses[32]), W, H, ids=sel)
    assert ((last != pm.EMPTY_KEY) & (last == keys)).any()           # and so does the one past the 32-range flush
    assert_frame(*r.render_pano(cam, W, H, LEVELS), *pm.pyramid_of(keys, W, H, LEVELS), "33 instances")


# ---- FrameRenderer ---------------------------------------------------------------------------------------------------------------
def _check_rgb(got, ref, what):
    diff = got.double() - ref.double()
    p = unet_torch.psnr(got, ref)
    rel = float(diff.pow(2).mean().sqrt() / ref.double().std())
    print("%s: max|diff| %.3e  PSNR %.1f dB  rms/std %.2e" % (what, float(diff.abs().max()), p, rel))
    assert p >= MIN_PSNR, f"{what}: PSNR {p:.1f} dB"
    assert rel <= MAX_REL_RMS, f"{what}: relative rms {rel:.3e}"


def test_frame_renderer_render_pano(hip):
    W, H, N = 192, 48, 20_000
    xyz, desc = pc.ring_cloud(N, 14, dup=300), synthetic.make_descriptors(N)
    state = synthetic.make_unet_state(weight_spec())
    P = pc.proj(W, H)
    fr1 = FrameRenderer(xyz, desc, state, W, H, proj_matrix=P)
    fr2 = FrameRenderer(xyz, desc, state, W, H, proj_matrix=P, frames_in_flight=2)
    views = _poses("rolled")
    outs1, outs2 = [], []
    for k, view in enumerate(views):
        rgba = fr1.render_pano(view, 360.0)
        torch.cuda.synchronize()
        outs1.append(rgba.clone())
        cam = camera.pano_camera(P, view, 360.0)
        mi, md = pm.frame(xyz, cam, W, H, LEVELS)
        assert_frame(fr1.idx, fr1.depth, mi, md, f"frame {k}")
        if k == 0:
            with torch.no_grad():
                ref = unet_torch.net_and_texture_forward(state, desc[None], mi)[0]
            _check_rgb(rgba[:, :, :3].permute(2, 0, 1).cpu(), ref, "render_pano vs oracle")
            assert bool((rgba[:, :, 3] == 1).all())
        outs2.append(fr2.render_pano(view, 360.0))
    fr2.sync()
    torch.cuda.synchronize()
    for k in range(3):
        assert torch.equal(outs1[k], outs2[k]), f"frames_in_flight 2, frame {k}"
    assert not torch.equal(outs1[0], outs1[1])
    # the total-level twin, and a pinhole frame on the same renderer afterwards
    cam = camera.pano_camera(P, views[2], 360.0)
    assert torch.equal(fr1.render_pano_total(cam), outs1[2])
    fr1.render(views[0])
    M = camera.total_matrix(P, views[0])[0]
    assert_frame(fr1.idx, fr1.depth, *oracle.raster_multiscale(xyz, M, W, H, LEVELS), "pinhole afterwards")
    with pytest.raises(ValueError):
        fr1.render_pano(views[0], 0.0)


# ---- Scene.set_panorama through OGL ----------------------------------------------------------------------------------------------
def test_ogl_set_panorama_stays_on_the_fast_path(hip):
    from tests.test_gpu_api import _model
    W, H, N = 192, 48, 20_000
    xyz = pc.ring_cloud(N, 15)
    model, state, tex = _model(N)
    P, view = pc.proj(W, H), pc.pose(yaw=30.0, pitch=4.0, roll=-3.0, t=(0.25, 0.125, -0.5))
    scene = Scene(xyz)
    scene.set_proj_matrix(P)
    scene.set_camera_view(view)
    ogl = OGL.from_model(scene, model, FMT, (W, H))
    pin0 = ogl.infer()['output'].clone()
    assert ogl.last_path == 'fast'
    scene.set_panorama(360.0)
    scene.announce_next_camera_view(pc.pose(yaw=31.0))               # ignored by a panorama frame (and consumed)
    out = ogl.infer()['output'].clone()
    assert ogl.last_path == 'fast' and scene.take_next_total_matrix() is None
    texture = tex.texture_.detach().reshape(-1, N)
    fr = FrameRenderer(xyz, texture, state, W, H, proj_matrix=P)
    ref = fr.render_pano(view, 360.0)
    torch.cuda.synchronize()
    cam = camera.pano_camera(P, view, 360.0)
    assert_frame(fr.idx, fr.depth, *pm.frame(xyz, cam, W, H, LEVELS), "FrameRenderer")
    torch.testing.assert_close(out, ref, rtol=0, atol=1e-6)
    assert not torch.equal(out, pin0)
    # the model matrix takes part as in total_matrix: moving the cloud and the camera together changes nothing (the
    # translations are dyadic, so the camera comes out the same 16 floats)
    T = pc.translation((1.0, -2.0, 0.5))
    scene.set_model_view(T)
    scene.set_camera_view((T.astype(np.float64) @ view.astype(np.float64)).astype(np.float32))
    assert np.array_equal(scene.pano_camera(), cam)
    assert torch.equal(ogl.infer()['output'], out)
    scene.set_model_view(np.eye(4, dtype=np.float32))
    scene.set_camera_view(view)
    # ---- refusals, each by name
    with pytest.raises(NotImplementedError, match="input_dict.*panorama"):
        ogl.infer({'id': 0})
    ogl.model.temporal_average = True
    with pytest.raises(NotImplementedError, match="temporal_average.*panorama"):
        ogl.infer()
    ogl.model.temporal_average = False
    ss = ogl.model.ss
    ogl.model.ss = 2
    with pytest.raises(NotImplementedError, match="supersampling 2.*panorama"):
        ogl.infer()
    ogl.model.ss = ss
    scene.set_point_discard(np.zeros(N, bool))
    with pytest.raises(NotImplementedError, match="augmentation.*panorama"):
        ogl.infer()
    scene.set_point_discard(None)
    with pytest.raises(NotImplementedError, match="xyz_p1.*panorama"):
        OGL.from_model(scene, model, "uv_1d_p1, xyz_p1_ds1, uv_1d_p1_ds2, uv_1d_p1_ds3", (W, H)).infer()
    with pytest.raises(NotImplementedError, match="panorama.*MultiscaleRender"):
        MultiscaleRender(scene, FMT, (W, H), out_buffer_location='torch').render()
    with pytest.raises(NotImplementedError, match="render_gl.*panorama"):
        scene.rasterizer().render_gl(scene.total_matrix(), W, H, pano=scene.pano_camera())
    st = StitchedScene([scene])
    with pytest.raises(NotImplementedError, match="panorama.*StitchedScene"):
        OGL.from_model(st, model, FMT, (W, H)).infer()
    with pytest.raises(NotImplementedError, match="panorama.*StitchedScene"):
        st.set_panorama(90.0)
    # ---- back to the pinhole, bit for bit
    scene.set_panorama(None)
    assert torch.equal(ogl.infer()['output'], pin0) and ogl.last_path == 'fast'
