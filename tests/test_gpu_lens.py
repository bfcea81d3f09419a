"""GPU: the lens cameras — a distorted pinhole and a fisheye — on the fast render path against their NumPy definition,
tests/lens_model.py.  Every rasteriser comparison is exact: pixel per point, index and depth bit patterns on
every level.  Sizes are small on purpose (64x48 with 5 levels, 32x16 with 2, 2e4 points); the one large cloud is the cell path's
threshold."""
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
from read_amd.raster import PointCloudRasterizer
from read_amd.render import MultiscaleRender, Scene, StitchedScene
from read_amd.texture import PointTexture
from read_amd.train import huber_loss
from read_amd.unet import weight_spec
from tests import lens_cases as lc
from tests import lens_model as lm
from tests import pano_cases as pc
from tests import pano_model as pm

pytestmark = pytest.mark.gpu

W, H, LEVELS = 64, 48, 5
FMT = "uv_1d_p1, uv_1d_p1_ds1, uv_1d_p1_ds2, uv_1d_p1_ds3, uv_1d_p1_ds4"
MIN_PSNR, MAX_REL_RMS = 120.0, 1e-4          # the standing frame guards
f32 = np.float32


def assert_frame(idx, dep, ref_idx, ref_dep, what=""):
    for l in range(len(ref_idx)):
        ri = torch.as_tensor(np.ascontiguousarray(ref_idx[l])).reshape(idx[l].shape).to(idx[l].device)
        assert torch.equal(idx[l], ri), f"{what}: index level {l}: {int((idx[l] != ri).sum())} pixels differ"
        if dep is not None:
            rd = torch.as_tensor(np.ascontiguousarray(ref_dep[l])).reshape(dep[l].shape).to(dep[l].device)
            assert torch.equal(dep[l].view(torch.int32), rd.view(torch.int32)), f"{what}: depth level {l}"


def copy(frame):
    return [t.clone() for t in frame[0]], [t.clone() for t in frame[1]]


def _poses(kind):
    if kind == "upright":
        return [pc.pose(yaw=10.0 * k, t=(0.2 * k, 0.0, -0.3 * k)) for k in range(3)]
    return [pc.pose(yaw=-25.0 + 8.0 * k, pitch=7.0, roll=-12.0 + k, t=(0.1, 0.2 * k, 0.3 * k)) for k in range(3)]


# ---- the projection entry --------------------------------------------------------------------------------------------------------
OFFSET = np.array([5000.0, -5000.0, 5000.0])
ENTRY = {"brown": lc.LENSES["brown"], "brown-limit-1": (0, lc.LENSES["brown"][1], 0.5, 1.0), "fisheye-200": lc.LENSES["fisheye"],
         "equidistant": lc.LENSES["equidistant"]}


@functools.lru_cache(maxsize=None)
def _operands():
    """100 003 points (not a multiple of 256): random ones all round the camera — behind its plane too — near the origin and
    5 km away for the third camera, the camera's axis in front and behind at many distances (rho = 0 under the first camera),
    directions at and next to every lens's limit, NaN and Inf coordinates."""
    rng = np.random.default_rng(21)
    n = 100_003
    xyz = np.empty((n, 3), f32)
    m = 60_000
    r = np.exp(rng.uniform(np.log(0.02), np.log(3000.0), m))
    th, az = np.arccos(rng.uniform(-1, 1, m)), rng.uniform(-np.pi, np.pi, m)          # theta off the -z axis, all of the sphere
    xyz[:m] = np.stack([r * np.sin(th) * np.cos(az), r * np.sin(th) * np.sin(az), -r * np.cos(th)], 1)
    k = 30_000
    r = np.exp(rng.uniform(np.log(0.5), np.log(500.0), k))
    th, az = np.arccos(rng.uniform(-1, 1, k)), rng.uniform(-np.pi, np.pi, k)
    xyz[m:m + k] = (np.stack([r * np.sin(th) * np.cos(az), r * np.sin(th) * np.sin(az), -r * np.cos(th)], 1) + OFFSET).astype(f32)
    a = m + k
    d = np.exp(rng.uniform(np.log(0.01), np.log(5000.0), 2000)).astype(f32)
    xyz[a:a + 4000] = 0.0
    xyz[a:a + 2000, 2] = -d                                         # the axis in front: rho = 0
    xyz[a + 2000:a + 4000, 2] = d                                   # and behind: theta = pi
    xyz[a + 4000] = 0.0                                             # the camera centre itself
    b = a + 4001
    at = []                                                         # directions at the limits: theta (model 1), r^2 (model 0)
    for lim in (float(np.deg2rad(100.0)), np.pi / 2, np.pi):
        for e in np.linspace(-3e-6, 3e-6, 25):
            for azi in (0.3, 2.0, -1.1):
                t = lim + e
                at.append(7.0 * np.array([np.sin(t) * np.cos(azi), np.sin(t) * np.sin(azi), -np.cos(t)]))
    for r2 in (1.0, 0.999 * 3.372159156302036):
        for e in np.linspace(-3e-6, 3e-6, 25):
            for azi in (0.3, 2.0, -1.1):
                rr = np.sqrt(r2 + e)
                at.append(3.0 * np.array([rr * np.cos(azi), rr * np.sin(azi), -1.0]))
    xyz[b:b + len(at)] = np.asarray(at)
    fill = xyz[b + len(at):n - 1000]
    fill[:] = rng.uniform(-10, 10, fill.shape)
    bad = xyz[n - 1000:]
    bad[:] = rng.uniform(-10, 10, (1000, 3))
    vals = np.array([np.nan, np.inf, -np.inf], f32)
    bad[np.arange(1000), rng.integers(0, 3, 1000)] = vals[rng.integers(0, 3, 1000)]
    bad[:100, :] = vals[rng.integers(0, 3, (100, 3))]
    return xyz


@pytest.mark.parametrize("lens", list(ENTRY))
def test_projection_entry_equals_the_model(hip, lens):
    Wp, Hp = 1216, 352
    xyz = _operands()
    n = xyz.shape[0]
    assert n % 256
    dev = torch.from_numpy(xyz).cuda()
    pix = torch.empty(n, dtype=torch.int32, device='cuda')
    dep = torch.empty(n, dtype=torch.float32, device='cuda')
    views = (pc.pose(), pc.pose(yaw=140.0, pitch=9.0, roll=-4.0, t=(0.4, -0.3, 0.8)), pc.pose(yaw=-33.0, pitch=2.0, t=OFFSET))
    for v, view in enumerate(views):
        cam = lc.lens_cam(ENTRY[lens], Wp, Hp, view)
        _lib.check(hip.read_splat_lens_project_points(dev.data_ptr(), n, cam.ctypes.data_as(C.POINTER(C.c_float)), Wp, Hp,
                                                      pix.data_ptr(), dep.data_ptr(), _lib.stream_ptr()), "read_splat_lens_project_points")
        want_pix, want_dep = lm.project(xyz, cam, Wp, Hp)
        got_pix, got_dep = pix.cpu().numpy(), dep.cpu().numpy()
        ok = want_pix >= 0
        print(f"{lens} view {v}: {int(ok.sum())} of {ok.size} accepted, {int((got_pix != want_pix).sum())} pixels differ")
        assert np.array_equal(got_pix, want_pix), f"view {v}: {int((got_pix != want_pix).sum())} pixels differ"
        assert np.array_equal(got_dep[ok].view(np.uint32), want_dep[ok].view(np.uint32)), f"view {v}: depth bits"
        assert ok.sum() > 2_000
        assert (want_pix[-1000:] == -1).all()                                       # NaN / Inf
        if v == 0:
            front, back = want_pix[90_000:92_000], want_pix[92_000:94_000]
            assert (front >= 0).sum() > 1000 and len(set(front[front >= 0])) == 1   # rho = 0 in front: the principal point
            c3 = -xyz[:, 2]
            behind = ok & (c3 < 0)
            if lens == "equidistant":                                               # limit pi: the axis behind is kept too
                assert (back >= 0).sum() > 1000 and set(back[back >= 0]) == set(front[front >= 0])
            elif lens == "fisheye-200":                                             # up to 100 degrees off the axis
                assert behind.sum() > 500 and (back == -1).all()
            else:
                assert not behind.any() and (back == -1).all()
            edge = want_pix[94_001:94_001 + 375]                                    # around the limits: both verdicts occur
            if lens in ("brown-limit-1", "fisheye-200"):
                assert (edge >= 0).any() and (edge == -1).any()


# ---- frames ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", ["brown", "fisheye"])
@pytest.mark.parametrize("kind", ["upright", "rolled"])
@pytest.mark.parametrize("w,h,levels", [(64, 48, 5), (32, 16, 2)])
def test_frames_equal_the_model_and_alternate(hip, w, h, levels, kind, lens):
    xyz = pc.ring_cloud(20_000, 11, dup=500)
    P = pc.proj(w, h)
    r = PointCloudRasterizer(xyz)
    views = _poses(kind)
    for k, view in enumerate(views):                                 # one workspace: frames 1 and 2 start from seeds
        cam = lc.lens_cam(lens, w, h, view)
        got = r.render_lens(cam, w, h, levels)
        want = lm.frame(xyz, cam, w, h, levels)
        assert_frame(*got, *want, f"pose {k}")
        assert_frame(*got, *lm.pyramid_of(lm.key_image(xyz, cam, w, h), w, h, levels), f"pose {k}, reduced")
        assert (want[0][0] != 0).sum() > 0.25 * w * h
    assert len(r._workspaces) == 1
    M = camera.total_matrix(P, views[0])[0]
    got = r.render(M, w, h, levels)                                  # the pinhole, warm-started from a lens frame's winners
    assert_frame(*got, *oracle.raster_multiscale(xyz, M, w, h, levels), "pinhole after lens")
    cam = lc.lens_cam(lens, w, h, views[1])
    got = r.render_lens(cam, w, h, levels, want_depth=False)         # and back, from the pinhole's winners; ids only
    assert got[1] is None
    assert_frame(got[0], None, *lm.frame(xyz, cam, w, h, levels), "lens after pinhole")
    pano = camera.pano_camera(P, views[2], 360.0)
    assert_frame(*r.render_pano(pano, w, h, levels), *pm.frame(xyz, pano, w, h, levels), "panorama after lens")
    other = lc.lens_cam("fisheye" if lens == "brown" else "brown", w, h, views[0])
    assert_frame(*r.render_lens(other, w, h, levels), *lm.frame(xyz, other, w, h, levels), "the other lens after panorama")
    assert len(r._workspaces) == 1
    with pytest.raises(ValueError, match="one camera"):
        r.render_lens(np.stack([cam, cam]), w, h, levels)


def test_lens_alternates_with_the_cell_path(hip):
    """2^20 points and more, W % 16 == 0: the pinhole frames take the cell-ordered path (hi-z, bins, an announced next camera);
    lens and panorama frames in between use the same workspace and leave it EMPTY."""
    w, h = 256, 64
    xyz = pc.ring_cloud(PointCloudRasterizer.CELLS_MIN_POINTS, 12, dup=2000)
    P = pc.proj(w, h)
    r = PointCloudRasterizer(xyz)
    assert r.cells is not None
    views = _poses("rolled")
    totals = [camera.total_matrix(P, v)[0] for v in views]
    fish = [lc.lens_cam("fisheye", w, h, v) for v in views[:2]]
    brown = lc.lens_cam("brown", w, h, views[2])
    pano = camera.pano_camera(P, views[1], 360.0)
    want_fish = [lm.pyramid_of(lm.key_image(xyz, c, w, h), w, h, LEVELS) for c in fish]
    want_brown = lm.pyramid_of(lm.key_image(xyz, brown, w, h), w, h, LEVELS)
    want_pano = pm.pyramid_of(pm.key_image(xyz, pano, w, h), w, h, LEVELS)
    want_pin = [oracle.raster_multiscale(xyz, M, w, h, LEVELS, threads=16) for M in totals]
    assert_frame(*r.render_lens(fish[0], w, h, LEVELS), *want_fish[0], "fisheye on a fresh workspace")
    assert_frame(*r.render(totals[0], w, h, LEVELS, next_total=totals[1]), *want_pin[0], "cell path after fisheye")
    assert_frame(*r.render_lens(fish[1], w, h, LEVELS), *want_fish[1], "fisheye over a pending announcement")
    assert_frame(*r.render(totals[1], w, h, LEVELS, next_total=totals[2]), *want_pin[1], "cell path again")
    assert_frame(*r.render(totals[2], w, h, LEVELS), *want_pin[2], "cell path, announced")
    assert_frame(*r.render_lens(brown, w, h, LEVELS), *want_brown, "distorted pinhole after two cell frames")
    assert_frame(*r.render_pano(pano, w, h, LEVELS), *want_pano, "panorama after lens")
    assert_frame(*r.render_lens(fish[0], w, h, LEVELS), *want_fish[0], "fisheye after panorama")
    assert len(r._workspaces) == 1


@pytest.mark.parametrize("lens", ["brown", "fisheye"])
def test_warm_start_on_and_off(hip, lens):
    xyz = pc.ring_cloud(20_000, 16, dup=500)
    views = _poses("rolled")
    cams = [lc.lens_cam(lens, W, H, v) for v in views[:2]]
    want = [lm.frame(xyz, c, W, H, LEVELS) for c in cams]
    assert not np.array_equal(want[0][0][0], want[1][0][0])          # the camera moved
    frames = {}
    try:
        for seeds in (1, 0):
            _lib.check(hip.read_tuning_set(b"splat_seeds", seeds), "read_tuning_set")
            r = PointCloudRasterizer(xyz)
            assert_frame(*r.render_lens(cams[0], W, H, LEVELS), *want[0], f"seeds {seeds}, first frame")
            frames[seeds] = copy(r.render_lens(cams[1], W, H, LEVELS))
            assert_frame(*frames[seeds], *want[1], f"seeds {seeds}, second frame")
    finally:
        _lib.check(hip.read_tuning_set(b"splat_seeds", 1), "read_tuning_set")


# ---- labels and instances --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", ["brown", "fisheye"])
def test_labels_moved_hidden_and_empty(hip, lens):
    n = 5000
    xyz = pc.ring_cloud(n, 13, dup=200)
    labels = pc.labels_for(n, 4, n_objects=3, share=0.15)
    labels[labels == 2] = 0                                          # object 2 has no points
    assert set(np.unique(labels)) == {0, 1, 3}
    r = PointCloudRasterizer(xyz, labels=labels)
    assert r.n_objects == 3
    cam = lc.lens_cam(lens, W, H, pc.pose(yaw=20.0, pitch=-5.0, roll=6.0))
    poses = {1: (pc.translation((3.0, 1.0, -2.0)) @ pc.rot(1, 40.0)).astype(f32), 2: pc.translation((1.0, 1.0, 1.0))}
    for k, Pk in poses.items():
        r.set_object_pose(k, Pk)
    first = copy(r.render_lens(cam, W, H, LEVELS))
    keys = lm.labelled_keys(xyz, labels, cam, poses, set(), W, H)
    assert_frame(*first, *lm.pyramid_of(keys, W, H, LEVELS), "moved")
    assert not np.array_equal(keys, lm.labelled_keys(xyz, labels, cam, {}, set(), W, H))          # the move shows
    r.set_object_visible(3, False)
    hidden = r.render_lens(cam, W, H, LEVELS)
    assert_frame(*hidden, *lm.pyramid_of(lm.labelled_keys(xyz, labels, cam, poses, {3}, W, H), W, H, LEVELS), "hidden")
    assert not torch.equal(hidden[0][0], first[0][0])
    r.set_object_visible(3, True)
    again = r.render_lens(cam, W, H, LEVELS)
    assert_frame(*again, [t.cpu().numpy() for t in first[0]], [t.cpu().numpy() for t in first[1]], "shown again")
    r.set_object_pose(1, None)                                       # identity poses: the unlabelled rasteriser's frame
    r.set_object_pose(2, None)
    plain = PointCloudRasterizer(xyz).render_lens(cam, W, H, LEVELS)
    assert_frame(*r.render_lens(cam, W, H, LEVELS), [t.cpu().numpy() for t in plain[0]], [t.cpu().numpy() for t in plain[1]], "identity")


def test_thirty_three_instances_cross_the_flush(hip):
    """33 copies of object 1 beside the object itself: 34 ranges, two launches of range_splat_kernel<LensCam> (32 ranges each at most)."""
    n = 5000
    xyz = pc.ring_cloud(n, 17)
    labels = pc.labels_for(n, 5, n_objects=1, share=0.04)
    sel = np.flatnonzero(labels == 1)
    r = PointCloudRasterizer(xyz, labels=labels)
    rng = np.random.default_rng(8)
    poses = [pc.translation(rng.uniform(-6.0, 6.0, 3)) for _ in range(33)]
    hs = [r.add_instance(1, P) for P in poses]
    r.set_instance_visible(hs[31], False)
    cam = lc.lens_cam("fisheye", W, H, pc.pose(yaw=20.0, pitch=-5.0, roll=6.0))
    assert r.lens_instance_cameras(cam).shape == (34, 16)
    keys = lm.labelled_keys(xyz, labels, cam, {}, set(), W, H)
    before = keys.copy()
    for i, P in enumerate(poses):
        if i != 31:
            lm.key_image(xyz[sel], lm.object_camera(cam, P), W, H, ids=sel, keys=keys)
    assert (keys != before).sum() > 30                               # the copies show
    last = lm.key_image(xyz[sel], lm.object_camera(cam, poses[32]), W, H, ids=sel)
    assert ((last != lm.EMPTY_KEY) & (last == keys)).any()           # and so does the one past the 32-range flush
    assert_frame(*r.render_lens(cam, W, H, LEVELS), *lm.pyramid_of(keys, W, H, LEVELS), "33 instances")


# ---- FrameRenderer ---------------------------------------------------------------------------------------------------------------
def _check_rgb(got, ref, what):
    diff = got.double() - ref.double()
    p = unet_torch.psnr(got, ref)
    rel = float(diff.pow(2).mean().sqrt() / ref.double().std())
    print("%s: max|diff| %.3e  PSNR %.1f dB  rms/std %.2e" % (what, float(diff.abs().max()), p, rel))
    assert p >= MIN_PSNR, f"{what}: PSNR {p:.1f} dB"
    assert rel <= MAX_REL_RMS, f"{what}: relative rms {rel:.3e}"


def test_frame_renderer_render_lens(hip):
    N = 20_000
    xyz, desc = pc.ring_cloud(N, 14, dup=300), synthetic.make_descriptors(N)
    state = synthetic.make_unet_state(weight_spec())
    model, coeffs, limit = lc.lens_args("fisheye")
    P = lc.proj(W, H, lc.LENSES["fisheye"][2])
    fr1 = FrameRenderer(xyz, desc, state, W, H, proj_matrix=P)
    fr2 = FrameRenderer(xyz, desc, fr1.packed, W, H, proj_matrix=P, frames_in_flight=2)      # the blob fr1 packed: no second packing
    views = _poses("rolled")
    outs1, outs2 = [], []
    for k, view in enumerate(views):
        rgba = fr1.render_lens(view, model, coeffs, limit)
        torch.cuda.synchronize()
        outs1.append(rgba.clone())
        cam = camera.lens_camera(P, view, model, coeffs, limit)
        mi, md = lm.frame(xyz, cam, W, H, LEVELS)
        assert_frame(fr1.idx, fr1.depth, mi, md, f"frame {k}")
        if k == 0:
            with torch.no_grad():
                ref = unet_torch.net_and_texture_forward(state, desc[None], mi)[0]
            _check_rgb(rgba[:, :, :3].permute(2, 0, 1).cpu(), ref, "render_lens vs oracle")
            assert bool((rgba[:, :, 3] == 1).all())
        outs2.append(fr2.render_lens(view, model, coeffs, limit))
    fr2.sync()
    torch.cuda.synchronize()
    for k in range(3):
        assert torch.equal(outs1[k], outs2[k]), f"frames_in_flight 2, frame {k}"
    assert not torch.equal(outs1[0], outs1[1])
    # the total-level twin, and a pinhole frame on the same renderer afterwards
    cam = camera.lens_camera(P, views[2], model, coeffs, limit)
    assert torch.equal(fr1.render_lens_total(cam), outs1[2])
    fr1.render(views[0])
    M = camera.total_matrix(P, views[0])[0]
    assert_frame(fr1.idx, fr1.depth, *oracle.raster_multiscale(xyz, M, W, H, LEVELS), "pinhole afterwards")
    with pytest.raises(ValueError):
        fr1.render_lens(views[0], 2, ())
    with pytest.raises(ValueError, match="pi"):
        fr1.render_lens(views[0], 1, (), 3.5)


# ---- Scene.set_lens through OGL --------------------------------------------------------------------------------------------------
def test_ogl_set_lens_stays_on_the_fast_path(hip):
    from tests.test_gpu_api import _model
    N = 20_000
    xyz = pc.ring_cloud(N, 15)
    net, state, tex = _model(N)
    lens_model, coeffs, limit = lc.lens_args("fisheye")
    P, view = lc.proj(W, H, lc.LENSES["fisheye"][2]), pc.pose(yaw=30.0, pitch=4.0, roll=-3.0, t=(0.25, 0.125, -0.5))
    scene = Scene(xyz)
    scene.set_proj_matrix(P)
    scene.set_camera_view(view)
    ogl = OGL.from_model(scene, net, FMT, (W, H))
    pin0 = ogl.infer()['output'].clone()
    assert ogl.last_path == 'fast'
    scene.set_lens(lens_model, coeffs, limit)
    scene.announce_next_camera_view(pc.pose(yaw=31.0))               # ignored by a lens frame (and consumed)
    out = ogl.infer()['output'].clone()
    assert ogl.last_path == 'fast' and scene.take_next_total_matrix() is None
    texture = tex.texture_.detach().reshape(-1, N)
    fr = FrameRenderer(xyz, texture, ogl.model.net.packed_weights(), W, H, proj_matrix=P)   # the blob the model packed
    ref = fr.render_lens(view, lens_model, coeffs, limit)
    torch.cuda.synchronize()
    cam = camera.lens_camera(P, view, lens_model, coeffs, limit)
    assert_frame(fr.idx, fr.depth, *lm.frame(xyz, cam, W, H, LEVELS), "FrameRenderer")
    torch.testing.assert_close(out, ref, rtol=0, atol=1e-6)
    assert not torch.equal(out, pin0)
    # the model matrix takes part as in total_matrix (dyadic translations: the camera comes out the same 32 floats)
    T = pc.translation((1.0, -2.0, 0.5))
    scene.set_model_view(T)
    scene.set_camera_view((T.astype(np.float64) @ view.astype(np.float64)).astype(f32))
    assert np.array_equal(scene.lens_camera(), cam)
    assert torch.equal(ogl.infer()['output'], out)
    scene.set_model_view(np.eye(4, dtype=f32))
    scene.set_camera_view(view)
    # ---- the dict path serves the same id pyramid under the lens
    maps = MultiscaleRender(scene, FMT, (W, H), out_buffer_location='torch').render()
    mi, _ = lm.frame(xyz, cam, W, H, LEVELS)
    for l, key in enumerate(FMT.replace(' ', '').split(',')):
        assert np.array_equal(maps[key][..., 0].cpu().numpy(), mi[l].astype(f32)), key
    # ---- refusals, each by name
    with pytest.raises(NotImplementedError, match="input_dict.*lens"):
        ogl.infer({'id': 0})
    ogl.model.temporal_average = True
    with pytest.raises(NotImplementedError, match="temporal_average.*lens"):
        ogl.infer()
    ogl.model.temporal_average = False
    ss = ogl.model.ss
    ogl.model.ss = 2
    with pytest.raises(NotImplementedError, match="supersampling 2.*lens"):
        ogl.infer()
    ogl.model.ss = ss
    scene.set_point_discard(np.zeros(N, bool))
    with pytest.raises(NotImplementedError, match="augmentation.*lens"):
        ogl.infer()
    with pytest.raises(NotImplementedError, match="augmentation.*lens"):
        MultiscaleRender(scene, FMT, (W, H), out_buffer_location='torch').render()
    scene.set_point_discard(None)
    with pytest.raises(NotImplementedError, match="xyz_p1.*lens"):
        OGL.from_model(scene, net, "uv_1d_p1, xyz_p1_ds1, uv_1d_p1_ds2, uv_1d_p1_ds3", (W, H)).infer()
    with pytest.raises(NotImplementedError, match="xyz_p1.*lens"):
        MultiscaleRender(scene, "uv_1d_p1, xyz_p1_ds1", (W, H), out_buffer_location='torch').render()
    with pytest.raises(NotImplementedError, match="supersampling 2.*lens"):
        MultiscaleRender(scene, FMT, (W, H), out_buffer_location='torch', supersampling=2).render()
    with pytest.raises(NotImplementedError, match="render_gl.*lens"):
        scene.rasterizer().render_gl(scene.total_matrix(), W, H, lens=scene.lens_camera())
    with pytest.raises(NotImplementedError, match="lens.*select_masks"):
        scene.select_masks([], [], (W, H))
    with pytest.raises(NotImplementedError, match="lens.*annotate_frame"):
        scene.annotate_frame((W, H))
    with pytest.raises(NotImplementedError, match="lens.*infer_annotated"):
        ogl.infer_annotated()
    with pytest.raises(ValueError, match="set_panorama.*lens"):
        scene.set_panorama(180.0)
    st = StitchedScene([scene])
    with pytest.raises(NotImplementedError, match="lens.*StitchedScene"):
        OGL.from_model(st, net, FMT, (W, H)).infer()
    with pytest.raises(NotImplementedError, match="lens.*StitchedScene"):
        st.set_lens(1, ())
    # ---- back to the pinhole, bit for bit
    scene.set_lens(None)
    assert torch.equal(ogl.infer()['output'], pin0) and ogl.last_path == 'fast'


# ---- training under a lens -------------------------------------------------------------------------------------------------------
def test_one_training_step_under_a_fisheye(hip):
    """The TexturePipeline step on the 64x48 scene: MultiscaleRender's id pyramid under the lens -> NetAndTexture -> loss ->
    backward.  The rows that receive gradient are exactly the ids of the levels the UNet reads (four of the five)."""
    from read_amd.net_texture import NetAndTexture
    from read_amd.train import SparseDescriptorRMSprop
    from read_amd.unet import UNet
    N = 20_000
    xyz = pc.ring_cloud(N, 18)
    lens_model, coeffs, limit = lc.lens_args("fisheye")
    P, view = lc.proj(W, H, lc.LENSES["fisheye"][2]), pc.pose(yaw=-20.0, pitch=3.0, roll=5.0, t=(0.2, 0.1, 0.4))
    scene = Scene(xyz)
    scene.set_proj_matrix(P)
    scene.set_camera_view(view)
    scene.set_lens(lens_model, coeffs, limit)
    renderer = MultiscaleRender(scene, FMT, (W, H), out_buffer_location='torch')
    maps = renderer.render()
    keys = FMT.replace(' ', '').split(',')
    cam = camera.lens_camera(P, view, lens_model, coeffs, limit)
    mi, _ = lm.frame(xyz, cam, W, H, LEVELS)
    assert np.array_equal(maps['uv_1d_p1'][..., 0].cpu().numpy(), mi[0].astype(f32))
    assert maps['uv_1d_p1'].shape == (H, W, 3) and not maps['uv_1d_p1'][..., 1:].any()
    assert_frame(renderer.last_index, None, mi, None, "last_index")
    tex = PointTexture(8, N, init_method='rand')
    tex.sparse_training = True
    net = UNet()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synthetic.make_unet_state(weight_spec(), 8).items()})
    model = NetAndTexture(net, {0: tex})
    model.load_textures(0)
    model.cuda().eval()
    inputs = {'id': [0]}
    inputs.update({k: maps[k].permute(2, 0, 1)[None, :1].contiguous() for k in keys})
    adam = torch.optim.Adam(model.net.parameters(), lr=1e-3)
    opt = SparseDescriptorRMSprop([tex], lr=0.1)
    before = tex.rows().clone()
    loss = huber_loss(model(inputs), torch.rand(1, 3, H, W, device="cuda"))
    loss.backward()
    pids, pg = tex.take_pending()
    tex._pending.append((pids, pg))
    named = np.unique(pids.cpu().numpy().astype(np.int64))
    want = np.unique(np.concatenate([m.reshape(-1) for m in mi[:4]]).astype(np.int64))
    assert np.array_equal(named, want), "the rows that receive gradient are not the ids of the lens pyramid"
    adam.step()
    opt.step()
    model.check_ids()
    assert np.isfinite(float(loss.detach()))
    changed = np.flatnonzero((tex.rows() != before).any(1).cpu().numpy())
    assert changed.size > 0 and np.isin(changed, want).all()
