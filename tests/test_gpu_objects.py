"""GPU: scene editing — objects of a labelled cloud moved by poses and hidden, on the fast render path.

The contract (read_splat_forward_objects): label k is projected with M_k = M_0 @ P_k (raster.object_matrix), per pixel the minimum
(depth, original id) wins over every visible point, levels as always.  Its oracle: oracle.raster_multiscale on each label's subset
with its own matrix, local ids mapped to original ids, merged on (depth, id).  Every comparison is exact (torch.equal on the ids and
on the depth bit patterns, all 5 levels)."""
import numpy as np
import pytest
import torch

import oracle
from oracle import unet_torch
from read_amd import camera, synthetic
from read_amd.frame import FrameRenderer
from read_amd.ogl import OGL
from read_amd.raster import PointCloudRasterizer, object_matrix
from read_amd.render import MultiscaleRender, Scene
from read_amd.unet import weight_spec

pytestmark = pytest.mark.gpu

LEVELS = 5
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
FMT = "uv_1d_p1, uv_1d_p1_ds1, uv_1d_p1_ds2, uv_1d_p1_ds3, uv_1d_p1_ds4"


def oracle_edit(xyz, labels, M0, W, H, poses=None, hidden=()):
    """The merge the contract defines, level by level."""
    poses = poses or {}
    sizes = camera.level_sizes(W, H, LEVELS)
    keys = [np.full((h, w), EMPTY, np.uint64) for (w, h) in sizes]
    for k in np.unique(labels):
        if int(k) in hidden:
            continue
        sel = np.flatnonzero(labels == k)
        Mk = object_matrix(M0, poses.get(int(k))) if k else np.asarray(M0, np.float32).reshape(4, 4)
        oi, od = oracle.raster_multiscale(xyz[sel], Mk, W, H, LEVELS, threads=16)
        for l in range(LEVELS):
            bits = od[l].view(np.uint32)
            key = (bits.astype(np.uint64) << np.uint64(32)) | sel[oi[l]].astype(np.uint64)
            key[(oi[l] == 0) & (bits == 0)] = EMPTY
            keys[l] = np.minimum(keys[l], key)
    idx, dep = [], []
    for key in keys:
        empty = key == EMPTY
        idx.append(np.where(empty, 0, key & np.uint64(0xFFFFFFFF)).astype(np.int32))
        dep.append(np.where(empty, 0, key >> np.uint64(32)).astype(np.uint32).view(np.float32))
    return idx, dep


def assert_frame(idx, dep, ref_idx, ref_dep, what=""):
    for l in range(LEVELS):
        ri = torch.as_tensor(np.ascontiguousarray(ref_idx[l])).reshape(idx[l].shape).to(idx[l].device)
        rd = torch.as_tensor(np.ascontiguousarray(ref_dep[l])).reshape(dep[l].shape).to(dep[l].device)
        assert torch.equal(idx[l], ri), f"{what}: index level {l}: {int((idx[l] != ri).sum())} pixels differ"
        assert torch.equal(dep[l].view(torch.int32), rd.view(torch.int32)), f"{what}: depth level {l}"


def assert_same(a, b, what=""):
    assert_frame(a[0], a[1], [t.cpu().numpy() for t in b[0]], [t.cpu().numpy() for t in b[1]], what)


def copy(frame):
    return [t.clone() for t in frame[0]], [t.clone() for t in frame[1]]


def cluster_labels(xyz, n_objects, size, seed):
    """Objects = clusters of `size` points around random seed points (disjoint), label 0 for the rest."""
    rng = np.random.default_rng(seed)
    labels = np.zeros(xyz.shape[0], np.int32)
    for k in range(1, n_objects + 1):
        free = np.flatnonzero(labels == 0)
        c = xyz[free[rng.integers(free.size)]]
        d = ((xyz[free] - c) ** 2).sum(1)
        labels[free[np.argpartition(d, size)[:size]]] = k
    return labels


def camera_space_target(view, proj, ndc_x, depth, behind=False):
    """A world point at normalised image column ndc_x, `depth` in front of the camera of `view` (camera -> world), or the mirror
    image of that point behind the camera."""
    P = proj.astype(np.float64)
    for s in (-1.0, 1.0):
        z = s * depth
        clip = P @ np.array([0.0, 0.0, z, 1.0])
        if clip[3] > 0 and abs(clip[2] / clip[3]) <= 1:
            x = (ndc_x * clip[3] - P[0, 2] * z - P[0, 3]) / P[0, 0]
            c = np.array([-x if behind else x, 0.0, -z if behind else z, 1.0])
            return (view.astype(np.float64) @ c)[:3]
    raise AssertionError("no direction in front of the camera")


def translation(t):
    P = np.eye(4, dtype=np.float32)
    P[:3, 3] = np.asarray(t, np.float32)
    return P


def about(c, R, t):
    """Rotate by R about the point c, then translate to c + t."""
    P = np.eye(4, dtype=np.float64)
    P[:3, :3] = R
    P[:3, 3] = np.asarray(c) + np.asarray(t) - R @ np.asarray(c)
    return P.astype(np.float32)


def rot_z(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]], np.float64)


# ---- identity poses: the unlabelled frame, bit for bit ------------------------------------------------------------------
@pytest.mark.parametrize("cloud", ["street3M", "cloud200k"])
def test_identity_poses_equal_the_unlabelled_rasteriser(hip, cloud):
    W, H = 1216, 352
    xyz = synthetic.make_street_cloud(3_000_000, 5) if cloud == "street3M" else synthetic.make_cloud(200_000, 6)
    labels = cluster_labels(xyz, 6, 20_000 if cloud == "street3M" else 5_000, 11)
    proj = synthetic.make_proj(W, H)
    plain = PointCloudRasterizer(xyz)
    edit = PointCloudRasterizer(xyz, labels=labels)
    assert (edit.cells is not None) == (cloud == "street3M") and (edit.n_static >= (1 << 20)) == (cloud == "street3M")
    totals = [camera.total_matrix(proj, synthetic.sweep_pose(k))[0] for k in range(9)]
    for k in range(8):
        a = plain.render(totals[k], W, H, LEVELS, next_total=totals[k + 1])
        b = edit.render(totals[k], W, H, LEVELS, next_total=totals[k + 1])
        assert_same(b, a, f"{cloud} pose {k}")
    assert_frame(*b, *oracle_edit(xyz, labels, totals[7], W, H), f"{cloud} oracle")


# ---- objects re-posed every frame -------------------------------------------------------------------------------------------
def _street_scene():
    W, H = 1216, 352
    xyz = synthetic.make_street_cloud(3_000_000, 5)
    labels = cluster_labels(xyz, 6, 20_000, 12)
    return W, H, xyz, labels, synthetic.make_proj(W, H)


def _poses_for_frame(f, xyz, labels, view, proj, W, H):
    cents = {k: xyz[labels == k].astype(np.float64).mean(0) for k in range(1, 7)}
    poses = {}
    # 1: crosses in front of the camera, left to right over the frames
    poses[1] = translation(camera_space_target(view, proj, -0.9 + 0.36 * f, 6.0) - cents[1])
    # 2: straddles the left image border
    poses[2] = translation(camera_space_target(view, proj, -1.0, 20.0) - cents[2])
    # 3: entirely behind the camera
    poses[3] = translation(camera_space_target(view, proj, 0.0, 10.0, behind=True) - cents[3])
    # 4, 5: turned about their centres and shifted a little; 6: identity
    poses[4] = about(cents[4], rot_z(0.2 * f), (0.1 * f, 0.0, 0.0))
    poses[5] = about(cents[5], rot_z(-0.35 * f), (0.0, 0.05 * f, 0.02 * f))
    poses[6] = None
    return poses


def test_reposed_objects_every_frame_equal_the_oracle(hip):
    W, H, xyz, labels, proj = _street_scene()
    r = PointCloudRasterizer(xyz, labels=labels)
    assert r.cells is not None
    views = [synthetic.sweep_pose(10 + 2 * f) for f in range(7)]
    totals = [camera.total_matrix(proj, v)[0] for v in views]
    for f in range(6):
        poses = _poses_for_frame(f, xyz, labels, views[f], proj, W, H)
        for k, P in poses.items():
            r.set_object_pose(k, P)
        got = r.render(totals[f], W, H, LEVELS, next_total=totals[f + 1])
        ref = oracle_edit(xyz, labels, totals[f], W, H, poses)
        assert_frame(*got, *ref, f"frame {f}")
        if f == 0:       # the near object really covers pixels; the one behind the camera none
            assert bool(torch.isin(got[0][0], torch.from_numpy(np.flatnonzero(labels == 1)).cuda()).any())
            assert not bool(torch.isin(got[0][0], torch.from_numpy(np.flatnonzero(labels == 3)).cuda()).any())


@pytest.mark.parametrize("cloud", ["street3M", "cloud200k"])
def test_hide_then_show(hip, cloud):
    W, H = 1216, 352
    xyz = synthetic.make_street_cloud(3_000_000, 5) if cloud == "street3M" else synthetic.make_cloud(200_000, 6)
    labels = cluster_labels(xyz, 4, 20_000 if cloud == "street3M" else 5_000, 13)
    proj = synthetic.make_proj(W, H)
    view = synthetic.sweep_pose(20)
    M0 = camera.total_matrix(proj, view)[0]
    r = PointCloudRasterizer(xyz, labels=labels)
    cent = xyz[labels == 2].astype(np.float64).mean(0)
    poses = {2: translation(camera_space_target(view, proj, 0.1, 8.0) - cent)}
    r.set_object_pose(2, poses[2])
    before = copy(r.render(M0, W, H, LEVELS, next_total=M0))
    assert_frame(*before, *oracle_edit(xyz, labels, M0, W, H, poses), "before")
    assert bool(torch.isin(before[0][0], torch.from_numpy(np.flatnonzero(labels == 2)).cuda()).any())
    r.set_object_visible(2, False)
    hidden = r.render(M0, W, H, LEVELS, next_total=M0)
    assert_frame(*hidden, *oracle_edit(xyz, labels, M0, W, H, poses, hidden={2}), "hidden")
    # the frame of the cloud without those points (the others are not posed), every other point keeping its id
    keep = np.flatnonzero(labels != 2)
    oi, od = oracle.raster_multiscale(xyz[keep], M0, W, H, LEVELS, threads=16)
    assert_frame(*hidden, [np.where((oi[l] == 0) & (od[l].view(np.uint32) == 0), 0, keep[oi[l]]).astype(np.int32)
                           for l in range(LEVELS)], od, "hidden vs the cloud without the object")
    r.set_object_visible(2, True)
    again = r.render(M0, W, H, LEVELS)
    assert_same(again, before, "shown again")


# ---- edge cases -----------------------------------------------------------------------------------------------------------------
def test_empty_static_part_and_empty_object(hip):
    W, H = 256, 128
    xyz = synthetic.make_cloud(50_000, 8)
    labels = np.where(np.arange(50_000) % 3 == 0, 1, 3).astype(np.int32)       # no label 0; label 2 has no points
    proj = synthetic.make_proj(W, H, f=120.0)
    M0 = camera.total_matrix(proj, synthetic.sweep_pose(2))[0]
    r = PointCloudRasterizer(xyz, labels=labels)
    assert r.n_static == 0 and r.n_objects == 3 and r.cells is None
    poses = {1: translation((0.3, 0.0, 0.1)), 2: translation((5.0, 5.0, 5.0)), 3: None}
    for k, P in poses.items():
        r.set_object_pose(k, P)
    got = r.render(M0, W, H, LEVELS)
    assert_frame(*got, *oracle_edit(xyz, labels, M0, W, H, poses), "no static part")
    r.set_object_visible(1, False)
    r.set_object_visible(3, False)
    got = r.render(M0, W, H, LEVELS)                                            # nothing drawn: every pixel empty
    for l in range(LEVELS):
        assert not bool(got[0][l].any()) and not bool(got[1][l].view(torch.int32).any())


@pytest.mark.parametrize("n_static", [20_000, (1 << 20) + 4096])
def test_tie_between_object_and_static_point_goes_to_the_minimum_id(hip, n_static):
    W, H = 256, 128
    base = synthetic.make_cloud(n_static, 9)
    proj = synthetic.make_proj(W, H, f=120.0)
    M0 = camera.total_matrix(proj, synthetic.sweep_pose(1))[0]
    # 64 static points that win their pixels get an object twin at exactly their position: ties on every level-0 pixel they own
    front = np.unique(oracle.raster_multiscale(base, M0, W, H, 1, threads=16)[0][0])
    dup_src = np.random.default_rng(1).choice(front[front > 0], 64, replace=False)
    # the first 32 twins get smaller ids than their originals, the last 32 larger ones
    xyz = np.concatenate([base[dup_src[:32]], base, base[dup_src[32:]]]).astype(np.float32)
    labels = np.zeros(xyz.shape[0], np.int32)
    labels[:32] = 1
    labels[32 + n_static:] = 2
    r = PointCloudRasterizer(xyz, labels=labels)
    assert (r.cells is not None) == (n_static >= (1 << 20))
    got = r.render(M0, W, H, LEVELS)
    assert_frame(*got, *oracle_edit(xyz, labels, M0, W, H), "ties")
    plain = PointCloudRasterizer(xyz)                                           # identity poses: the unlabelled frame
    assert_same(got, plain.render(M0, W, H, LEVELS), "ties vs unlabelled")
    pix, _ = oracle.project_points(base[dup_src], M0, W, H)
    assert (pix >= 0).all()
    won = got[0][0].reshape(-1).cpu().numpy()[pix]
    assert np.array_equal(won[:32], np.arange(32)), "a twin with the smaller id must win"
    assert np.array_equal(won[32:], 32 + dup_src[32:]), "the original with the smaller id must win"


# ---- FrameRenderer, OGL, MultiscaleRender ---------------------------------------------------------------------------------------
def _frame_setup(N=40_000):
    W = H = 256
    xyz, desc = synthetic.make_cloud(N, 3), synthetic.make_descriptors(N)
    labels = cluster_labels(xyz, 4, 2_000, 14)
    state = synthetic.make_unet_state(weight_spec())
    proj = synthetic.make_proj(W, H, f=160.0)
    return W, H, xyz, desc, labels, state, proj


def _frame_poses(f, xyz, labels):
    return {k: about(xyz[labels == k].astype(np.float64).mean(0), rot_z(0.3 * f * k), (0.05 * f, -0.03 * f * k, 0.0))
            for k in range(1, int(labels.max()) + 1)}


def test_frame_renderer_with_objects_matches_the_oracle_frame(hip):
    W, H, xyz, desc, labels, state, proj = _frame_setup()
    fr = FrameRenderer(xyz, desc, state, W, H, proj_matrix=proj, object_labels=labels)
    for f in range(2):
        poses = _frame_poses(f, xyz, labels)
        for k, P in poses.items():
            fr.set_object_pose(k, P)
        fr.set_object_visible(2, f == 0)
        view = synthetic.sweep_pose(3 + f)
        rgba = fr.render(view)
        torch.cuda.synchronize()
        M = camera.total_matrix(proj, view)[0]
        oi, od = oracle_edit(xyz, labels, M, W, H, poses, hidden=() if f == 0 else {2})
        assert_frame(fr.idx, fr.depth, oi, od, f"frame {f}")
        with torch.no_grad():
            ref = unet_torch.net_and_texture_forward(state, desc[None], oi)[0]
        got = rgba[:, :, :3].permute(2, 0, 1).cpu()
        assert float((got - ref).abs().max()) <= 5e-6
        assert unet_torch.psnr(got, ref) >= 120.0


def test_frames_in_flight_with_poses_changing_between_calls(hip):
    W, H, xyz, desc, labels, state, proj = _frame_setup()
    fr1 = FrameRenderer(xyz, desc, state, W, H, proj_matrix=proj, object_labels=labels)
    fr2 = FrameRenderer(xyz, desc, state, W, H, proj_matrix=proj, object_labels=labels, frames_in_flight=2)
    outs1, outs2 = [], []
    for f in range(5):
        for fr in (fr1, fr2):
            for k, P in _frame_poses(f, xyz, labels).items():
                fr.set_object_pose(k, P)
            fr.set_object_visible(3, f % 2 == 0)
        outs1.append(fr1.render(synthetic.sweep_pose(f)).clone())
        outs2.append(fr2.render(synthetic.sweep_pose(f)))               # a fresh tensor per call, complete on frame_done
    fr2.sync()
    torch.cuda.synchronize()
    for f in range(5):
        assert torch.equal(outs1[f], outs2[f]), f"frame {f}"
    assert not torch.equal(outs1[0], outs1[1])


def test_ogl_fast_path_and_multiscale_render_honour_the_edits(hip):
    from tests.test_gpu_api import _model
    W, H, N = 128, 64, 25_000
    xyz = synthetic.make_cloud(N)
    labels = cluster_labels(xyz, 3, 1_500, 15)
    model, state, tex = _model(N)
    scene = Scene(xyz)
    proj, pose = synthetic.make_proj(W, H, f=80.0), synthetic.sweep_pose(4)
    scene.set_proj_matrix(proj)
    scene.set_camera_view(pose)
    scene.set_object_labels(labels)
    poses = _frame_poses(2, xyz, labels)
    for k, P in poses.items():
        scene.set_object_pose(k, P)
    scene.set_object_visible(3, False)
    assert not scene.augmented()
    ogl = OGL.from_model(scene, model, FMT, (W, H))
    out = ogl.infer()['output']
    assert ogl.last_path == 'fast'
    M = camera.total_matrix(proj, pose)[0]
    oi, od = oracle_edit(xyz, labels, M, W, H, poses, hidden={3})
    texture = tex.texture_.detach().reshape(-1, N)
    fr = FrameRenderer(xyz, texture, state, W, H, proj_matrix=proj, object_labels=labels)
    for k, P in poses.items():
        fr.set_object_pose(k, P)
    fr.set_object_visible(3, False)
    ref = fr.render(pose)
    torch.cuda.synchronize()
    assert_frame(fr.idx, fr.depth, oi, od, "FrameRenderer")
    torch.testing.assert_close(out, ref, rtol=0, atol=1e-6)
    with torch.no_grad():
        want = unet_torch.net_and_texture_forward(state, texture.cpu().numpy()[None], oi)[0]
    assert unet_torch.psnr(out[..., :3].permute(2, 0, 1).cpu(), want) >= 120.0
    maps = MultiscaleRender(scene, FMT, (W, H), out_buffer_location='torch').render()
    for l, k in enumerate(FMT.replace(' ', '').split(',')):
        assert torch.equal(maps[k][..., 0].cpu(), torch.from_numpy(oracle.index_to_float(oi[l])))
    # a pose change reaches the next frame without a rebuild
    raster = scene.rasterizer()
    scene.set_object_pose(1, None)
    scene.set_object_visible(3, True)
    assert scene.rasterizer() is raster
    ogl.infer()
    poses.pop(1)
    oi2, _ = oracle_edit(xyz, labels, M, W, H, poses)
    idx, _ = raster.render(M, W, H, LEVELS, want_depth=False)
    assert torch.equal(idx[0][0].cpu(), torch.from_numpy(oi2[0]))
    with pytest.raises(NotImplementedError, match="xyz"):
        MultiscaleRender(scene, "uv_1d_p1, xyz_p1_ds1", (W, H), out_buffer_location='torch').render()
