"""GPU: object selection — read_select_boxes / _near / _vote / _finish and the Python layer above them against
the NumPy model (tests/select_model.py).  Every comparison is array_equal.  The inputs come from tests/select_cases.py; that they
exercise every class of the contract is checked on the CPU (tests/test_select_cpu.py)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from read_amd import _lib, camera, select, synthetic
from read_amd.ogl import OGL
from read_amd.raster import PointCloudRasterizer
from read_amd.render import Scene, StitchedScene
from tests import select_cases as sc
from tests import select_model as sm

pytestmark = pytest.mark.gpu

f32 = np.float32
FMT = "uv_1d_p1, uv_1d_p1_ds1, uv_1d_p1_ds2, uv_1d_p1_ds3, uv_1d_p1_ds4"


def _mp(M):
    return np.ascontiguousarray(M, f32).reshape(16).ctypes.data_as(C.POINTER(C.c_float))


# ---- boxes ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _box_cloud():
    return synthetic.make_cloud(max(sc.BOX_N))


@functools.lru_cache(maxsize=None)
def _box_reference(K):
    """(boxes, label_of, the model's labels of the whole cloud): labels are per point, so a prefix of the cloud has the prefix."""
    boxes, label_of = sc.random_boxes(K, 31)
    return boxes, label_of, sm.label_boxes(_box_cloud(), boxes, label_of)


@pytest.mark.parametrize("K", sc.BOX_K)
@pytest.mark.parametrize("N", sc.BOX_N)
def test_boxes_equal_the_model(hip, N, K):
    boxes, label_of, want = _box_reference(K)
    if K:
        in_a_box = (sm.label_boxes(_box_cloud(), boxes, label_of, np.full(max(sc.BOX_N), -1)) >= 0).mean() \
            if N == max(sc.BOX_N) else None
        assert in_a_box is None or 0.01 <= in_a_box <= 0.30, in_a_box
    got = select.label_boxes(_box_cloud()[:N], boxes, label_of)
    assert got.dtype == torch.int32 and got.is_cuda and tuple(got.shape) == (N,)
    assert np.array_equal(got.cpu().numpy(), want[:N])
    if K in (2, 33) and N:
        assert np.array_equal(select.label_boxes(_box_cloud()[:N], boxes).cpu().numpy(), sm.label_boxes(_box_cloud()[:N], boxes))


def test_boxes_face_exact_and_nonfinite_points(hip):
    box, pts, inside = sc.face_points()
    assert np.array_equal(select.label_boxes(pts, box).cpu().numpy(), inside.astype(np.int32))
    bad = sc.nonfinite_points()
    for b in (box, select.box_matrix((0, 0, 0), (4, 4, 4), yaw=0.7)[None]):
        assert np.array_equal(select.label_boxes(bad, b, labels=np.full(len(bad), 5)).cpu().numpy(), np.full(len(bad), 5))
        assert not select.label_boxes(bad, b).any()


def test_boxes_labels_in_out_of_place_and_in_place(hip):
    N = 100_003
    xyz = _box_cloud()[:N]
    boxes, label_of, _ = _box_reference(33)
    labels_in = np.random.default_rng(2).integers(0, 9, N).astype(np.int32)
    want = sm.label_boxes(xyz, boxes, label_of, labels_in)
    assert (want != labels_in).mean() > 0.01 and (want == labels_in).mean() > 0.5
    lab_d = torch.from_numpy(labels_in).cuda()
    got = select.label_boxes(xyz, boxes, label_of, labels=lab_d)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(lab_d.cpu().numpy(), labels_in)
    # in place, through the C entry: labels_in = labels_out
    x_d, b_d, l_d = torch.from_numpy(xyz).cuda(), torch.from_numpy(boxes).cuda(), torch.from_numpy(label_of).cuda()
    for K in (33, 0):
        buf = torch.from_numpy(labels_in).cuda()
        _lib.check(hip.read_select_boxes(x_d.data_ptr(), N, b_d.data_ptr(), l_d.data_ptr(), K, buf.data_ptr(), buf.data_ptr(),
                                         _lib.stream_ptr()), "read_select_boxes")
        assert np.array_equal(buf.cpu().numpy(), want if K else labels_in)
    # K = 0: labels_in copied, or zeros
    assert np.array_equal(select.label_boxes(xyz, np.zeros((0, 12), f32), labels=labels_in).cpu().numpy(), labels_in)
    assert not select.label_boxes(xyz, np.zeros((0, 12), f32)).any()


def test_boxes_past_the_grid_cap(hip):
    # the launch caps its grid at 8 workgroups per compute unit and strides: points past cap * 256 take a second trip
    cap = torch.cuda.get_device_properties(0).multi_processor_count * 8
    N = cap * 256 + 257
    xyz = synthetic.make_cloud(N, 12)
    boxes, label_of = sc.random_boxes(2, 31)
    want = sm.label_boxes(xyz, boxes, label_of)
    assert want[cap * 256:].any() and want[:cap * 256].any()
    assert np.array_equal(select.label_boxes(xyz, boxes, label_of).cpu().numpy(), want)


# ---- near, vote, finish ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case():
    return sc.vote_case()


@functools.lru_cache(maxsize=None)
def _case_raster():
    return PointCloudRasterizer(_case()['xyz'])


def _level0(raster, M, W, H):
    idx, dep = raster.render(M, W, H, 1)
    return idx[0].contiguous(), dep[0].contiguous()


def test_near_equals_the_model_on_the_rasterisers_own_frame(hip):
    case = _case()
    xyz, W, H = case['xyz'], case['W'], case['H']
    r = _case_raster()
    for M in case['totals'][:2]:
        idx, dep = _level0(r, M, W, H)
        near = torch.full((W * H,), -1.0, dtype=torch.float32, device='cuda')
        _lib.check(hip.read_select_near(r.xyz.data_ptr(), r.n, _mp(M), W, H, idx.data_ptr(), dep.data_ptr(), near.data_ptr(),
                                        _lib.stream_ptr()), "read_select_near")
        want = sm.near_image(xyz, M, idx.cpu().numpy(), dep.cpu().numpy())
        assert np.isposinf(want).sum() > 100 and np.isfinite(want).sum() > 1000          # sky and street
        assert np.array_equal(near.cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_votes_equal_the_model_after_every_view_and_finish(hip):
    case = _case()
    xyz, W, H = case['xyz'], case['W'], case['H']
    r = _case_raster()
    votes = select.MaskVotes(r.xyz)
    state = np.zeros(len(xyz), np.uint32)
    assert votes.n_views == 0 and not votes.state.any()
    for v, (M, mask) in enumerate(zip(case['totals'], case['masks'])):
        idx, dep = _level0(r, M, W, H)
        near = sm.near_image(xyz, M, idx.cpu().numpy(), dep.cpu().numpy())
        state = sm.vote(state, xyz, M, W, H, near, mask, sm.scale_of(case['rel']), f32(case['slack']))
        votes.add_view(M, W, H, idx, dep, mask, case['rel'], case['slack'])
        assert votes.n_views == v + 1
        assert np.array_equal(votes.state.cpu().numpy().view(np.uint32), state), f"state after view {v}"
    assert len(np.unique(state)) > 10
    labels_in = np.random.default_rng(3).integers(0, 5, len(xyz)).astype(np.int32)
    for min_hits, ratio in ((1, (0, 1)), (2, (1, 2)), (3, (1, 1))):
        want = sm.finish(state, min_hits, ratio)
        assert np.array_equal(votes.labels(min_hits, ratio).cpu().numpy(), want), (min_hits, ratio)
        assert np.array_equal(votes.labels(min_hits, ratio, labels=labels_in).cpu().numpy(),
                              sm.finish(state, min_hits, ratio, labels_in)), (min_hits, ratio)
    n = select.counts(votes.labels(case['min_hits'], case['ratio']))
    assert n.dtype == np.int64 and n.tolist() == np.bincount(sm.finish(state, case['min_hits'], case['ratio'])).tolist()
    assert n[1] >= 500 and n[2] >= 500 and len(n) == 3


def test_vote_at_the_big_viewport(hip):
    W, H = 1216, 352
    case = sc.vote_case(W, H, n_views=1)
    xyz, M, mask = case['xyz'], case['totals'][0], case['masks'][0]
    r = _case_raster()
    idx, dep = _level0(r, M, W, H)
    near = sm.near_image(xyz, M, idx.cpu().numpy(), dep.cpu().numpy())
    want = sm.vote(np.zeros(len(xyz), np.uint32), xyz, M, W, H, near, mask, sm.scale_of(case['rel']), f32(case['slack']))
    pix = sm.project(xyz, M, W, H)
    assert pix.max() > 64 * 48 * 100 and (want >> 16 == 1).sum() > 500 and (want >> 16 == 2).sum() > 500
    votes = select.MaskVotes(r.xyz)
    votes.add_view(M, W, H, idx, dep, mask, case['rel'], case['slack'])
    assert np.array_equal(votes.state.cpu().numpy().view(np.uint32), want)


# ---- end to end: a built scene ---------------------------------------------------------------------------------------------------------------
def _car_scene(W, H, f):
    xyz, is_car = sc.car_scene()
    scene = Scene(xyz)
    scene.set_proj_matrix(synthetic.make_proj(W, H, f=f))
    scene.set_camera_view(synthetic.sweep_pose(0))
    return scene, xyz, is_car


def test_scene_select_boxes_then_hide_the_car(hip):
    from tests.test_gpu_api import _model
    W, H = 128, 64
    scene, xyz, is_car = _car_scene(W, H, 80.0)
    model, _, _ = _model(len(xyz))
    plain = OGL.from_model(scene, model, FMT, (W, H)).infer()['output'].clone()
    n = scene.select_boxes(sc.car_box()[None])
    assert n.tolist() == [int((~is_car).sum()), int(is_car.sum())]
    assert np.array_equal(scene.object_labels != 0, is_car)                          # exactly the car's ids
    ogl = OGL.from_model(scene, model, FMT, (W, H))
    shown = ogl.infer()['output']
    assert ogl.last_path == 'fast' and torch.equal(shown, plain)                     # everything visible: the unlabelled frame
    car_ids = torch.from_numpy(np.flatnonzero(is_car)).cuda()
    idx, _ = scene.rasterizer().render(scene.total_matrix(), W, H, 5, want_depth=False)
    assert int(torch.isin(idx[0], car_ids).sum()) > 50
    scene.set_object_visible(1, False)
    hidden = ogl.infer()['output']
    assert ogl.last_path == 'fast' and not torch.equal(hidden, plain)
    idx, _ = scene.rasterizer().render(scene.total_matrix(), W, H, 5, want_depth=False)      # the id pyramid infer() gathered from
    for l in range(5):
        assert not bool(torch.isin(idx[l], car_ids).any()), f"a car id at level {l}"
    # keep: a second box adds label 2 without losing label 1
    n = scene.select_boxes(select.box_matrix((0, 1.0, -20.0), (4, 2, 1))[None], label_of=[2], keep=True)
    assert n[1] == int(is_car.sum()) and n[2] > 0 and n.sum() == len(xyz)


def test_scene_select_masks_from_two_views(hip):
    W, H = 256, 128
    scene, xyz, is_car = _car_scene(W, H, 160.0)
    views = [synthetic.sweep_pose(0), synthetic.sweep_pose(8)]
    r = PointCloudRasterizer(xyz)
    state = np.zeros(len(xyz), np.uint32)
    masks, winners = [], np.zeros(len(xyz), bool)
    for view in views:
        M = scene.total_matrix(view)[0].reshape(16)
        assert np.array_equal(M, camera.total_matrix(scene.proj_matrix, view)[0].reshape(16))
        idx, dep = (t.cpu().numpy().reshape(H, W) for t in _level0(r, M, W, H))
        covered = (idx != 0) | (dep.view(np.uint32) != 0)
        masks.append((covered & is_car[idx]).astype(np.int32))                       # "the winner is a car point"
        winners[idx[masks[-1] != 0]] = True
        near = sm.near_image(xyz, M, idx, dep)
        state = sm.vote(state, xyz, M, W, H, near, masks[-1], sm.scale_of(0.05), f32(0.0))
    assert masks[0].sum() > 200 and masks[1].sum() > 200
    n = scene.select_masks(views, masks, (W, H))
    want = sm.finish(state, 1, (1, 2))
    assert np.array_equal(scene.object_labels, want) and n.tolist() == np.bincount(want).tolist()
    assert winners.sum() > 200 and (want[winners] == 1).all()                        # every car point that won a pixel
    # the labels are live: hiding the object removes its winners from the frame
    scene.set_object_visible(1, False)
    idx, _ = scene.rasterizer().render(scene.total_matrix(), W, H, 1, want_depth=False)
    assert not bool(torch.isin(idx[0], torch.from_numpy(np.flatnonzero(want == 1)).cuda()).any())
    # an edited scene renders its views through a temporary unlabelled rasteriser: the same labels again
    n2 = scene.select_masks(views, masks, (W, H))
    assert np.array_equal(scene.object_labels, want) and n2.tolist() == n.tolist()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_refusals(hip):
    W, H = 64, 48
    scene, xyz, _ = _car_scene(W, H, 48.0)
    mask = np.zeros((H, W), np.int32)
    view = synthetic.sweep_pose(0)
    scene.set_panorama(120.0)
    with pytest.raises(NotImplementedError, match="panorama"):
        scene.select_masks([view], [mask], (W, H))
    scene.set_panorama(None)
    scene.set_point_discard(np.zeros(len(xyz), bool))
    with pytest.raises(NotImplementedError, match="augmentation"):
        scene.select_masks([view], [mask], (W, H))
    scene.set_point_discard(None)
    stitched = StitchedScene([scene])
    with pytest.raises(NotImplementedError, match="StitchedScene"):
        stitched.select_boxes(sc.car_box()[None])
    with pytest.raises(NotImplementedError, match="StitchedScene"):
        stitched.select_masks([view], [mask], (W, H))
    # K = 1025: in Python and at the C entry
    with pytest.raises(ValueError, match="1024"):
        select.label_boxes(xyz, np.zeros((1025, 12), f32))
    x_d = torch.from_numpy(xyz).cuda()
    out = torch.zeros(len(xyz), dtype=torch.int32, device='cuda')
    rc = hip.read_select_boxes(x_d.data_ptr(), len(xyz), x_d.data_ptr(), out.data_ptr(), 1025, None, out.data_ptr(), None)
    assert rc == -22 and "read_select_boxes" in hip.read_last_error().decode()
    with pytest.raises(ValueError, match="label_of"):
        select.label_boxes(xyz, sc.car_box()[None], label_of=[select.MAX_LABEL + 1])
    # masks out of range or shape; the 256th view
    small = xyz[:1000]
    r = PointCloudRasterizer(small)
    M = scene.total_matrix(view)[0]
    idx, dep = _level0(r, M, W, H)
    votes = select.MaskVotes(r.xyz)
    for bad in (np.full((H, W), select.MAX_LABEL + 1), np.full((H, W), -1), np.zeros((W, H), np.int32), np.zeros((H, W), f32)):
        with pytest.raises(ValueError, match="mask"):
            votes.add_view(M, W, H, idx, dep, bad)
    assert votes.n_views == 0 and not votes.state.any()
    for _ in range(255):
        votes.add_view(M, W, H, idx, dep, mask)
    assert votes.n_views == 255 and int(votes.state.max()) == 255                    # seen in every view, never named
    with pytest.raises(ValueError, match="255"):
        votes.add_view(M, W, H, idx, dep, mask)
    assert int(votes.state.max()) == 255
