"""GPU: frame flow (read_flow_frame, csrc/flow.hip; PointCloudRasterizer.frame_state / flow, Scene.capture_frame / flow_between,
OGL.infer_tracked) against the NumPy model tests/flow_model.py on the state pairs of tests/flow_cases.py.  Every comparison is
exact: flow and depth_next as uint32 bit patterns, the state image, the eight counts, all four statistics of every instance, and the
unmatched counter.  No tolerance anywhere: model and kernel perform the same fp32 operations in the same order."""
import numpy as np
import pytest
import torch

from read_amd import flow
from read_amd.ogl import OGL
from read_amd.raster import PointCloudRasterizer
from read_amd.render import Scene, StitchedScene
from read_amd.texture import PointTexture
from tests import annotate_cases as ac
from tests import flow_cases as fc
from tests import flow_model as fm

pytestmark = pytest.mark.gpu

FMT = "uv_1d_p1, uv_1d_p1_ds1, uv_1d_p1_ds2, uv_1d_p1_ds3, uv_1d_p1_ds4"
SIZES = fc.SIZES


def build(case, cells=False):
    """The rasteriser of a case in state A.  The own objects are the first instances of every list (as the rasteriser lists them
    itself); the rest is added.  -> (rasteriser, handles in list order)."""
    r = PointCloudRasterizer(case['xyz'], labels=case['labels'], cells=cells)
    for f in case['foreign']:
        r.add_object(f)
    K_own = 0 if case['labels'] is None else int(case['labels'].max())
    handles = list(range(K_own))
    for i, (k, P, visible) in enumerate(case['inst_a']):
        if i < K_own:
            assert k == i + 1 and P is None and visible
        else:
            handles.append(r.add_instance(k, P, visible))
    return r, handles


def to_state_b(r, handles, case):
    K_own = 0 if case['labels'] is None else int(case['labels'].max())
    for i, (k, P, visible) in enumerate(case['inst_b']):
        if i < K_own:
            r.set_object_pose(k, P)
            r.set_object_visible(k, visible)
        else:
            r.set_instance_pose(handles[i], P)
            r.set_instance_visible(handles[i], visible)


def capture(r, M0, W, H):
    idx, dep = r.render(M0, W, H, 1)
    return r.frame_state(M0, W, H, idx[0], dep[0])


def states(case, cells=False):
    r, hs = build(case, cells)
    sa = capture(r, case['M0_a'], case['W'], case['H'])
    to_state_b(r, hs, case)
    sb = capture(r, case['M0_b'], case['W'], case['H'])
    return r, hs, sa, sb


def assert_frames_are_the_models(case, sa, sb):
    H, W = case['H'], case['W']
    for s, idx, dep in ((sa, case['idx_a'], case['depth_a']), (sb, case['idx_b'], case['depth_b'])):
        assert np.array_equal(s.idx0.cpu().numpy().reshape(H, W), idx)
        assert np.array_equal(s.depth0.cpu().numpy().reshape(H, W).view(np.uint32), dep.view(np.uint32))


def assert_equal(f, out, handles=None):
    """A FrameFlow against a model result, bit for bit."""
    H, W = out['state'].shape
    assert f.flow.shape == (H, W, 2) and f.flow.dtype == torch.float32 and f.state.dtype == torch.int32
    assert f.depth_next.shape == (H, W) and f.counts.shape == (8,) and f.stats.shape == out['stats'].shape
    st = f.state.cpu().numpy()
    assert np.array_equal(st, out['state']), f"{(st != out['state']).sum()} state pixels differ"
    got = f.flow.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, out['flow'].view(np.uint32)), f"{(got != out['flow'].view(np.uint32)).sum()} flow words differ"
    assert np.array_equal(f.depth_next.cpu().numpy().view(np.uint32), out['depth_next'].view(np.uint32))
    assert np.array_equal(f.counts.cpu().numpy(), out['counts']), (f.counts.cpu().numpy(), out['counts'])
    assert np.array_equal(f.stats.cpu().numpy(), out['stats']), (f.stats.cpu().numpy(), out['stats'])
    assert int(f.unmatched.item()) == out['unmatched']
    if handles is not None:
        assert f.handles == handles


def model_on_device_frames(case, inst_a, inst_b, M0_a, M0_b, sa, sb):
    return fm.flow(case['xyz'], case['labels'], case['foreign'], inst_a, inst_b, M0_a, M0_b, case['W'], case['H'],
                   sa.idx0.cpu().numpy(), sa.depth0.cpu().numpy(), sb.idx0.cpu().numpy(), sb.depth0.cpu().numpy())


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", ["moved", "foreign_moves", "identity", "one_moved_instance"])
def test_cases_equal_the_model(hip, name, W, H):
    case = getattr(fc, name)(W, H)
    r, hs, sa, sb = states(case)
    assert r.cells is None and hs == list(range(len(case['inst_a'])))
    assert_frames_are_the_models(case, sa, sb)
    f = r.flow(sa, sb)
    assert_equal(f, case['out'], hs)
    assert f.check() is f
    if name == "moved":
        s = f.summary()
        assert s['counts']['hidden'] == case['out']['counts'][fm.HIDDEN] > 0 and s['counts']['unmatched'] == 0
        assert s['instances'][5] == {'px': s['counts']['hidden'], 'visible': 0, 'occluded': 0, 'outside': 0}
        assert s['instances'][1]['outside'] == s['instances'][1]['px'] > 0 and set(s['instances']) == set(hs)
    if name == "identity":
        assert not bool(f.flow.view(torch.int32).any()), "B = A: the flow's bits are 0"
        filled = f.state == flow.VISIBLE
        assert torch.equal(f.depth_next.view(torch.int32)[filled], sa.depth0.reshape(H, W).view(torch.int32)[filled])


@pytest.mark.parametrize("W,H", SIZES)
def test_count_zero(hip, W, H):
    """A plain cloud (no list at all), the same as an empty range list, and count = 0 through the C entry on a frame that has objects:
    object pixels are UNMATCHED, static pixels still flow."""
    case = fc.no_instances(W, H)
    for as_ranges in (False, True):
        r = PointCloudRasterizer(case['xyz'], cells=False)
        if as_ranges:
            r._as_range_list()
        sa, sb = capture(r, case['M0_a'], W, H), capture(r, case['M0_b'], W, H)
        assert_frames_are_the_models(case, sa, sb)
        f = r.flow(sa, sb)
        assert_equal(f, case['out'], [])
        assert f.stats.shape == (0, 4) and f.summary()['instances'] == {} and f.check() is f
    case = fc.moved(W, H)
    r, hs, sa, sb = states(case)
    f = flow.flow_frames(r.xyz, r.labels, 2, [(case['xyz'].shape[0], 400, r._ranges[2][0])], r._pool_xyz, [], [],
                         np.zeros((0, 16), np.float32), [], np.zeros((0, 16), np.float32), [], case['M0_a'], case['M0_b'], W, H,
                         sa.idx0, sa.depth0, sb.idx0, sb.depth0)
    out = fm.flow(case['xyz'], case['labels'], case['foreign'], [], [], case['M0_a'], case['M0_b'], W, H, case['idx_a'], case['depth_a'],
                  case['idx_b'], case['depth_b'])
    assert out['unmatched'] == (case['out']['won'] >= 0).sum() > 0
    assert_equal(f, out, [])
    with pytest.raises(RuntimeError, match=f"{out['unmatched']} pixels match no drawer"):
        f.check()


def test_frames_from_the_cell_path(hip):
    """2^20 + 50 000 static points at 256x128: the static part of both frames takes the cell route."""
    W, H = 256, 128
    case = fc.moved(W, H, (1 << 20) + 50_000)
    r, hs, sa, sb = states(case, cells=True)
    assert r.cells is not None and r.n_static >= 1 << 20
    assert_frames_are_the_models(case, sa, sb)
    assert_equal(r.flow(sa, sb), case['out'], hs)


def test_a_frame_of_more_pixels_than_one_turn(hip):
    """600x300 = 180 000 pixels: the pixel pass's 512 workgroups take a second, partly filled turn; static and object pixels lie in it."""
    case = fc.wide()
    r, hs, sa, sb = states(case)
    assert_frames_are_the_models(case, sa, sb)
    assert_equal(r.flow(sa, sb), case['out'], hs)


def test_a_mismatched_list_is_counted(hip):
    """State A taken with another pose than its frame was drawn with: the moved instance's pixels find no drawer — a counter, the
    UNMATCHED state, and check() raises."""
    W, H = 80, 48
    case = fc.moved(W, H)
    r, hs = build(case)
    idx, dep = r.render(case['M0_a'], W, H, 1)
    inst_a, inst_b = fc.mismatched(case)
    r.set_instance_pose(hs[5], inst_a[5][1])
    sa = r.frame_state(case['M0_a'], W, H, idx[0], dep[0])
    to_state_b(r, hs, case)
    sb = capture(r, case['M0_b'], W, H)
    f = r.flow(sa, sb)
    out = model_on_device_frames(case, inst_a, inst_b, case['M0_a'], case['M0_b'], sa, sb)
    assert out['unmatched'] == case['out']['stats'][5, fm.PX] > 0
    assert_equal(f, out, hs)
    assert int((f.state == flow.UNMATCHED).sum().item()) == out['unmatched']
    with pytest.raises(RuntimeError, match=f"{out['unmatched']} pixels match no drawer"):
        f.check()


def test_refresh_after_rendering_into_the_same_tensors(hip):
    W, H = 75, 37
    case = fc.moved(W, H)
    r, hs, sa, sb = states(case)
    f = r.flow(sa, sb)
    assert_equal(f, case['out'], hs)
    # state B's frame is overwritten by state A's, in place: refresh() sees what the tensors hold now
    for t in (f.flow, f.depth_next, f.state, f.counts, f.stats, f.unmatched):
        t.fill_(77)
    to_state_b(r, hs, dict(case, inst_b=case['inst_a']))
    r.render(case['M0_a'], W, H, 1, out=([sb.idx0], [sb.depth0]))
    assert torch.equal(sb.idx0, sa.idx0) and f.refresh() is f
    out = model_on_device_frames(case, case['inst_a'], case['inst_b'], case['M0_a'], case['M0_b'], sa, sb)
    assert out['counts'][fm.OCCLUDED] != case['out']['counts'][fm.OCCLUDED]
    assert_equal(f, out, hs)
    # and back: B's own frame into the same tensors
    to_state_b(r, hs, case)
    r.render(case['M0_b'], W, H, 1, out=([sb.idx0], [sb.depth0]))
    assert_equal(f.refresh(), case['out'], hs)


def test_states_that_do_not_belong_together_are_refused(hip):
    W, H = 64, 32
    case = fc.moved(W, H)
    r, hs, sa, sb = states(case)
    other, _, oa, _ = states(case)
    with pytest.raises(ValueError, match="different rasterisers"):
        r.flow(sa, oa)
    with pytest.raises(ValueError, match="different rasterisers"):
        other.flow(sa, sb)
    with pytest.raises(NotImplementedError, match="more than one camera"):
        r.frame_state(np.stack([case['M0_a'], case['M0_a']]), W, H, sa.idx0, sa.depth0)
    with pytest.raises(ValueError, match="idx0 must be"):
        r.frame_state(case['M0_a'], W, H, sa.idx0.float(), sa.depth0)
    with pytest.raises(ValueError, match="differ in size"):
        r.flow(sa, capture(r, case['M0_b'], W, H + 1))
    r.add_object(case['foreign'][0])                             # the pool grows: ids of a later state mean something else
    with pytest.raises(ValueError, match="pool or the object count changed"):
        r.flow(sa, capture(r, case['M0_b'], W, H))
    assert r.flow(sa, sb).check().handles == hs                  # the two old states still belong together


def _scene(case):
    from read_amd import synthetic
    scene = Scene(case['xyz'])
    scene.set_proj_matrix(synthetic.make_proj(case['W'], case['H'], f=float(case['W'])))
    scene.set_camera_view(synthetic.sweep_pose(0))
    scene.set_object_labels(case['labels'])
    k = scene.add_foreign_object(case['foreign'][0], PointTexture(8, 400, init_method='rand').cuda())
    assert k == 3
    hs = [scene.add_object_instance(k_, P, v) for k_, P, v in case['inst_a'][2:]]
    return scene, hs


def _edit_scene(scene, hs, case):
    """State B of ``moved`` through the scene's own setters, with instance 6 removed and a new instance added on top."""
    from read_amd import synthetic
    T = np.eye(4)
    T[:3, 3] = fc.CAMERA_STEP
    scene.set_camera_view((T @ synthetic.sweep_pose(0).astype(np.float64)).astype(np.float32))
    b = list(case['inst_b'])
    scene.set_object_pose(1, b[0][1])
    scene.set_object_pose(2, b[1][1])
    scene.set_instance_pose(hs[0], b[2][1])
    scene.set_instance_visible(hs[3], False)
    scene.remove_instance(hs[4])
    b[6] = (b[6][0], b[6][1], False)                             # a removed instance is hidden in B
    scene.add_object_instance(1, ac.translation((2.0, 1.0, 6.0)))        # drawn in B only: it covers, it has no row
    return b


def test_scene_capture_frame_and_flow_between(hip):
    W, H = 80, 48
    case = fc.moved(W, H)
    scene, hs = _scene(case)
    assert np.array_equal(scene.total_matrix()[0], case['M0_a'])
    sa = scene.capture_frame((W, H))
    assert sa.handles == list(range(7)) and [scene.annotation_handle(h) for h in hs] == [2, 3, 4, 5, 6]
    inst_b = _edit_scene(scene, hs, case)
    sb = scene.capture_frame((W, H))
    assert sb.handles == [0, 1, 2, 3, 4, 5, 7] and sb.raster is sa.raster
    f = scene.flow_between(sa, sb)
    out = model_on_device_frames(case, case['inst_a'], inst_b, sa.M0, sb.M0, sa, sb)
    assert_equal(f, out, list(range(7)))
    f.check()
    s = f.summary()['instances']
    assert s[6]['px'] > 0 and s[6]['visible'] + s[6]['occluded'] + s[6]['outside'] == 0, "the removed instance is hidden in B"
    assert s[5]['px'] > 0 and s[5]['visible'] == 0 and out['counts'][fm.HIDDEN] == s[5]['px'] + s[6]['px']
    assert out['counts'][fm.VISIBLE] > fc.MIN_PIXELS and out['counts'][fm.CLIPPED] > fc.MIN_PIXELS
    # the other direction serves what B newly shows
    back = scene.flow_between(sb, sa)
    assert back.handles == sb.handles and back.check() is back and int(back.counts.sum().item()) == W * H
    # a rebuild of the rasteriser between two states is refused
    scene.set_object_labels(case['labels'])
    with pytest.raises(ValueError, match="different rasterisers"):
        scene.flow_between(sa, scene.capture_frame((W, H)))
    # the refusals, each by name
    with pytest.raises(NotImplementedError, match="level 1 with capture_frame"):
        scene.capture_frame((W, H), level=1)
    scene.set_panorama(200.0)
    with pytest.raises(NotImplementedError, match="panorama.*capture_frame"):
        scene.capture_frame((W, H))
    scene.set_panorama(None)
    scene.set_lens(0, (0.1, 0.0, 0.0, 0.0, 0.0))
    with pytest.raises(NotImplementedError, match="lens.*capture_frame"):
        scene.capture_frame((W, H))
    scene.set_lens(None)
    scene.set_point_drop(0.25, 3)
    with pytest.raises(NotImplementedError, match="GL-twin augmentation.*capture_frame"):
        scene.capture_frame((W, H))
    scene.set_point_drop(0.0)
    st = StitchedScene([Scene(case['xyz'])])
    with pytest.raises(NotImplementedError, match="capture_frame on a StitchedScene"):
        st.capture_frame((W, H))
    with pytest.raises(NotImplementedError, match="flow_between on a StitchedScene"):
        st.flow_between(sa, sb)


def test_ogl_infer_tracked(hip):
    from tests.test_gpu_api import _model
    W, H = 80, 48
    case = fc.moved(W, H)
    scene, hs = _scene(case)
    model, _, _ = _model(case['xyz'].shape[0])
    ogl = OGL.from_model(scene, model, FMT, (W, H))
    want = ogl.infer()['output'].clone()
    assert ogl.last_path == 'fast'
    res = ogl.infer_tracked()
    assert set(res) == {'output', 'net_input', 'state'} and ogl.last_path == 'fast'
    assert torch.equal(res['output'], want), "the tracked frame is infer()'s, bit for bit"
    sa = res['state']
    assert np.array_equal(sa.idx0.cpu().numpy().reshape(H, W), case['idx_a'])
    inst_b = _edit_scene(scene, hs, case)
    want_b = ogl.infer()['output'].clone()
    res_b = ogl.infer_tracked()
    assert torch.equal(res_b['output'], want_b) and not torch.equal(want_b, want)
    sb = res_b['state']
    f = scene.flow_between(sa, sb).check()
    assert_equal(f, model_on_device_frames(case, case['inst_a'], inst_b, sa.M0, sb.M0, sa, sb), list(range(7)))
    # the refusals, each by name
    scene.set_panorama(200.0)
    with pytest.raises(NotImplementedError, match="panorama.*infer_tracked"):
        ogl.infer_tracked()
    scene.set_panorama(None)
    scene.set_lens(0, (0.1, 0.0, 0.0, 0.0, 0.0))
    with pytest.raises(NotImplementedError, match="lens.*infer_tracked"):
        ogl.infer_tracked()
    scene.set_lens(None)
    scene.set_point_drop(0.25, 3)
    with pytest.raises(NotImplementedError, match="GL-twin augmentation.*infer_tracked"):
        ogl.infer_tracked()
    scene.set_point_drop(0.0)
    with pytest.raises(NotImplementedError, match="supersampling 2.*infer_tracked"):
        OGL.from_model(scene, model, FMT, (W, H), supersampling=2).infer_tracked()
    model.ss = 1
    with pytest.raises(NotImplementedError, match="temporal_average.*infer_tracked"):
        OGL.from_model(scene, model, FMT, (W, H), temporal_average=True).infer_tracked()
    model.temporal_average = False
    with pytest.raises(NotImplementedError, match="input format.*infer_tracked"):
        OGL.from_model(scene, model, "uv_1d_p1, uv_1d_p1_ds1", (W, H)).infer_tracked()
    stitched = StitchedScene([Scene(case['xyz'])])
    with pytest.raises(NotImplementedError, match="infer_tracked.*StitchedScene"):
        OGL.from_model(stitched, model, FMT, (W, H), texture_ids=[0]).infer_tracked()
    assert torch.equal(ogl.infer_tracked()['output'], want_b)
