"""GPU: frame annotations (read_annotate_frame, csrc/annotate.hip; PointCloudRasterizer.annotate, Scene.annotate_frame,
OGL.infer_annotated) against the NumPy model tests/annotate_model.py on the scenes of tests/annotate_cases.py.  Every comparison is
exact: the object and instance images, all twelve statistics of every instance, and the unmatched counter."""
import numpy as np
import pytest
import torch

from read_amd import annotate
from read_amd.ogl import OGL
from read_amd.raster import PointCloudRasterizer
from read_amd.render import Scene, StitchedScene
from read_amd.texture import PointTexture
from tests import annotate_cases as ac
from tests import annotate_model as am

pytestmark = pytest.mark.gpu

FMT = "uv_1d_p1, uv_1d_p1_ds1, uv_1d_p1_ds2, uv_1d_p1_ds3, uv_1d_p1_ds4"
SIZES = [(80, 48), (64, 32)]           # rows of 80 pixels are no multiple of a wave: runs end at row starts inside a wave


def build(case, cells=False):
    """The rasteriser of a case.  The own objects are the first instances of every list (as the rasteriser lists them itself); the
    rest is added.  -> (rasteriser, handles in list order)."""
    r = PointCloudRasterizer(case['xyz'], labels=case['labels'], cells=cells)
    for f in case['foreign']:
        r.add_object(f)
    K_own = 0 if case['labels'] is None else int(case['labels'].max())
    handles = list(range(K_own))
    for i, (k, P, visible) in enumerate(case['inst']):
        if i < K_own:
            assert k == i + 1 and P is None and visible
        else:
            handles.append(r.add_instance(k, P, visible))
    return r, handles


def render(r, case):
    idx, dep = r.render(case['M0'], case['W'], case['H'], 1)
    return idx[0], dep[0]


def assert_annotation(a, case, r, idx0, dep0):
    """The annotation against the model run on the frame the device drew, with the rasteriser's current list and handles."""
    W, H = case['W'], case['H']
    handles = list(r._inst.keys()) if r._inst is not None else []
    inst = r._instance_list() if r._inst is not None else []
    obj, inst_img, stats, unmatched, _ = am.annotate(case['xyz'], case['labels'], case['foreign'], inst, case['M0'], W, H,
                                                     idx0.cpu().numpy(), dep0.cpu().numpy(), np.array(handles, np.int32))
    assert a.handles == handles
    assert a.objects.shape == (H, W) and a.objects.dtype == torch.int32 and a.instances.dtype == torch.int32
    assert np.array_equal(a.objects.cpu().numpy(), obj), f"{(a.objects.cpu().numpy() != obj).sum()} object pixels differ"
    assert np.array_equal(a.instances.cpu().numpy(), inst_img), f"{(a.instances.cpu().numpy() != inst_img).sum()} instance pixels differ"
    assert np.array_equal(a.stats.cpu().numpy(), stats), (a.stats.cpu().numpy(), stats)
    assert int(a.unmatched.item()) == unmatched
    assert torch.equal(a.depth.view(torch.int32), dep0.reshape(H, W).view(torch.int32))
    return unmatched


def assert_frame_is_the_models(case, idx0, dep0):
    assert np.array_equal(idx0.cpu().numpy().reshape(case['H'], case['W']), case['idx'])
    assert np.array_equal(dep0.cpu().numpy().reshape(case['H'], case['W']).view(np.uint32), case['depth'].view(np.uint32))


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("name", ["edited", "unlabelled", "seventy"])
def test_cases_equal_the_model(hip, name, W, H):
    case = getattr(ac, name)(W, H)
    r, handles = build(case)
    assert r.cells is None and handles == list(range(len(case['inst'])))
    idx0, dep0 = render(r, case)
    assert_frame_is_the_models(case, idx0, dep0)
    a = r.annotate(case['M0'], W, H, idx0, dep0)
    assert assert_annotation(a, case, r, idx0, dep0) == 0
    assert np.array_equal(a.instances.cpu().numpy(), case['won']) and np.array_equal(a.stats.cpu().numpy(), case['stats'])
    assert a.check() is a
    if name == "seventy":
        assert sum(1 for _, _, v in case['inst'] if v) > 64, "the extents walk takes three launches"
    if name == "edited":
        b = a.boxes()
        assert b[4]['visible_box'] is None and b[4]['amodal_box'] is None and b[4]['n_pts'] == 500 and b[4]['truncation'] == 1.0
        assert 0.0 < b[6]['truncation'] < 1.0 and b[6]['amodal_box'][0] == 0 and b[0]['truncation'] == 0.0
        x0, y0, x1, y1 = b[5]['visible_box']
        ax0, ay0, ax1, ay1 = b[5]['amodal_box']
        assert ax0 <= x0 <= x1 <= ax1 and ay0 <= y0 <= y1 <= ay1 and 0.0 < b[5]['nearest_depth'] < 1.0


def test_caller_values_through_the_c_entry(hip):
    """read_annotate_frame with values of the caller's choosing (10..16) in place of the handles."""
    W, H = 80, 48
    case = ac.edited(W, H)
    r, _ = build(case)
    idx0, dep0 = render(r, case)
    lst = r._instance_list()
    a = annotate.annotate_frame(r.xyz, r.labels, 2, [(case['xyz'].shape[0], 400, r._ranges[2][0])], r._pool_xyz,
                                [r._ranges[k - 1][0] for k, _, _ in lst], [r._ranges[k - 1][1] for k, _, _ in lst],
                                [k for k, _, _ in lst], r.instance_matrices(case['M0']), [v for _, _, v in lst], case['values'],
                                W, H, idx0, dep0)
    assert np.array_equal(a.instances.cpu().numpy(), case['inst_img']) and a.handles == [10, 11, 12, 13, 14, 15, 16]
    assert np.array_equal(a.objects.cpu().numpy(), case['obj']) and np.array_equal(a.stats.cpu().numpy(), case['stats'])
    assert int(a.unmatched.item()) == 0


def test_frame_from_the_cell_path(hip):
    """2^20 + 50 000 static points at 256x128: the static part takes the cell route, the instances join after its pass B."""
    W, H = 256, 128
    case = ac.edited(W, H, (1 << 20) + 50_000)
    r, _ = build(case, cells=True)
    assert r.cells is not None and r.n_static >= 1 << 20
    idx0, dep0 = render(r, case)
    assert_frame_is_the_models(case, idx0, dep0)
    a = r.annotate(case['M0'], W, H, idx0, dep0)
    assert assert_annotation(a, case, r, idx0, dep0) == 0
    assert np.array_equal(a.stats.cpu().numpy(), case['stats'])


@pytest.mark.parametrize("route", ["ranges", "plain"])
def test_no_instances(hip, route):
    W, H = 80, 48
    case = ac.no_instances(W, H)
    r = PointCloudRasterizer(case['xyz'], cells=False)
    if route == "ranges":
        r._as_range_list()                                   # an empty instance list through read_splat_forward_instances
        assert r._inst == {}
    idx0, dep0 = render(r, case)
    assert_frame_is_the_models(case, idx0, dep0)
    a = r.annotate(case['M0'], W, H, idx0, dep0)
    assert assert_annotation(a, case, r, idx0, dep0) == 0
    assert a.stats.shape == (0, 12) and a.boxes() == {} and bool((a.instances == -1).all())
    assert set(np.unique(a.objects.cpu().numpy())) == {-1, 0}


def test_the_next_annotation_follows_the_edits(hip):
    W, H = 80, 48
    case = ac.edited(W, H)
    r, hs = build(case)
    r.set_instance_pose(hs[2], ac.translation((6.0, 2.0, 3.0)))          # the twins part: instance 3 now wins pixels of its own
    r.set_instance_visible(hs[4], True)                                   # the hidden one shows
    r.set_instance_visible(hs[5], False)
    idx0, dep0 = render(r, case)
    a = r.annotate(case['M0'], W, H, idx0, dep0)
    assert assert_annotation(a, case, r, idx0, dep0) == 0
    st = a.stats.cpu().numpy()
    assert st[3, am.VIS_PX] > 0 and st[4, am.VIS_PX] > 0 and np.array_equal(st[5], am.empty_row(400))
    r.remove_instance(hs[2])
    idx0, dep0 = render(r, case)
    a = r.annotate(case['M0'], W, H, idx0, dep0)
    assert a.handles == [0, 1, 3, 4, 5, 6] and a.stats.shape == (6, 12)
    assert assert_annotation(a, case, r, idx0, dep0) == 0
    assert 2 not in np.unique(a.instances.cpu().numpy()) and 3 in np.unique(a.instances.cpu().numpy())
    assert set(a.boxes()) == {0, 1, 3, 4, 5, 6}


def test_a_mismatched_list_is_counted(hip):
    """Annotating with a pose other than the frame's: the moved instance's pixels match nothing — a counter, and check() raises."""
    W, H = 80, 48
    case = ac.edited(W, H)
    r, hs = build(case)
    idx0, dep0 = render(r, case)
    r.set_instance_pose(hs[5], ac.translation((-1.0, -1.25, -12.0)))
    a = r.annotate(case['M0'], W, H, idx0, dep0)
    unmatched = assert_annotation(a, case, r, idx0, dep0)
    assert unmatched == case['stats'][5, am.VIS_PX] > 0
    with pytest.raises(RuntimeError, match=f"{unmatched} pixels match no instance"):
        a.check()
    with pytest.raises(NotImplementedError, match="more than one camera"):
        r.annotate(np.stack([case['M0'], case['M0']]), W, H, idx0, dep0)
    with pytest.raises(ValueError, match="idx0 must be"):
        r.annotate(case['M0'], W, H, idx0.float(), dep0)


def _scene(case):
    from read_amd import synthetic
    scene = Scene(case['xyz'])
    scene.set_proj_matrix(synthetic.make_proj(case['W'], case['H'], f=float(case['W'])))
    scene.set_camera_view(synthetic.sweep_pose(0))
    scene.set_object_labels(case['labels'])
    k = scene.add_foreign_object(case['foreign'][0], PointTexture(8, 400, init_method='rand').cuda())
    assert k == 3
    hs = [scene.add_object_instance(k_, P, v) for k_, P, v in case['inst'][2:]]
    return scene, hs


def test_scene_annotate_frame(hip):
    W, H = 80, 48
    case = ac.edited(W, H)
    scene, hs = _scene(case)
    assert np.array_equal(scene.total_matrix()[0], case['M0'])
    a = scene.annotate_frame((W, H))
    assert [scene.annotation_handle(h) for h in hs] == [2, 3, 4, 5, 6] and a.handles == list(range(7))
    assert np.array_equal(a.objects.cpu().numpy(), case['obj']) and np.array_equal(a.instances.cpu().numpy(), case['won'])
    assert np.array_equal(a.stats.cpu().numpy(), case['stats']) and np.array_equal(a.depth.cpu().numpy().view(np.uint32),
                                                                                   case['depth'].view(np.uint32))
    a.check()
    scene.set_panorama(200.0)
    with pytest.raises(NotImplementedError, match="panorama"):
        scene.annotate_frame((W, H))
    scene.set_panorama(None)
    with pytest.raises(NotImplementedError, match="StitchedScene"):
        StitchedScene([Scene(case['xyz'])]).annotate_frame((W, H))


def test_ogl_infer_annotated(hip):
    from tests.test_gpu_api import _model
    W, H = 80, 48
    case = ac.edited(W, H)
    scene, _ = _scene(case)
    model, _, _ = _model(case['xyz'].shape[0])
    ogl = OGL.from_model(scene, model, FMT, (W, H))
    want = ogl.infer()['output'].clone()
    assert ogl.last_path == 'fast'
    res = ogl.infer_annotated()
    assert set(res) == {'output', 'net_input', 'annotation'} and ogl.last_path == 'fast'
    assert torch.equal(res['output'], want), "the annotated frame is infer()'s, bit for bit"
    a = res['annotation'].check()
    assert np.array_equal(a.objects.cpu().numpy(), case['obj']) and np.array_equal(a.instances.cpu().numpy(), case['won'])
    assert np.array_equal(a.stats.cpu().numpy(), case['stats'])
    assert np.array_equal(a.depth.cpu().numpy().view(np.uint32), case['depth'].view(np.uint32))
    # the refusals, each by name
    scene.set_panorama(200.0)
    with pytest.raises(NotImplementedError, match="panorama"):
        ogl.infer_annotated()
    scene.set_panorama(None)
    scene.set_point_drop(0.25, 3)
    with pytest.raises(NotImplementedError, match="GL-twin augmentation"):
        ogl.infer_annotated()
    scene.set_point_drop(0.0)
    with pytest.raises(NotImplementedError, match="supersampling 2"):
        OGL.from_model(scene, model, FMT, (W, H), supersampling=2).infer_annotated()
    model.ss = 1
    with pytest.raises(NotImplementedError, match="temporal_average"):
        OGL.from_model(scene, model, FMT, (W, H), temporal_average=True).infer_annotated()
    model.temporal_average = False
    with pytest.raises(NotImplementedError, match="input format"):
        OGL.from_model(scene, model, "uv_1d_p1, uv_1d_p1_ds1", (W, H)).infer_annotated()
    st = StitchedScene([Scene(case['xyz'])])
    with pytest.raises(NotImplementedError, match="StitchedScene"):
        OGL.from_model(st, model, FMT, (W, H), texture_ids=[0]).infer_annotated()
    assert torch.equal(ogl.infer_annotated()['output'], want)
