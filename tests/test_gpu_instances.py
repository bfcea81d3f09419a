"""GPU: scene editing's third verb, add — instances of labelled objects and objects from other scenes on the fast render path.

The contract (read_splat_forward_instances; tests/instances_model.py): instance i draws a range of one point pool with
M_i = object_matrix(M_0, P_i); per pixel the minimum of depth bits << 32 | id wins over every visible point of every visible
instance and the static part; a foreign object's ids follow the scene's.  The oracle is oracle.raster_multiscale per instance,
merged on the key.  Every comparison of index and depth images is exact (torch.equal on the ids and on the depth bit patterns, all
5 levels)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import oracle
from oracle import unet_torch
from read_amd import _lib, camera, synthetic
from read_amd.camera import level_sizes
from read_amd.frame import FrameRenderer
from read_amd.ogl import OGL
from read_amd.raster import PointCloudRasterizer, build_cells_device, label_layout, object_matrix
from read_amd.render import Scene
from read_amd.stitch import StitchedRasterizer
from read_amd.texture import PointTexture, gather_pyramid, gather_tables_pyramid
from read_amd.unet import default_layout, pack_state, weight_spec
from tests import instances_model as im
from tests import stitch_model as sm

pytestmark = pytest.mark.gpu

LEVELS = 5
FMT = "uv_1d_p1, uv_1d_p1_ds1, uv_1d_p1_ds2, uv_1d_p1_ds3, uv_1d_p1_ds4"
W, H = 1216, 352


# ---- helpers (the pattern of tests/test_gpu_objects.py) ------------------------------------------------------------------------
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


@functools.lru_cache(maxsize=None)
def _cloud(name):
    """-> (xyz, labels): 6 clusters of 5 000 points in a 200 000-point cloud (the route without cells) or in a 1 200 000-point
    street cloud (the static part above 2^20 points: the cell route)."""
    xyz = synthetic.make_street_cloud(1_200_000, 5) if name == "street" else synthetic.make_cloud(200_000, 6)
    return xyz, cluster_labels(xyz, 6, 5_000, 11)


def _four_poses(xyz, labels, k, view, proj):
    """Object k rotated about its centre, translated, behind the camera, straddling the left image edge."""
    c = xyz[labels == k].astype(np.float64).mean(0)
    return [about(c, rot_z(0.6), (0.0, 0.0, 0.0)),
            translation(camera_space_target(view, proj, 0.3, 7.0) - c),
            translation(camera_space_target(view, proj, 0.0, 10.0, behind=True) - c),
            translation(camera_space_target(view, proj, -1.0, 12.0) - c)]


def _instance_list(r):
    """The rasteriser's current list in the model's form [(first, npts, P, visible)]."""
    return [(r._ranges[k - 1][0], r._ranges[k - 1][1], P, v) for k, P, v in r._instance_list()]


# ---- 1. the partition listed once equals read_splat_forward_objects, both routes --------------------------------------------------
class _ForwardObjects:
    """read_splat_forward_objects called directly, as a C caller would: the partition of ``label_layout`` in a hand-built
    read_splat_objects, a cell blob of the static part when it is large enough, a workspace of its own."""

    def __init__(self, xyz, labels, W, H):
        L, dev = _lib.lib(), torch.device("cuda")
        pts = torch.from_numpy(xyz).to(dev)
        self.static_ids, self.obj_ids, self.begin = label_layout(torch.from_numpy(labels).to(dev))
        self.static_xyz = pts[self.static_ids.long()].contiguous()
        self.obj_xyz = pts[self.obj_ids.long()].contiguous()
        self.n_static, self.K = int(self.static_ids.numel()), len(self.begin) - 1
        self.cells = None
        if self.n_static >= (1 << 20):
            self.cells = build_cells_device(self.static_xyz, ids=self.static_ids)
            _lib.check(L.read_splat_cells_invalidate(self.cells.data_ptr(), self.n_static), "read_splat_cells_invalidate")
        self.W, self.H = W, H
        self.ws = torch.empty(L.read_splat_workspace_bytes(1, W, H), dtype=torch.uint8, device=dev)
        _lib.check(L.read_splat_workspace_init(self.ws.data_ptr(), self.ws.numel(), _lib.stream_ptr()), "read_splat_workspace_init")
        self.M = np.zeros((self.K, 16), np.float32)
        self.visible = np.ones(self.K, np.uint8)
        self.objs = _lib.SplatObjects(self.obj_xyz.data_ptr(), self.obj_ids.data_ptr(), int(self.obj_ids.numel()), self.K,
                                      self.begin.ctypes.data, self.M.ctypes.data, self.visible.ctypes.data)

    def render(self, M0, poses, hidden, next_total):
        L = _lib.lib()
        M0 = np.ascontiguousarray(M0, np.float32).reshape(4, 4)
        for k in range(1, self.K + 1):
            self.M[k - 1] = object_matrix(M0, poses.get(k)).reshape(16)
            self.visible[k - 1] = 0 if k in hidden else 1
        sizes = level_sizes(self.W, self.H, LEVELS)
        idx = [torch.empty((1, h, w), dtype=torch.int32, device="cuda") for (w, h) in sizes]
        dep = [torch.empty((1, h, w), dtype=torch.float32, device="cuda") for (w, h) in sizes]
        if self.cells is not None:                               # the announcement PointCloudRasterizer.render makes
            Mn = np.ascontiguousarray(next_total, np.float32).reshape(16)
            _lib.check(L.read_splat_hint_next_camera(self.ws.data_ptr(), Mn.ctypes.data_as(C.POINTER(C.c_float))),
                       "read_splat_hint_next_camera")
        _lib.check(L.read_splat_forward_objects(
            self.static_xyz.data_ptr(), self.static_ids.data_ptr(), self.cells.data_ptr() if self.cells is not None else None,
            self.n_static, M0.ctypes.data_as(C.POINTER(C.c_float)), self.W, self.H, LEVELS, C.byref(self.objs),
            _lib.ptr_array([t.data_ptr() for t in idx]), _lib.ptr_array([t.data_ptr() for t in dep]), self.ws.data_ptr(),
            self.ws.numel(), _lib.stream_ptr()), "read_splat_forward_objects")
        return idx, dep


@pytest.mark.parametrize("cloud", ["street", "cloud200k"])
def test_partition_listed_once_equals_forward_objects(hip, cloud):
    xyz, labels = _cloud(cloud)
    proj = synthetic.make_proj(W, H)
    old = _ForwardObjects(xyz, labels, W, H)
    new = PointCloudRasterizer(xyz, labels=labels)              # a range list from the constructor on: every label once
    assert new._inst is not None and len(new._inst) == 6
    street = cloud == "street"
    assert (new.cells is not None) == street and (new.n_static >= (1 << 20)) == street
    assert (old.cells is not None) == street and old.n_static == new.n_static and old.K == 6
    views = [synthetic.sweep_pose(10 + 2 * f) for f in range(4)]
    totals = [camera.total_matrix(proj, v)[0] for v in views]
    for f in range(3):
        c = {k: xyz[labels == k].astype(np.float64).mean(0) for k in range(1, 7)}
        poses = {1: translation(camera_space_target(views[f], proj, -0.5 + 0.4 * f, 6.0) - c[1]), 2: about(c[2], rot_z(0.3 * f), (0.1, 0, 0)),
                 3: translation(camera_space_target(views[f], proj, 0.0, 10.0, behind=True) - c[3]), 4: None,
                 5: translation(camera_space_target(views[f], proj, -1.0, 20.0) - c[5]), 6: about(c[6], rot_z(-0.2), (0, 0.05 * f, 0))}
        for k, P in poses.items():
            new.set_object_pose(k, P)
        new.set_object_visible(4, f != 1)
        new.set_object_visible(6, f == 1)
        hidden = ({4} if f == 1 else set()) | (set() if f == 1 else {6})
        a = old.render(totals[f], poses, hidden, totals[f + 1])                       # announced: consecutive frames still match
        b = new.render(totals[f], W, H, LEVELS, next_total=totals[f + 1])
        assert_same(b, a, f"{cloud} frame {f}")
        if f == 0:
            assert bool(torch.isin(b[0][0], torch.from_numpy(np.flatnonzero(labels == 1)).cuda()).any())
    static, pool, _ = im.layout(xyz, labels)
    assert_frame(*b, *im.oracle_frame(static, pool, _instance_list(new), totals[2], W, H), f"{cloud} oracle")


# ---- 2. copies ----------------------------------------------------------------------------------------------------------------------
def test_four_copies_with_the_original_hidden(hip):
    xyz, labels = _cloud("street")
    proj, view = synthetic.make_proj(W, H), synthetic.sweep_pose(14)
    M0 = camera.total_matrix(proj, view)[0]
    r = PointCloudRasterizer(xyz, labels=labels)
    blob = r.cells.data_ptr()
    r.set_object_visible(1, False)
    hs = [r.add_instance(1, P) for P in _four_poses(xyz, labels, 1, view, proj)]
    static, pool, _ = im.layout(xyz, labels)
    got = r.render(M0, W, H, LEVELS)
    assert_frame(*got, *im.oracle_frame(static, pool, _instance_list(r), M0, W, H), "four copies")
    ids1 = torch.from_numpy(np.flatnonzero(labels == 1)).cuda()
    on = torch.isin(got[0][0], ids1)
    assert bool(on[0, :, :8].any()) and bool(on[0, :, 600:].any()), "the copy at the left edge and the one right of the centre are drawn"
    # re-posing and hiding between frames: the next frame, nothing rebuilt
    c = xyz[labels == 1].astype(np.float64).mean(0)
    r.set_instance_pose(hs[0], about(c, rot_z(-0.9), (0.2, 0.0, 0.1)))
    r.set_instance_visible(hs[1], False)
    r.set_object_visible(1, True)
    got = r.render(M0, W, H, LEVELS)
    lst = _instance_list(r)
    assert [v for _, _, _, v in lst] == [True] * 7 + [False] + [True] * 2
    assert_frame(*got, *im.oracle_frame(static, pool, lst, M0, W, H), "re-posed")
    r.remove_instance(hs[3])
    got = r.render(M0, W, H, LEVELS)
    assert_frame(*got, *im.oracle_frame(static, pool, _instance_list(r), M0, W, H), "one removed")
    assert r.cells.data_ptr() == blob


# ---- 3. the 32-range flush ----------------------------------------------------------------------------------------------------------
def test_seventy_instances_cross_the_batch_boundary_twice(hip):
    w, h = 256, 128
    xyz = synthetic.make_cloud(50_000, 8)
    labels = cluster_labels(xyz, 1, 300, 5)
    labels[np.flatnonzero(labels == 0)[:40]] = 3                               # label 2 has no points: an empty range
    M0 = camera.total_matrix(synthetic.make_proj(w, h, f=120.0), synthetic.sweep_pose(2))[0]
    r = PointCloudRasterizer(xyz, labels=labels)
    rng = np.random.default_rng(7)
    hs = [r.add_instance(1, translation(rng.uniform(-1.5, 1.5, 3))) for _ in range(66)]   # + the 3 own ones = 69
    hs.append(r.add_instance(2, translation((0.1, 0.0, 0.0))))                # the empty range, instance 70
    lst = _instance_list(r)
    assert len(lst) == 70 and lst[1][1] == 0 and lst[69][1] == 0
    for i in (31, 32, 33, 64):                                                 # list positions; handle = position here
        r.set_instance_visible(i, False)
    lst = _instance_list(r)
    assert [i for i, x in enumerate(lst) if not x[3]] == [31, 32, 33, 64]
    static, pool, _ = im.layout(xyz, labels)
    got = r.render(M0, w, h, LEVELS)
    ref = im.oracle_frame(static, pool, lst, M0, w, h)
    assert_frame(*got, *ref, "70 instances")
    assert_frame(*got, *im.frame(static, pool, lst, M0, w, h), "70 instances, model")
    assert np.isin(ref[0][0], np.flatnonzero(labels == 1)).sum() > 300


# ---- 4. a foreign object --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _foreign_case():
    """The frames of case 4, shared with the gather test: a 200 000-point labelled cloud, 3 000 points cut from a second cloud with
    extract_object (its first 32 moved onto scene points that win pixels: exact ties), instanced twice."""
    xyz, labels = _cloud("cloud200k")
    N = xyz.shape[0]
    proj, view = synthetic.make_proj(W, H), synthetic.sweep_pose(12)
    M0 = camera.total_matrix(proj, view)[0]
    other = Scene(synthetic.make_cloud(60_000, 17))
    other.set_object_labels(cluster_labels(other.xyz, 2, 3_000, 3))
    cut, cut_ids = other.extract_object(2)
    assert cut.shape == (3_000, 3) and np.array_equal(cut, other.xyz[cut_ids])
    front = np.unique(oracle.raster_multiscale(xyz, M0, W, H, 1, threads=16)[0][0])
    twins = np.random.default_rng(1).choice(front[front > 0], 32, replace=False)
    cut[:32] = xyz[twins]
    r = PointCloudRasterizer(xyz, labels=labels)
    k = r.add_object(cut)
    assert k == 7 and r.id_ranges() == [(0, N), (N, 3_000)]
    c = cut[32:].astype(np.float64).mean(0)
    r.add_instance(k, None)                                                    # where it is: the 32 twins tie with scene points
    r.add_instance(k, translation(camera_space_target(view, proj, -0.2, 5.0) - c))
    frame = copy(r.render(M0, W, H, LEVELS))
    return dict(xyz=xyz, labels=labels, N=N, M0=M0, cut=cut, twins=twins, r=r, frame=frame, proj=proj, view=view)


def test_foreign_object_instanced_twice(hip):
    s = _foreign_case()
    N, r, (idx, dep) = s['N'], s['r'], s['frame']
    static, pool, _ = im.layout(s['xyz'], s['labels'], foreign=[s['cut']])
    assert_frame(idx, dep, *im.oracle_frame(static, pool, _instance_list(r), s['M0'], W, H), "static + own + foreign")
    won = idx[0][idx[0] >= N]
    assert won.numel() > 500 and int(won.max()) < N + 3_000, "the foreign object wins pixels with ids in [N, N + 3000)"
    pix, _ = oracle.project_points(s['xyz'][s['twins']], s['M0'], W, H)
    assert (pix >= 0).all()
    assert np.array_equal(idx[0].reshape(-1).cpu().numpy()[pix], s['twins']), "a scene point wins an exact tie: its id is smaller"
    # a cloud without labels takes the same object as if every label were 0, and keeps its one copy of xyz
    plain = PointCloudRasterizer(s['xyz'])
    k = plain.add_object(s['cut'])
    assert k == 1 and plain._static_xyz is plain.xyz
    for _, P, v in r._instance_list()[6:]:
        plain.add_instance(k, P, v)
    s0, p0, _ = im.layout(s['xyz'], None, foreign=[s['cut']])
    assert_frame(*plain.render(s['M0'], W, H, LEVELS), *im.oracle_frame(s0, p0, _instance_list(plain), s['M0'], W, H), "unlabelled")
    with pytest.raises(ValueError, match="int32"):
        big = PointCloudRasterizer.__new__(PointCloudRasterizer)
        big.n, big._foreign, big._inst, big.labels, big.device = (1 << 31) - 100, [], None, None, r.device
        big.add_object(s['cut'])


# ---- 5. the gather over several tables ----------------------------------------------------------------------------------------------
def test_table_gather_on_the_foreign_frames(hip):
    s = _foreign_case()
    N, idx = s['N'], s['frame'][0]
    rows = torch.from_numpy(np.ascontiguousarray(synthetic.make_descriptors(N).T)).cuda()
    rows_f = torch.from_numpy(np.ascontiguousarray(synthetic.make_descriptors(3_000, seed=5).T)).cuda()
    both = torch.cat([rows, rows_f]).contiguous()
    assert int((idx[0] >= N).sum()) > 500
    for a, b in zip(gather_tables_pyramid([(both, 0, 'none')], idx), gather_pyramid(both, idx)):                 # T = 1
        assert torch.equal(a, b)
    for act in ('sigmoid', 'tanh'):
        for a, b in zip(gather_tables_pyramid([(both, 0, act)], idx), gather_pyramid(both, idx, act)):
            assert torch.equal(a, b), act
    plain = gather_pyramid(both, idx)
    two = gather_tables_pyramid([(rows, 0, 'none'), (rows_f, N, 'none')], idx)                                   # T = 2, none / none
    for a, b in zip(two, plain):
        assert torch.equal(a, b)
    for a, b in zip(gather_tables_pyramid([(rows, 0, 'tanh'), (rows_f, N, 'tanh')], idx), gather_pyramid(both, idx, 'tanh')):
        assert torch.equal(a, b)                                                                                  # equal activations
    # an activation per table, against torch on the selected rows (the bound of tests/test_gpu_gather.py)
    got = gather_tables_pyramid([(rows, 0, 'sigmoid'), (rows_f, N, 'tanh')], idx)
    for g, i, p in zip(got, idx, plain):
        want = torch.where((i >= N)[..., None], torch.tanh(p), torch.sigmoid(p))
        torch.testing.assert_close(g, want, rtol=1e-6, atol=1e-6)
    # ids no table serves: below 0 -> row 0 of table 0; beyond the end -> the last row of the last table; T = 8 with a gap
    bad = [i.clone() for i in idx]
    bad[0][0, 5, :7] = -1
    bad[0][0, 6, :7] = N + 3_000 + 5
    bad[4][0, 0, 0] = -1
    bad[4][0, 0, 1] = N + 3_000 + 5
    got = gather_tables_pyramid([(rows, 0, 'none'), (rows_f, N, 'none')], bad)
    for g, i in zip(got, bad):
        ref = im.gather_tables([(rows.cpu().numpy(), 0, 'none'), (rows_f.cpu().numpy(), N, 'none')], i.cpu().numpy())
        assert np.array_equal(g.cpu().numpy(), ref)
    assert torch.equal(got[0][0, 5, 0], rows[0]) and torch.equal(got[0][0, 6, 0], rows_f[-1])
    cuts = [0, 1, 1000, 50_000, 50_001, 120_000, 150_000, 199_999, N]
    tabs = [(rows[a:b].contiguous(), a, 'none') for a, b in zip(cuts[:-1], cuts[1:])]
    tabs = tabs[:3] + tabs[4:]                                                  # id 50 000 falls in a gap: row 49 999
    tabs.append((rows_f[:2_000].contiguous(), N + 500, 'none'))                # ids N .. N + 499 fall in a gap: row N - 1
    assert len(tabs) == 8
    got = gather_tables_pyramid(tabs, bad)
    for g, i in zip(got, bad):
        ref = im.gather_tables([(t.cpu().numpy(), b, a) for t, b, a in tabs], i.cpu().numpy())
        assert np.array_equal(g.cpu().numpy(), ref)


# ---- 6. panorama ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hfov", [200.0, 360.0])
def test_copies_and_a_foreign_object_under_a_panorama_camera(hip, hfov):
    s = _foreign_case()
    xyz, labels, view, proj = s['xyz'], s['labels'], s['view'], s['proj']
    cam = camera.pano_camera(proj, view, hfov)
    r = PointCloudRasterizer(xyz, labels=labels)
    r.set_object_visible(1, False)
    for P in _four_poses(xyz, labels, 1, view, proj):
        r.add_instance(1, P)
    k = r.add_object(s['cut'])
    c = s['cut'][32:].astype(np.float64).mean(0)
    r.add_instance(k, None)
    r.add_instance(k, translation(camera_space_target(view, proj, -0.2, 5.0) - c))
    r.add_instance(k, translation(camera_space_target(view, proj, 0.0, 6.0, behind=True) - c), visible=hfov == 360.0)
    got = r.render_pano(cam, W, H, LEVELS)
    static, pool, _ = im.layout(xyz, labels, foreign=[s['cut']])
    ref = im.frame(static, pool, _instance_list(r), cam, W, H, pano=True)
    assert_frame(*got, *ref, f"hfov {hfov}")
    assert (ref[0][0] >= s['N']).sum() > 200 and np.isin(ref[0][0], np.flatnonzero(labels == 1)).sum() > 200
    pinhole = r.render(s['M0'], W, H, LEVELS)                                  # pinhole and panorama frames alternate
    assert_frame(*pinhole, *im.oracle_frame(static, pool, _instance_list(r), s['M0'], W, H), "pinhole after panorama")


# ---- 7. end to end --------------------------------------------------------------------------------------------------------------------
def test_ogl_fast_path_with_a_foreign_object(hip):
    from tests.test_gpu_api import _model
    w, h, N, m = 256, 64, 25_000, 1_500
    xyz = synthetic.make_cloud(N)
    labels = cluster_labels(xyz, 3, 1_500, 15)
    model, state, tex = _model(N)
    other = Scene(synthetic.make_cloud(20_000, 17))
    other.set_object_labels(cluster_labels(other.xyz, 1, m, 3))
    cut, _ = other.extract_object(1)
    ftex = PointTexture(8, m, init_method='rand').cuda()
    scene = Scene(xyz)
    proj, pose = synthetic.make_proj(w, h, f=80.0), synthetic.sweep_pose(4)
    scene.set_proj_matrix(proj)
    scene.set_camera_view(pose)
    scene.set_object_labels(labels)
    k = scene.add_foreign_object(cut, ftex)
    assert k == 4
    c = cut.astype(np.float64).mean(0)
    P = translation(camera_space_target(pose, proj, 0.1, 4.0) - c)
    P_own = about(xyz[labels == 2].astype(np.float64).mean(0), rot_z(0.5), (0.3, 0.0, 0.0))
    scene.add_object_instance(k, P)
    h_own = scene.add_object_instance(2, P_own)
    ogl = OGL.from_model(scene, model, FMT, (w, h))
    out = ogl.infer()['output']
    assert ogl.last_path == 'fast'
    M = camera.total_matrix(proj, pose)[0]
    static, pool, ranges = im.layout(xyz, labels, foreign=[cut])
    lst = [(f, n, None, True) for f, n in ranges[:3]] + [(ranges[3][0], m, P, True), (ranges[1][0], ranges[1][1], P_own, True)]
    oi, od = im.oracle_frame(static, pool, lst, M, w, h)
    assert (oi[0] >= N).sum() > 100
    table = torch.cat([tex.texture_.detach().reshape(-1, N), ftex.texture_.detach().reshape(-1, m)], 1)
    with torch.no_grad():
        want = unet_torch.net_and_texture_forward(state, table.cpu().numpy()[None], oi)[0]
    assert unet_torch.psnr(out[..., :3].permute(2, 0, 1).cpu(), want) >= 120.0
    fr = FrameRenderer(xyz, tex.texture_.detach().reshape(-1, N), model.net.packed_weights(), w, h, proj_matrix=proj,
                       object_labels=labels)                                   # the blob the model packed: no second packing
    kf = fr.add_object(cut, ftex.texture_.detach().reshape(-1, m))
    fr.add_instance(kf, P)
    fr.add_instance(2, P_own)
    ref = fr.render(pose)
    torch.cuda.synchronize()
    assert_frame(fr.idx, fr.depth, oi, od, "FrameRenderer")
    torch.testing.assert_close(out, ref, rtol=0, atol=1e-6)
    # a table that does not fit the rasteriser's range is refused by size
    scene.foreign_objects[0] = (cut, PointTexture(8, m + 1, init_method='rand').cuda())
    with pytest.raises(ValueError, match="foreign object 1"):
        ogl.infer()
    scene.foreign_objects[0] = (cut, ftex)
    # the edit reaches the next frame without a rebuild
    raster = scene.rasterizer()
    scene.remove_instance(h_own)
    assert scene.rasterizer() is raster
    ogl.infer()
    idx, _ = raster.render(M, w, h, LEVELS, want_depth=False)
    assert torch.equal(idx[0][0].cpu(), torch.from_numpy(im.oracle_frame(static, pool, lst[:4], M, w, h)[0][0]))


def test_frames_in_flight_show_the_pose_they_were_enqueued_with(hip):
    w = h = 256
    N, m = 40_000, 1_000
    xyz, desc = synthetic.make_cloud(N, 3), synthetic.make_descriptors(N)
    labels = cluster_labels(xyz, 2, 2_000, 14)
    packed = torch.from_numpy(pack_state(synthetic.make_unet_state(weight_spec()), layout=default_layout())).cuda()   # packed once
    proj = synthetic.make_proj(w, h, f=160.0)
    cut = synthetic.make_cloud(30_000, 21)[:m] * 0.1 + xyz[labels == 1].mean(0)
    fdesc = synthetic.make_descriptors(m, seed=9)
    frs = [FrameRenderer(xyz, desc, packed, w, h, proj_matrix=proj, object_labels=labels, frames_in_flight=f) for f in (1, 2)]
    hs = []
    for fr in frs:
        k = fr.add_object(cut, fdesc)
        hs.append((fr.add_instance(k, None), fr.add_instance(1, translation((0.4, 0.0, 0.0)))))
    outs = [[], []]
    pose = synthetic.sweep_pose(3)
    for f in range(4):
        for j, fr in enumerate(frs):
            fr.set_instance_pose(hs[j][0], translation((0.15 * f, -0.1 * f, 0.0)))
            fr.set_instance_visible(hs[j][1], f != 2)
            o = fr.render(pose)                                                # same camera: only the instances move
            outs[j].append(o.clone() if j == 0 else o)
    frs[1].sync()
    torch.cuda.synchronize()
    for f in range(4):
        assert torch.equal(outs[0][f], outs[1][f]), f"frame {f}"
    assert not torch.equal(outs[0][0], outs[0][1]) and not torch.equal(outs[0][1], outs[0][2])


# ---- 8. inside a stitched part ------------------------------------------------------------------------------------------------------
def test_own_instances_inside_a_stitched_part(hip):
    w, h = 64, 48
    a = synthetic.make_cloud(20_000, 1)
    b = synthetic.make_cloud(15_000, 2)
    labels_b = cluster_labels(b, 2, 600, 4)
    M0 = sm.union_camera(w, h)
    st = StitchedRasterizer([a, b], cells=False, labels=[None, labels_b])
    P1 = translation((0.5, 0.0, 0.0))
    st.set_part_pose(1, P1)
    st.part(1).add_instance(1, translation((0.0, 0.0, 70.0)))                 # in front of the clouds' near face
    st.part(1).add_instance(2, about(b[labels_b == 2].astype(np.float64).mean(0), rot_z(0.7), (30.0, 0.0, 110.0)))
    st.part(1).set_object_visible(2, False)
    idx, dep = st.render_merged(M0, w, h, LEVELS)
    Ms = st.part_matrices(M0)
    static, pool, _ = im.layout(b, labels_b)
    part1 = im.oracle_frame(static, pool, _instance_list(st.part(1)), Ms[1], w, h)
    part0 = oracle.raster_multiscale(a, Ms[0], w, h, LEVELS, threads=16)
    mi, md, _, _ = sm.merge([(part0[0], part0[1], 0), (part1[0], part1[1], 20_000)])
    assert_frame(idx, dep, mi, md, "stitched")
    assert np.isin(mi[0], 20_000 + np.flatnonzero(labels_b == 1)).any() and np.isin(mi[0], 20_000 + np.flatnonzero(labels_b == 2)).any()
