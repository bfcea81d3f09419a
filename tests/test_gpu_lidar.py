"""GPU: LiDAR sweeps against their NumPy definition, tests/lidar_model.py.  Every comparison is exact: cell and
range bits per point, range / index images, count, and the return list's cells, ids and xyz bit patterns."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from read_amd import _lib, lidar
from read_amd.ogl import OGL
from read_amd.raster import PointCloudRasterizer
from read_amd.render import Scene
from tests import lidar_cases as lc
from tests import lidar_model as lm
from tests import pano_cases as pc

pytestmark = pytest.mark.gpu

f32 = np.float32
FMT = "uv_1d_p1, uv_1d_p1_ds1, uv_1d_p1_ds2, uv_1d_p1_ds3, uv_1d_p1_ds4"
GUARD = 64                                                       # entries behind every list buffer that must stay untouched


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- the projection entry --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _operands():
    """2e5 random points all round the sensor, log-uniform in range from 5 cm to 500 m, and the edge catalogue (the axis, c1 = 0,
    the ends of the range gate, the seam, NaN / Inf, scales 10^5 apart) of the upright sensor."""
    rng = np.random.default_rng(21)
    n = 200_000
    r = np.exp(rng.uniform(np.log(0.05), np.log(500.0), n))
    th = rng.uniform(-np.pi, np.pi, n)
    el = rng.uniform(-0.6, 0.6, n)
    xyz = np.stack([r * np.cos(el) * np.sin(th), r * np.sin(el), -r * np.cos(el) * np.cos(th)], 1).astype(f32)
    cat = lc.edge_catalogue(lc.sensor_cam(lc.uniform_table(16, -15.0, 15.0), 360.0, 0.5))
    return np.concatenate([xyz, cat])


@pytest.mark.parametrize("B,W,hfov", [(1, 16, 360.0), (16, 64, 360.0), (64, 512, 120.0), (128, 1024, 360.0)])
def test_project_points_equals_the_model(hip, B, W, hfov):
    elev = np.array([-0.05], f32) if B == 1 else lc.nonuniform_table(B, -25.0, 15.0, seed=B)
    xyz = _operands()
    n = xyz.shape[0]
    dev = torch.from_numpy(xyz).cuda()
    cell = torch.empty(n, dtype=torch.int32, device='cuda')
    rng = torch.empty(n, dtype=torch.float32, device='cuda')
    views = (np.eye(4, dtype=f32), lc.pose(yaw=140.0, pitch=9.0, roll=-4.0, t=(0.4, -0.3, 0.8)))
    for v, view in enumerate(views):
        cam = lc.sensor_cam(elev, hfov, 0.02 if B == 1 else 0.5, view=view)
        _lib.check(hip.read_lidar_project_points(dev.data_ptr(), n, cam.ctypes.data, elev.ctypes.data, B, W, cell.data_ptr(),
                                                 rng.data_ptr(), _lib.stream_ptr()), "read_lidar_project_points")
        want_cell, want_rng = lm.project(xyz, cam, elev, W)
        got_cell, got_rng = cell.cpu().numpy(), rng.cpu().numpy()
        ok = want_cell >= 0
        print(f"B {B} W {W} hfov {hfov} view {v}: {int(ok.sum())} of {n} accepted, {int((got_cell != want_cell).sum())} cells differ")
        assert np.array_equal(got_cell, want_cell), f"view {v}: {int((got_cell != want_cell).sum())} cells differ"
        assert np.array_equal(bits(got_rng), bits(want_rng)), f"view {v}: range bits"
        assert ok.sum() > (300 if B == 1 else 5000)
        assert (want_cell[-8:] == -1).all()                                      # NaN / Inf


# ---- sweeps through the C ABI ----------------------------------------------------------------------------------------------------
class Buffers:
    """Device outputs of one read_lidar_sweep call, with guard bands behind the list."""

    def __init__(self, B, W, capacity):
        dev = 'cuda'
        self.B, self.W, self.capacity = B, W, capacity
        self.range = torch.full((B, W), -1.0, dtype=torch.float32, device=dev)
        self.idx = torch.full((B, W), -1, dtype=torch.int32, device=dev)
        self.count = torch.full((1,), -1, dtype=torch.int32, device=dev)
        self.cell = torch.full((capacity + GUARD,), -7, dtype=torch.int32, device=dev)
        self.rid = torch.full((capacity + GUARD,), -7, dtype=torch.int32, device=dev)
        self.xyz = torch.full((capacity + GUARD, 3), -7.0, dtype=torch.float32, device=dev)


def workspace(hip, B, W):
    ws = torch.empty(hip.read_lidar_workspace_bytes(B, W), dtype=torch.uint8, device='cuda')
    _lib.check(hip.read_lidar_workspace_init(ws.data_ptr(), ws.numel(), _lib.stream_ptr()), "read_lidar_workspace_init")
    return ws


def c_sweep(hip, dev_xyz, n, cam, elev, W, tables, window, wrap, scale, slack, out, ws):
    args = _lib.LidarArgs(dev_xyz.data_ptr() if n else None, None, n, None, cam.ctypes.data, elev.ctypes.data, elev.size, W,
                          tables[0].data_ptr(), tables[1].data_ptr(), window[0], window[1], int(wrap), float(scale), float(slack),
                          out.range.data_ptr(), out.idx.data_ptr(), out.count.data_ptr(), out.cell.data_ptr(), out.rid.data_ptr(),
                          out.xyz.data_ptr(), out.capacity, ws.data_ptr(), ws.numel())
    _lib.check(hip.read_lidar_sweep(C.byref(args), _lib.stream_ptr()), "read_lidar_sweep")


def device_tables(elev, W, kx):
    return torch.from_numpy(lm.beam_dir(elev)).cuda(), torch.from_numpy(lm.col_dir(W, kx)).cuda()


def assert_sweep(out, want, what):
    """``out``: Buffers; ``want``: lidar_model.sweep's dict at out.capacity."""
    assert np.array_equal(bits(out.range.cpu().numpy()), bits(want['range'])), f"{what}: range image"
    assert np.array_equal(out.idx.cpu().numpy(), want['idx']), f"{what}: index image"
    assert int(out.count.item()) == want['count'], f"{what}: count {int(out.count.item())} != {want['count']}"
    m = min(want['count'], out.capacity)
    cell, rid, xyz = out.cell.cpu().numpy(), out.rid.cpu().numpy(), out.xyz.cpu().numpy()
    assert np.array_equal(cell[:m], want['cell']) and np.array_equal(rid[:m], want['id']), f"{what}: list cells / ids"
    assert np.array_equal(bits(xyz[:m]), bits(want['xyz'])), f"{what}: list xyz"
    assert (cell[m:] == -7).all() and (rid[m:] == -7).all() and (xyz[m:] == -7.0).all(), f"{what}: written past the list"


@functools.lru_cache(maxsize=None)
def _sweep_case():
    """A 5e4-point cloud under a 24-beam sensor of 200 columns: 4800 cells, 19 tiles of 256 with a part-filled last one."""
    elev = lc.nonuniform_table(24, -22.0, 12.0, seed=2)
    W = 200
    cam = lc.sensor_cam(elev, 360.0, 0.5, view=lc.pose(yaw=33.0, pitch=1.5, roll=-1.0, t=(0.5, 0.1, -0.7)))
    xyz = lc.street_cloud(50_000, 9, dup=1000)
    return elev, W, cam, xyz, lm.key_image(xyz, cam, elev, W)


@pytest.mark.parametrize("wrap", [True, False])
@pytest.mark.parametrize("window", [(0, 0), (1, 2), (4, 4)])
def test_sweep_equals_the_model(hip, window, wrap):
    elev, W, cam, xyz, keys = _sweep_case()
    B = elev.size
    dev = torch.from_numpy(xyz).cuda()
    tables = device_tables(elev, W, cam[12])
    ws = workspace(hip, B, W)
    scale = lm.scale_of(0.05)
    count = lm.sweep(None, cam, elev, W, window, wrap, scale, 0.1, keys=keys.copy())['count']
    assert 100 < count < B * W
    for cap in (count - 37, count, count + 100, 0):               # below, at and above the count; and no list at all
        out = Buffers(B, W, cap)
        c_sweep(hip, dev, xyz.shape[0], cam, elev, W, tables, window, wrap, scale, 0.1, out, ws)
        want = lm.sweep(None, cam, elev, W, window, wrap, scale, 0.1, capacity=cap, keys=keys.copy())
        assert_sweep(out, want, f"window {window} wrap {wrap} capacity {cap}")
    # the sweep left its workspace as init did
    assert bool((ws == 0xFF).all())


def test_empty_sweep_and_absent_outputs(hip):
    elev, W, cam, xyz, keys = _sweep_case()
    B = elev.size
    tables = device_tables(elev, W, cam[12])
    ws = workspace(hip, B, W)
    out = Buffers(B, W, 10)
    c_sweep(hip, None, 0, cam, elev, W, tables, (1, 2), True, 1.05, 0.0, out, ws)          # n = 0, no instances
    assert int(out.count.item()) == 0 and not out.range.any() and not out.idx.any() and (out.cell == -7).all()
    # every output absent but the count; then only the images
    dev = torch.from_numpy(xyz).cuda()
    want = lm.sweep(None, cam, elev, W, (1, 2), True, lm.scale_of(0.05), 0.0, keys=keys.copy())
    cnt = torch.full((1,), -1, dtype=torch.int32, device='cuda')
    args = _lib.LidarArgs(dev.data_ptr(), None, xyz.shape[0], None, cam.ctypes.data, elev.ctypes.data, B, W, None, None, 1, 2, 1,
                          float(lm.scale_of(0.05)), 0.0, None, None, cnt.data_ptr(), None, None, None, 1000, ws.data_ptr(), ws.numel())
    _lib.check(hip.read_lidar_sweep(C.byref(args), _lib.stream_ptr()), "read_lidar_sweep")
    assert int(cnt.item()) == want['count']
    args.range, args.idx, args.count = out.range.data_ptr(), out.idx.data_ptr(), None
    _lib.check(hip.read_lidar_sweep(C.byref(args), _lib.stream_ptr()), "read_lidar_sweep")
    assert np.array_equal(bits(out.range.cpu().numpy()), bits(want['range'])) and np.array_equal(out.idx.cpu().numpy(), want['idx'])
    assert bool((ws == 0xFF).all())


def test_two_sensors_share_a_workspace(hip):
    """A small sensor, then a larger one whose key image reaches over everything the first used, then the small one again: each
    equals the model, so every sweep left the workspace EMPTY."""
    xyz = lc.street_cloud(30_000, 4)
    dev = torch.from_numpy(xyz).cuda()
    small = (lc.uniform_table(8, -12.0, 2.0), 96, 360.0)
    large = (lc.nonuniform_table(40, -24.0, 14.0, seed=5), 333, 200.0)
    ws = workspace(hip, 40, 333)
    assert ws.numel() >= hip.read_lidar_workspace_bytes(8, 96)
    for k, (elev, W, hfov) in enumerate((small, large, small, large)):
        cam = lc.sensor_cam(elev, hfov, 0.5, view=lc.pose(yaw=20.0 * k, t=(0.2 * k, 0.0, 0.1)))
        out = Buffers(elev.size, W, elev.size * W)
        c_sweep(hip, dev, xyz.shape[0], cam, elev, W, device_tables(elev, W, cam[12]), (1, 2), hfov == 360.0, lm.scale_of(0.05), 0.2, out, ws)
        want = lm.sweep(xyz, cam, elev, W, (1, 2), hfov == 360.0, lm.scale_of(0.05), 0.2)
        assert want['count'] > 50
        assert_sweep(out, want, f"sweep {k}")


# ---- the rasteriser: labels, poses, visibility, instances ------------------------------------------------------------------------
def test_labelled_cloud_moved_hidden_and_drawn_twice(hip):
    n = 30_000
    xyz = lc.street_cloud(n, 13, dup=300)
    labels = lc.labels_for(n, 4, n_objects=3, share=0.1)
    r = PointCloudRasterizer(xyz, labels=labels)
    sensor = lidar.LidarSensor(np.linspace(-20.0, 10.0, 20), 160, window=(1, 2), rel=0.05, slack=0.2)
    assert sensor.wrap and np.array_equal(sensor.elev, lc.uniform_table(20, -20.0, 10.0))
    assert sensor.half_width == pytest.approx(0.5 * lc.spacing(sensor.elev))
    view = lc.pose(yaw=20.0, pitch=-2.0, roll=1.0, t=(0.3, 0.2, 0.1))
    cam = sensor.camera(view)
    P1 = (lc.translation((3.0, 0.5, -2.0)) @ lc.rot(1, 40.0)).astype(f32)
    P3 = lc.translation((0.0, 0.0, 6.0))
    r.set_object_pose(1, P1)
    r.set_object_visible(2, False)
    r.add_instance(3, P3)
    sw = r.sweep_lidar(sensor, cam)
    keys = lm.labelled_keys(xyz, labels, cam, sensor.elev, sensor.W, {1: P1}, {2}, extra=[(3, P3)])
    assert not np.array_equal(keys, lm.labelled_keys(xyz, labels, cam, sensor.elev, sensor.W, {}, set()))      # the edits show
    want = lm.sweep(None, cam, sensor.elev, sensor.W, (1, 2), True, sensor.scale, sensor.slack, keys=keys)
    assert np.array_equal(bits(sw.range.cpu().numpy()), bits(want['range'])) and np.array_equal(sw.ids.cpu().numpy(), want['idx'])
    count = sw.count
    assert count == want['count'] > 300 and sw.capacity == sensor.B * sensor.W
    assert np.array_equal(sw.cells[:count].cpu().numpy(), want['cell']) and np.array_equal(sw.return_ids[:count].cpu().numpy(), want['id'])
    assert sw.points.shape == (count, 3) and np.array_equal(bits(sw.points.cpu().numpy()), bits(want['xyz']))
    got_labels = sw.labels
    assert got_labels.shape == (sw.capacity,) and np.array_equal(got_labels[:count].cpu().numpy(), labels[want['id']])
    assert not (got_labels[:count] == 2).any() and (got_labels[:count] == 1).any()
    # a foreign object is numbered after the labels; a second sweep into the same result
    k = r.add_object(xyz[:500] + np.array([0.0, 3.0, 0.0], f32))
    r.add_instance(k)
    sw2 = r.sweep_lidar(sensor, cam, out=sw)
    assert sw2 is sw
    ids = sw.return_ids[:sw.count].cpu().numpy()
    lab = sw.labels[:sw.count].cpu().numpy()
    assert (ids >= n).any() and (lab[ids >= n] == 4).all() and np.array_equal(lab[ids < n], labels[ids[ids < n]])
    # a cloud without labels has none; a camera of another field is refused by name
    plain = PointCloudRasterizer(xyz).sweep_lidar(sensor, cam)
    assert plain.labels is None
    want = lm.sweep(xyz, cam, sensor.elev, sensor.W, (1, 2), True, sensor.scale, sensor.slack)
    assert plain.count == want['count'] and np.array_equal(bits(plain.points.cpu().numpy()), bits(want['xyz']))
    with pytest.raises(ValueError, match="sensor"):
        r.sweep_lidar(sensor, lc.sensor_cam(sensor.elev, 120.0, 0.5))


def test_thirty_three_instances_cross_the_flush(hip):
    """33 copies of object 1 beside the object itself: 34 ranges, two launches of lidar_pass_kernel (32 ranges each at most), one
    copy hidden: range image, ids and return list against the model's sweep over the same ranges."""
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
    sensor = lidar.LidarSensor(np.linspace(-20.0, 10.0, 16), 256, window=(1, 2), rel=0.05, slack=0.2)
    cam = sensor.camera(lc.pose(yaw=20.0, pitch=-2.0, roll=1.0, t=(0.3, 0.2, 0.1)))
    assert r.lidar_instance_cameras(cam).shape == (34, 16)
    shown = [(1, P) for i, P in enumerate(poses) if i != 31]
    keys = lm.labelled_keys(xyz, labels, cam, sensor.elev, sensor.W, {}, set(), extra=shown)
    assert (keys != lm.labelled_keys(xyz, labels, cam, sensor.elev, sensor.W, {}, set())).sum() > 30      # the copies show
    last = lm.key_image(xyz[sel], lm.object_camera(cam, poses[32]), sensor.elev, sensor.W, ids=sel)
    assert ((last != lm.EMPTY_KEY) & (last == keys)).any()           # and so does the one past the 32-range flush
    want = lm.sweep(None, cam, sensor.elev, sensor.W, (1, 2), True, sensor.scale, sensor.slack, keys=keys)
    sw = r.sweep_lidar(sensor, cam)
    assert np.array_equal(bits(sw.range.cpu().numpy()), bits(want['range'])) and np.array_equal(sw.ids.cpu().numpy(), want['idx'])
    count = sw.count
    assert count == want['count'] > 100
    assert np.array_equal(sw.cells[:count].cpu().numpy(), want['cell']) and np.array_equal(sw.return_ids[:count].cpu().numpy(), want['id'])
    assert sw.points.shape == (count, 3) and np.array_equal(bits(sw.points.cpu().numpy()), bits(want['xyz']))


# ---- Scene.lidar_sweep, and frames around it ---------------------------------------------------------------------------------------
def test_scene_lidar_sweep_leaves_frames_alone(hip):
    from tests.test_gpu_api import _model
    W, H, N = 192, 48, 20_000
    xyz = lc.street_cloud(N, 15)
    model, state, tex = _model(N)
    view = lc.pose(yaw=30.0, pitch=4.0, roll=-3.0, t=(0.25, 0.125, -0.5))
    scene = Scene(xyz)
    from tests import pano_cases as pc
    scene.set_proj_matrix(pc.proj(W, H))
    scene.set_camera_view(view)
    ogl = OGL.from_model(scene, model, FMT, (W, H))
    before = ogl.infer()['output'].clone()
    sensor = lidar.LidarSensor(np.linspace(-15.0, 15.0, 16), 128, hfov_deg=180.0, half_width_deg=0.9, slack=0.2)
    assert not sensor.wrap
    sw = scene.lidar_sweep(sensor)
    cam = sensor.camera(view)
    want = lm.sweep(xyz, cam, sensor.elev, sensor.W, (1, 2), False, sensor.scale, sensor.slack)
    assert sw.count == want['count'] > 100
    assert np.array_equal(bits(sw.range.cpu().numpy()), bits(want['range'])) and np.array_equal(sw.ids.cpu().numpy(), want['idx'])
    assert np.array_equal(bits(sw.points.cpu().numpy()), bits(want['xyz']))
    assert torch.equal(ogl.infer()['output'], before) and ogl.last_path == 'fast'
    # the model matrix takes part as in pano_camera; set_panorama plays none; another pose is another sweep
    T = lc.translation((1.0, -2.0, 0.5))
    scene.set_model_view(T)
    scene.set_panorama(90.0)
    moved = scene.lidar_sweep(sensor, (T.astype(np.float64) @ view.astype(np.float64)).astype(f32))
    assert moved.count == sw.count and torch.equal(moved.range, sw.range) and torch.equal(moved.ids, sw.ids)
    scene.set_panorama(None)
    scene.set_model_view(np.eye(4, dtype=f32))
    other = scene.lidar_sweep(sensor, lc.pose(yaw=-60.0))
    assert not torch.equal(other.ids, sw.ids)
    assert torch.equal(ogl.infer()['output'], before)
