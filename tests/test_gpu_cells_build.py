"""GPU: the device-side build of the cell-ordered cloud (read_splat_cells_build, raster.build_cells_device).

The blob must be the host builder's (read_splat_cells_build_host) on every byte the host defines — header, records, ids,
chunk boxes, the zeroed regions — except that a min / max field may hold the other signed zero (the host keeps whichever zero
it met first, the device reduction meets them in another order): those fields are compared by value.  Frames rendered over a
device blob are bit-exact against the oracle, also after the blob was rebuilt in place under a prepared next frame."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle
from read_amd import _lib, camera, pcpr, synthetic
from read_amd import raster as raster_mod
from read_amd.raster import PointCloudRasterizer, build_cells, build_cells_device

pytestmark = pytest.mark.gpu


def _layout(n):
    nc = (n + 1023) // 1024
    rec = 256
    aabb = rec + nc * 1024 * 16
    lists = aabb + nc * 32
    return nc, rec, aabb, lists


def _assert_same_blob(dev, host, n, what=""):
    dev = dev.cpu().numpy() if torch.is_tensor(dev) else dev
    assert dev.dtype == np.uint8 and dev.shape == host.shape, what
    nc, rec, aabb, lists = _layout(n)
    sticky = len(host) - ((nc + 255) // 256) * 256
    assert np.array_equal(dev[:16], host[:16]), f"{what}: header n / nchunks / version"
    assert np.array_equal(dev[16:40].view(np.float32), host[16:40].view(np.float32)), f"{what}: header bbox"
    assert np.array_equal(dev[40:44], host[40:44]), f"{what}: density"
    assert not host[44:256].any() and np.array_equal(dev[44:256], host[44:256]), f"{what}: header padding"
    d, h = dev[rec:aabb], host[rec:aabb]
    if not np.array_equal(d, h):
        bad = np.flatnonzero((d.view(np.uint32) != h.view(np.uint32)).reshape(-1, 4).any(1))
        raise AssertionError(f"{what}: {bad.size} records differ, first at {bad[0]}")
    db, hb = dev[aabb:lists].view(np.float32).reshape(nc, 8), host[aabb:lists].view(np.float32).reshape(nc, 8)
    assert np.array_equal(db[:, :6], hb[:, :6]), f"{what}: chunk boxes"
    assert not hb[:, 6:].view(np.uint32).any() and not db[:, 6:].view(np.uint32).any(), f"{what}: box padding"
    assert not host[sticky:].any() and not dev[sticky:].any(), f"{what}: sticky flags"


def _check_build(xyz, what=""):
    xyz = np.ascontiguousarray(xyz, np.float32)
    dev = build_cells_device(torch.from_numpy(xyz).cuda())
    _assert_same_blob(dev, build_cells(xyz), xyz.shape[0], what)


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 5000, (1 << 20) - 1, (1 << 20) + 3])
def test_device_blob_equals_host_blob_sizes(hip, n):
    _check_build(synthetic.make_cloud(n, 17 + n % 97), f"make_cloud({n})")


def test_device_blob_equals_host_blob_large(hip):
    _check_build(synthetic.make_cloud(3_000_000, 4), "make_cloud(3M)")
    _check_build(synthetic.make_street_cloud(3_000_000, 4), "make_street_cloud(3M)")
    _check_build(synthetic.make_cloud(30_000_000), "make_cloud(30M)")


def test_device_blob_equals_host_blob_degenerate_clouds(hip):
    rng = np.random.default_rng(5)
    base = synthetic.make_cloud(200_000, 9)
    _check_build(np.full((5000, 3), 2.5, np.float32), "all points identical (ext = 0)")
    _check_build(np.zeros((70_000, 3), np.float32), "all points at the origin")
    plane = base.copy()
    plane[:, 1] = 3.0
    _check_build(plane, "a plane")
    _check_build(base[rng.integers(0, 50, 300_000)], "50 distinct points, 300 K copies (equal Morton codes)")
    coarse = np.round(base / 7.0).astype(np.float32) * 7.0
    _check_build(coarse, "coarse lattice (many equal codes)")
    _check_build(base + np.float32(5000.0), "5 km world offset")
    _check_build(base - np.float32(200.0), "negative coordinates")
    z = base[:66_000].copy()
    signs = rng.integers(0, 4, z.shape)
    z[signs == 0] = 0.0
    z[signs == 1] = -0.0
    z[signs == 2] = rng.choice(np.array([1e-45, -1e-45, 1e-40, -3e-39, 1.1754942e-38], np.float32), int((signs == 2).sum()))
    _check_build(z, "+-0.0 and subnormals")
    sub = rng.choice(np.array([0.0, -0.0, 1e-45, 2e-45, 7e-42, -5e-44], np.float32), (9000, 3))
    _check_build(sub, "subnormal-sized cloud")
    # (x - lo) * scale exactly on an integer / on 1023.0: scale = 1 and 0.5 exactly (ext = 1023.999 and its double), and
    # non-power-of-two extents with points on the cell borders
    for ext in (np.float32(1023.999), np.float32(2047.998), np.float32(3.0), np.float32(100.0), np.float32(1e-3)):
        scale = np.float32(1023.999) / ext
        q = rng.integers(0, 1024, (40_000, 3)).astype(np.float64)
        pts = (q / np.float64(scale)).astype(np.float32)
        pts[0] = 0.0
        pts[1] = ext
        pts[2] = np.float32(1023.0) / scale
        _check_build(pts, f"cell borders, ext {ext}")
        _check_build(pts - np.float32(17.25), f"cell borders, ext {ext}, shifted")


@pytest.mark.parametrize("bad_at", [[0], [7, 123_456], [1_048_578], [900_000, 2, 700_000]])
def test_non_finite_points_report_the_smallest_index(hip, bad_at):
    n = (1 << 20) + 3
    xyz = synthetic.make_cloud(n, 3)
    for j, i in enumerate(bad_at):
        xyz[i, j % 3] = (np.nan, np.inf, -np.inf)[j % 3]
    first = min(bad_at)
    with pytest.raises(_lib.ReadHipError) as host_err:
        build_cells(xyz)
    # the blob is left as it was
    t = torch.from_numpy(xyz).cuda()
    L = _lib.lib()
    nbytes, sbytes = L.read_splat_cells_bytes(n), L.read_splat_cells_build_scratch_bytes(n)
    blob = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device="cuda")
    scratch = torch.empty(sbytes, dtype=torch.uint8, device="cuda")
    rc = L.read_splat_cells_build(t.data_ptr(), n, blob.data_ptr(), nbytes, scratch.data_ptr(), sbytes, _lib.stream_ptr())
    msg = L.read_last_error().decode()
    assert rc == -22 and msg == f"read_splat_cells_build: point {first} is not finite", msg
    assert str(host_err.value).endswith(f"read_splat_cells_build_host: point {first} is not finite"), str(host_err.value)
    assert bool((blob == 0xA5).all())
    with pytest.raises(_lib.ReadHipError, match=f"point {first} is not finite"):
        build_cells_device(t)
    with pytest.raises(_lib.ReadHipError, match=f"point {first} is not finite"):
        PointCloudRasterizer(t)


def _no_host_build(*a, **k):
    raise AssertionError("the host builder was called")


def _frame_exact(r, xyz, M, W, H, Mn=None, what=""):
    idx, dep = r.render(M, W, H, 5, next_total=Mn)
    oi, od = oracle.raster_multiscale(xyz, np.asarray(M, np.float32).reshape(4, 4), W, H, 5, threads=8)
    for l in range(5):
        assert np.array_equal(idx[l][0].cpu().numpy(), oi[l]), f"{what} level {l}"
        assert np.array_equal(dep[l][0].cpu().numpy().view(np.uint32), od[l].view(np.uint32)), f"{what} level {l} depth"


def test_frames_over_a_device_blob_are_exact(hip, monkeypatch):
    monkeypatch.setattr(raster_mod, "build_cells", _no_host_build)
    W, H = 304, 176
    xyz = synthetic.make_cloud(1_500_000, 21)
    proj = synthetic.make_proj(W, H, f=180.0)
    r = PointCloudRasterizer(torch.from_numpy(xyz).cuda())
    assert r.cells is not None
    _assert_same_blob(r.cells, build_cells(xyz), xyz.shape[0], "rasteriser blob")     # this module's own reference to it
    for k in (0, 40, 200):
        _frame_exact(r, xyz, camera.total_matrix(proj, synthetic.sweep_pose(k))[0], W, H, what=f"pose {k}")


def test_rebuild_in_place_under_a_prepared_frame(hip):
    """Warm frames with the next camera announced, then the SAME blob address rebuilt from another cloud of the same size
    through read_splat_cells_build: the announced frame must not consume the preparation made against the old contents."""
    W, H = 304, 176
    n = 1_500_000
    xyz1 = synthetic.make_cloud(n, 31)
    xyz2 = synthetic.make_cloud(n, 32) * np.float32(0.8) + np.float32([5.0, 1.0, -10.0])
    proj = synthetic.make_proj(W, H, f=180.0)
    Ms = [camera.total_matrix(proj, synthetic.sweep_pose(k))[0] for k in (3, 4, 5, 6)]
    r = PointCloudRasterizer(torch.from_numpy(xyz1).cuda())
    addr = r.cells.data_ptr()
    for i in range(3):
        _frame_exact(r, xyz1, Ms[i], W, H, Mn=Ms[i + 1], what=f"warm frame {i}")      # frame 2 prepares Ms[3]
    t2 = torch.from_numpy(xyz2).cuda()
    L = _lib.lib()
    sbytes = L.read_splat_cells_build_scratch_bytes(n)
    scratch = torch.empty(sbytes, dtype=torch.uint8, device="cuda")
    _lib.check(L.read_splat_cells_build(t2.data_ptr(), n, C.c_void_p(addr), r.cells.numel(), scratch.data_ptr(), sbytes,
                                        _lib.stream_ptr()), "read_splat_cells_build")
    r.xyz = t2
    assert r.cells.data_ptr() == addr
    _assert_same_blob(r.cells, build_cells(xyz2), n, "rebuilt blob")
    _frame_exact(r, xyz2, Ms[3], W, H, what="announced frame after the rebuild")
    _frame_exact(r, xyz2, Ms[0], W, H, what="next frame after the rebuild")


def test_pcpr_forward_builds_on_the_device(hip, monkeypatch):
    monkeypatch.setattr(raster_mod, "build_cells", _no_host_build)
    pcpr.clear_cache()
    W, H = 256, 128
    pts = torch.from_numpy(synthetic.make_cloud((1 << 20) + 17, 41)).cuda()
    tm = torch.from_numpy(camera.total_matrix(synthetic.make_proj(W, H, f=150.0), synthetic.sweep_pose(12)))

    def exact(what):
        index, depth = pcpr.forward(pts, tm, W, H, 512)
        oi, od = oracle.raster_level(pts.cpu().numpy(), tm[0].numpy(), W, H)
        assert np.array_equal(index[0].numpy(), oracle.index_to_float(oi)), what
        assert np.array_equal(depth[0].numpy().view(np.uint32), od.view(np.uint32)), what

    try:
        exact("first call")
        r = pcpr._rasterizer_for(pts)
        assert r.cells is not None
        pts.mul_(0.9).add_(torch.tensor([2.0, 0.5, -3.0], device="cuda"))        # in place: a cache miss, a new blob
        exact("after an in-place change")
        assert pcpr._rasterizer_for(pts) is not r
    finally:
        pcpr.clear_cache()
