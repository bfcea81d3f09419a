"""CPU: scene editing's third verb, add — the C ABI (read_splat_forward_instances, read_splat_forward_pano_instances,
read_gather_forward_tables: exported, bound, refusing bad arguments before any device work), the NumPy model of the contract against
the per-instance oracle, the table-gather model, and the Scene state that is replayed into a rebuilt rasteriser.  Frames are
checked on the GPU (tests/test_gpu_instances.py)."""
import ctypes as C
import functools
import os
import types

import numpy as np
import pytest

from read_amd import _lib, camera, synthetic
from read_amd import render as render_mod
from read_amd.ogl import OGL
from read_amd.render import MultiscaleRender, Scene, StitchedScene
from tests import instances_model as im
from tests import pano_cases as pc

FAKE = 1 << 20          # a 256-byte aligned non-null address: the calls below fail on their arguments and never touch it
NEW = ("read_splat_forward_instances", "read_splat_forward_pano_instances", "read_gather_forward_tables")
FMT = "uv_1d_p1, uv_1d_p1_ds1, uv_1d_p1_ds2, uv_1d_p1_ds3"


# ---- C ABI ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_bound_and_declared():
    L = C.CDLL(_lib.LIB_PATH)
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "read_hip.h")).read()
    for name in NEW:
        assert hasattr(L, name) and name in _lib.SIGNATURES and f"int {name}(" in hdr, name
    assert _lib.lib().read_abi_version() == 3


def test_struct_layouts():
    # const float *, const int32_t *, int64_t, int (+4 pad), const int64_t * x 2, const float *, const unsigned char *
    assert C.sizeof(_lib.SplatInstances) == 64
    assert [getattr(_lib.SplatInstances, f).offset for f in ("xyz", "ids", "n", "count", "first", "npts", "M", "visible")] == \
        [0, 8, 16, 24, 32, 40, 48, 56]
    # const float *, int64_t, int64_t, int (+4 pad)
    assert C.sizeof(_lib.GatherTable) == 32
    assert [getattr(_lib.GatherTable, f).offset for f in ("rows_nc", "n", "id_base", "activation")] == [0, 8, 16, 24]


def _cam(hfov=360.0):
    return camera.pano_camera(pc.proj(64, 48), np.eye(4), hfov)


class _Inst:
    """A read_splat_instances whose host arrays stay alive."""

    def __init__(self, first=(0, 10, 0), npts=(10, 20, 30), n=30, xyz=FAKE, ids=FAKE, M=True, visible=None, count=None, pano=False):
        self.first = None if first is None else np.asarray(first, np.int64)
        self.npts = None if npts is None else np.asarray(npts, np.int64)
        cnt = len(first) if count is None else count
        self.M = (np.tile(_cam(), (max(cnt, 1), 1)) if pano else np.zeros((max(cnt, 1), 16), np.float32)) if M else None
        self.visible = None if visible is None else np.asarray(visible, np.uint8)
        p = lambda a: None if a is None else a.ctypes.data
        self.s = _lib.SplatInstances(xyz, ids, n, cnt, p(self.first), p(self.npts), p(self.M), p(self.visible))


def _call(inst, pano=False, W=64, H=48, levels=5, xyz=FAKE, ids=FAKE, n_static=100, M=True, ws=FAKE, outs=True, cam=None,
          ws_bytes=1 << 40):
    L = _lib.lib()
    Mh = (np.eye(4, dtype=np.float32).reshape(16) if not pano else _cam()) if cam is None else np.ascontiguousarray(cam, np.float32)
    Mp = Mh.ctypes.data_as(C.POINTER(C.c_float)) if M else None
    idx = _lib.ptr_array([FAKE] * min(levels, 5)) if outs else None
    ip = C.byref(inst.s) if inst is not None else None
    if pano:
        rc = L.read_splat_forward_pano_instances(xyz, ids, n_static, Mp, W, H, levels, ip, idx, None, ws, ws_bytes, None)
    else:
        rc = L.read_splat_forward_instances(xyz, ids, None, n_static, Mp, W, H, levels, ip, idx, None, ws, ws_bytes, None)
    return rc, L.read_last_error().decode()


def _who(pano):
    return "read_splat_forward_pano_instances" if pano else "read_splat_forward_instances"


@pytest.mark.parametrize("pano", [False, True])
@pytest.mark.parametrize("case", ["M", "inst", "ws", "outputs", "static_xyz", "pool_xyz", "pool_ids", "first", "npts", "matrices"])
def test_forward_instances_refuses_null_pointers(case, pano):
    inst = _Inst(xyz=None if case == "pool_xyz" else FAKE, ids=None if case == "pool_ids" else FAKE, M=case != "matrices",
                 first=None if case == "first" else (0, 10, 0), npts=None if case == "npts" else (10, 20, 30), count=3, pano=pano)
    rc, msg = _call(None if case == "inst" else inst, pano, M=case != "M", ws=None if case == "ws" else FAKE, outs=case != "outputs",
                    xyz=None if case == "static_xyz" else FAKE)
    assert rc == -22 and _who(pano) in msg, (case, msg)
    assert ("no outputs" in msg) if case == "outputs" else ("null" in msg), (case, msg)


def test_forward_instances_refuses_null_static_ids():
    rc, msg = _call(_Inst(), ids=None)                                          # the pinhole entry needs explicit static ids
    assert rc == -22 and "null pointer (static xyz or ids)" in msg, msg


@pytest.mark.parametrize("pano", [False, True])
def test_forward_instances_refuses_bad_ranges(pano):
    rc, msg = _call(_Inst(count=-1, pano=pano), pano)
    assert rc == -22 and _who(pano) in msg and "count = -1 is negative" in msg, msg
    rc, msg = _call(_Inst(first=(0, -1, 0), pano=pano), pano)
    assert rc == -22 and "instance 1" in msg and "negative" in msg, msg
    rc, msg = _call(_Inst(npts=(10, 20, -30), pano=pano), pano)
    assert rc == -22 and "instance 2" in msg and "negative" in msg, msg
    rc, msg = _call(_Inst(first=(0, 11, 0), pano=pano), pano)
    assert rc == -22 and "instance 1: first + npts = 11 + 20 > inst->n = 30" in msg, msg
    rc, msg = _call(_Inst(first=(0, 1 << 62, 0), npts=(10, 1 << 62, 30), pano=pano), pano)          # no overflow in the sum
    assert rc == -22 and "instance 1" in msg and "> inst->n" in msg, msg
    # repeating and overlapping ranges, an empty one and a hidden one are fine: the call stops at the workspace size
    rc, msg = _call(_Inst(first=(0, 0, 5, 30), npts=(30, 30, 20, 0), visible=(1, 1, 0, 1), pano=pano), pano, ws_bytes=1024)
    assert rc == -12 and "workspace" in msg, msg
    rc, msg = _call(_Inst(first=(), npts=(), n=0, xyz=None, ids=None, pano=pano), pano, ws_bytes=1024)    # no instances at all
    assert rc == -12 and "workspace" in msg, msg


@pytest.mark.parametrize("pano", [False, True])
@pytest.mark.parametrize("W,H,levels", [(64, 40, 5), (40, 64, 5), (65, 48, 2), (1216, 352, 6)])
def test_forward_instances_refuses_sizes_off_the_pyramid(W, H, levels, pano):
    rc, msg = _call(_Inst(pano=pano), pano, W=W, H=H, levels=levels)
    assert rc == -22 and _who(pano) in msg, msg
    assert ("multiples of 2^(levels-1)" in msg) if levels <= 5 else ("levels" in msg), msg


def test_forward_pano_instances_refuses_bad_cameras():
    for i in (0, 7, 12, 15):
        for bad in (np.nan, np.inf):
            cam = _cam()
            cam[i] = bad
            rc, msg = _call(_Inst(pano=True), True, cam=cam)
            assert rc == -22 and "cam_host" in msg and "not finite" in msg, (i, bad, msg)
    cam = _cam()
    cam[12] = 0.3
    rc, msg = _call(_Inst(pano=True), True, cam=cam)
    assert rc == -22 and "kx" in msg and "1 / pi" in msg, msg
    inst = _Inst(pano=True)
    inst.M[1, 3] = np.nan
    rc, msg = _call(inst, True)
    assert rc == -22 and "instance 1" in msg and "not finite" in msg, msg
    inst = _Inst(pano=True, visible=(1, 0, 1))                                  # a hidden instance's camera is not looked at
    inst.M[1, 3] = np.nan
    rc, msg = _call(inst, True, ws_bytes=1024)
    assert rc == -12 and "workspace" in msg, msg


def _tables(spec, rows=FAKE):
    t = (_lib.GatherTable * max(len(spec), 1))()
    for i, (n, base, act) in enumerate(spec):
        t[i].rows_nc, t[i].n, t[i].id_base, t[i].activation = rows, n, base, act
    return t


def _gather(spec, C_=8, levels=5, count=None, tables=True, idx=True, feat=True, counts=True, null_level=None, rows=FAKE):
    L = _lib.lib()
    t = _tables(spec, rows)
    ip = [FAKE] * min(levels, 5)
    if null_level is not None:
        ip[null_level] = None
    cl = (C.c_int64 * 5)(*([16] * 5))
    rc = L.read_gather_forward_tables(t if tables else None, len(spec) if count is None else count, C_, levels,
                                      _lib.ptr_array(ip) if idx else None, cl if counts else None,
                                      _lib.ptr_array([FAKE] * min(levels, 5)) if feat else None, None)
    return rc, L.read_last_error().decode()


def test_gather_tables_refusals():
    ok = [(1000, 0, 0), (30, 1000, 1)]
    for kw in (dict(tables=False), dict(idx=False), dict(feat=False), dict(counts=False), dict(rows=None)):
        rc, msg = _gather(ok, **kw)
        assert rc == -22 and "read_gather_forward_tables" in msg and "null" in msg, (kw, msg)
    for count in (0, -1, 9):
        rc, msg = _gather(ok, count=count)
        assert rc == -22 and "count must be 1..8" in msg, msg
    for C_ in (6, 0, 3):
        rc, msg = _gather(ok, C_=C_)
        assert rc == -22 and "multiple of 4" in msg, msg
    rc, msg = _gather(ok, levels=6)
    assert rc == -22 and "levels" in msg, msg
    rc, msg = _gather([(1000, 5, 0), (30, 1005, 0)])
    assert rc == -22 and "table 0: id_base must be 0" in msg, msg
    rc, msg = _gather([(1000, 0, 0), (30, 2000, 0), (30, 1500, 0)])
    assert rc == -22 and "table 2" in msg and "does not ascend" in msg, msg
    rc, msg = _gather([(1000, 0, 0), (30, 0, 0)])
    assert rc == -22 and "table 1" in msg and "does not ascend" in msg, msg
    rc, msg = _gather([(1000, 0, 0), (30, 999, 0)])
    assert rc == -22 and "table 1" in msg and "overlaps" in msg, msg
    rc, msg = _gather([(1000, 0, 0), (30, (1 << 31) - 30, 0)])
    assert rc == -22 and "table 1" in msg and "int32 id range" in msg, msg
    rc, msg = _gather([((1 << 31), 0, 0)])
    assert rc == -22 and "int32 id range" in msg, msg
    rc, msg = _gather([(1000, 0, 0), (0, 1000, 0)])
    assert rc == -22 and "empty descriptor table" in msg, msg
    rc, msg = _gather([(1000, 0, 3)])
    assert rc == -22 and "activation" in msg, msg
    rc, msg = _gather(ok, null_level=2)
    assert rc == -22 and "null level 2" in msg, msg
    rc, msg = _gather([(1000, 0, 0), (30, 1000, 1)], rows=FAKE + 4)
    assert rc == -22 and "misaligned" in msg, msg


# ---- the model against the oracle ------------------------------------------------------------------------------------------------
W, H, N = 256, 128, 20_000


def _clusters(xyz, n_objects, size, seed):
    rng = np.random.default_rng(seed)
    labels = np.zeros(xyz.shape[0], np.int32)
    for k in range(1, n_objects + 1):
        free = np.flatnonzero(labels == 0)
        c = xyz[free[rng.integers(free.size)]]
        d = ((xyz[free] - c) ** 2).sum(1)
        labels[free[np.argpartition(d, size)[:size]]] = k
    return labels


def _translation(t):
    P = np.eye(4, dtype=np.float32)
    P[:3, 3] = np.asarray(t, np.float32)
    return P


@functools.lru_cache(maxsize=None)
def _scene():
    xyz = synthetic.make_cloud(N, 6)
    labels = _clusters(xyz, 3, 800, 21)
    M0 = camera.total_matrix(synthetic.make_proj(W, H, f=120.0), synthetic.sweep_pose(2))[0]
    return xyz, labels, M0


def _same(a, b, what):
    for l in range(im.LEVELS):
        assert np.array_equal(a[0][l], b[0][l]), f"{what}: index level {l}"
        assert np.array_equal(a[1][l].view(np.uint32), b[1][l].view(np.uint32)), f"{what}: depth level {l}"


def test_partition_list_equals_oracle_edit():
    from tests.test_gpu_objects import oracle_edit
    xyz, labels, M0 = _scene()
    static, pool, ranges = im.layout(xyz, labels)
    poses = {1: _translation((0.4, 0.1, -0.2)), 2: None, 3: _translation((-0.3, 0.0, 0.5))}
    inst = [(ranges[k - 1][0], ranges[k - 1][1], poses[k], k != 2) for k in (1, 2, 3)]
    ref = oracle_edit(xyz, labels, M0, W, H, poses, hidden={2})
    _same(im.frame(static, pool, inst, M0, W, H), ref, "model")
    _same(im.oracle_frame(static, pool, inst, M0, W, H), ref, "per-instance oracle")
    assert np.isin(ref[0][0], np.flatnonzero(labels == 1)).any()


def test_three_copies_with_the_original_hidden():
    xyz, labels, M0 = _scene()
    static, pool, ranges = im.layout(xyz, labels)
    f, n = ranges[0]
    inst = [(f, n, None, False)] + [(f, n, _translation((0.5 * j, 0.2 * j, 0.0)), True) for j in (1, 2, 3)] + \
           [(ranges[k][0], ranges[k][1], None, True) for k in (1, 2)]
    got = im.frame(static, pool, inst, M0, W, H)
    _same(got, im.oracle_frame(static, pool, inst, M0, W, H), "copies")
    # the object is on screen, and not only through its first copy
    ids1 = np.flatnonzero(labels == 1)
    one = im.frame(static, pool, [inst[1]] + inst[4:], M0, W, H)
    assert np.isin(got[0][0], ids1).sum() > 0 and not np.array_equal(got[0][0], one[0][0])


def test_a_copy_at_the_identical_pose_changes_nothing():
    xyz, labels, M0 = _scene()
    static, pool, ranges = im.layout(xyz, labels)
    P = _translation((0.2, -0.1, 0.3))
    once = [(ranges[0][0], ranges[0][1], P, True), (ranges[1][0], ranges[1][1], None, True)]
    twice = once + [(ranges[0][0], ranges[0][1], P, True), (ranges[1][0], ranges[1][1], None, True)]
    _same(im.frame(static, pool, twice, M0, W, H), im.frame(static, pool, once, M0, W, H), "model")
    _same(im.oracle_frame(static, pool, twice, M0, W, H), im.oracle_frame(static, pool, once, M0, W, H), "oracle")


def test_foreign_cluster_ids_start_at_n():
    xyz, labels, M0 = _scene()
    other = synthetic.make_cloud(N, 9)
    cut = other[_clusters(other, 1, 500, 22) == 1]
    assert cut.shape == (500, 3)
    static, pool, ranges = im.layout(xyz, labels, foreign=[cut])
    assert ranges[3] == (2400, 500) and pool[1][2400] == N and pool[1][-1] == N + 499
    # carried in front of the camera so that it wins pixels
    c = cut.astype(np.float64).mean(0)
    tgt = xyz[labels == 1].astype(np.float64).mean(0)
    inst = [(ranges[k][0], ranges[k][1], None, True) for k in range(3)] + [(2400, 500, _translation(tgt - c + (0.0, 0.0, 0.05)), True),
                                                                            (2400, 500, _translation(tgt - c + (0.6, 0.0, 0.0)), True)]
    got = im.frame(static, pool, inst, M0, W, H)
    _same(got, im.oracle_frame(static, pool, inst, M0, W, H), "foreign")
    won = got[0][0][got[0][0] >= N]
    assert won.size > 0 and won.max() < N + 500
    # a cloud without labels takes the same instances as if every label were 0
    s2, p2, r2 = im.layout(xyz, None, foreign=[cut])
    assert r2 == [(0, 500)] and s2[0].shape[0] == N
    inst2 = [(0, 500, inst[3][2], True)]
    _same(im.frame(s2, p2, inst2, M0, W, H), im.oracle_frame(s2, p2, inst2, M0, W, H), "unlabelled + foreign")
    # an exact depth tie between a scene point and a foreign one goes to the scene point: its id is smaller
    idx0 = im.frame(s2, p2, [], M0, W, H)[0][0]
    winners = np.unique(idx0[idx0 > 0])[:40]
    twin = xyz[winners]
    s3, p3, r3 = im.layout(xyz, None, foreign=[twin])
    tie = im.frame(s3, p3, [(0, 40, None, True)], M0, W, H)
    _same(tie, im.frame(s2, p2, [], M0, W, H), "tie")
    assert not (tie[0][0] >= N).any()


def test_object_matrices_equal_object_matrix_bit_for_bit():
    from read_amd.raster import object_matrices, object_matrix
    rng = np.random.default_rng(5)
    M0 = rng.standard_normal((4, 4)).astype(np.float32)
    poses = [None, np.eye(4), rng.standard_normal((4, 4)).astype(np.float32), _translation((1, -2, 0.5)), np.eye(4).tolist()] + \
            [rng.standard_normal((4, 4)) for _ in range(40)]
    got = object_matrices(M0, poses)
    assert got.dtype == np.float32 and got.shape == (45, 4, 4)
    for g, P in zip(got, poses):
        assert np.array_equal(g.view(np.uint32), object_matrix(M0, P).view(np.uint32))
    assert object_matrices(M0, []).shape == (0, 4, 4)


def test_labelled_rasteriser_lists_its_partition():
    """The partition equals the list at the host level: a labelled rasteriser's read_splat_instances holds range k of
    ``label_layout`` with M_k = object_matrix(M_0, P_k) and the flag set for label k + 1 — a label without points and an identity
    pose included.  Host arrays only: the state is what the constructor leaves, on CPU tensors."""
    import torch
    from read_amd.raster import PointCloudRasterizer, label_layout, object_matrix
    rng = np.random.default_rng(8)
    labels = rng.integers(0, 6, 400).astype(np.int32)
    labels[labels == 3] = 0                                                     # label 3 has no points
    static_ids, obj_ids, begin = label_layout(labels)
    K = len(begin) - 1
    assert K == 5 and begin[3] == begin[2]
    r = PointCloudRasterizer.__new__(PointCloudRasterizer)
    r.device, r.labels, r.n_objects, r._foreign = torch.device("cpu"), torch.from_numpy(labels), K, []
    r._start_ranges(torch.from_numpy(rng.standard_normal((obj_ids.numel(), 3)).astype(np.float32)), obj_ids, begin)
    assert sorted(r._inst) == list(range(K))
    poses = {1: _translation((0.4, 0.1, -0.2)), 2: np.eye(4), 3: rng.standard_normal((4, 4)), 4: None,
             5: torch.from_numpy(rng.standard_normal((4, 4)).astype(np.float32))}
    for k, P in poses.items():
        r.set_object_pose(k, P)
    r.set_object_visible(2, False)
    r.set_object_visible(5, False)
    r.set_object_visible(5, True)
    M0 = rng.standard_normal((4, 4)).astype(np.float32)
    s = r._instances_struct(r.instance_matrices(M0))
    assert s.count == K and s.n == obj_ids.numel() and s.xyz == r._pool_xyz.data_ptr() and s.ids == r._pool_ids.data_ptr()
    host = lambda p, ct, shape: np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), shape)
    assert np.array_equal(host(s.first, C.c_int64, (K,)), begin[:-1])
    assert np.array_equal(host(s.npts, C.c_int64, (K,)), begin[1:] - begin[:-1])
    assert host(s.visible, C.c_uint8, (K,)).tolist() == [1, 0, 1, 1, 1]
    M = host(s.M, C.c_float, (K, 4, 4))
    for k in range(1, K + 1):
        Pk = poses[k].numpy() if torch.is_tensor(poses[k]) else poses[k]
        assert np.array_equal(M[k - 1].view(np.uint32), object_matrix(M0, Pk).view(np.uint32)), k
    assert np.array_equal(M[1].view(np.uint32), M0.view(np.uint32)) and np.array_equal(M[3].view(np.uint32), M0.view(np.uint32))
    assert torch.equal(r._pool_ids, obj_ids)
    # the setters of the own instances are the object's setters: one pose and one flag per object
    r.set_instance_pose(0, None)
    r.set_instance_visible(1, True)
    assert [(k, P is None, v) for k, P, v in r._instance_list()][:2] == [(1, True, True), (2, False, True)]
    with pytest.raises(ValueError, match="itself"):
        r.remove_instance(2)


# ---- the table gather model ------------------------------------------------------------------------------------------------------
def test_table_gather_model():
    rng = np.random.default_rng(3)
    rows = [rng.standard_normal((n, 8)).astype(np.float32) for n in (1000, 30, 17)]
    idx = rng.integers(0, 1000, (2, 9, 13)).astype(np.int32)
    assert np.array_equal(im.gather_tables([(rows[0], 0, 'none')], idx), rows[0][idx])                   # T = 1: plain indexing
    t3 = [(rows[0], 0, 'none'), (rows[1], 1000, 'none'), (rows[2], 1030, 'none')]
    idx3 = rng.integers(0, 1047, (2, 9, 13)).astype(np.int32)
    idx3[0, 0, :4] = (999, 1000, 1029, 1030)
    assert np.array_equal(im.gather_tables(t3, idx3), np.concatenate(rows)[idx3])                       # the concatenated table
    # below 0: row 0 of table 0; a gap: the last row of the table before it; beyond the end: the last row of the last table
    gap = [(rows[0], 0, 'none'), (rows[1], 1200, 'sigmoid'), (rows[2], 1300, 'tanh')]
    ids = np.array([-1, -(1 << 31), 1000, 1199, 1200, 1229, 1230, 1299, 1300, 1316, 1317, (1 << 31) - 1], np.int64)
    t, loc = im.select(gap, ids)
    assert t.tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2]
    assert loc.tolist() == [0, 0, 999, 999, 0, 29, 29, 29, 0, 16, 16, 16]
    f = im.gather_tables(gap, ids)
    assert np.array_equal(f[0], rows[0][0]) and np.array_equal(f[3], rows[0][999])
    assert np.allclose(f[5], 1 / (1 + np.exp(-rows[1][29].astype(np.float64))), atol=1e-6)
    assert np.allclose(f[11], np.tanh(rows[2][16].astype(np.float64)), atol=1e-6)


# ---- Scene state, mocked at the rasteriser boundary ----------------------------------------------------------------------------------
class _FakeRaster:
    built = []

    def __init__(self, xyz, device=None, cells=True, labels=None):
        self.n = len(xyz)
        self.K = 0 if labels is None else int(np.max(labels))
        self.calls = []
        self.objects, self.inst, self._h = [], {}, 100
        _FakeRaster.built.append(self)

    def set_object_pose(self, k, P):
        self.calls.append(('pose', k))

    def set_object_visible(self, k, flag):
        self.calls.append(('visible', k, flag))

    def add_object(self, xyz):
        self.objects.append(np.asarray(xyz))
        return self.K + len(self.objects)

    def add_instance(self, k, P=None, visible=True):
        self._h += 1
        self.inst[self._h] = [k, P, visible]
        return self._h

    def set_instance_pose(self, h, P):
        self.inst[h][1] = P

    def set_instance_visible(self, h, flag):
        self.inst[h][2] = flag

    def remove_instance(self, h):
        del self.inst[h]

    def id_ranges(self):
        out, base = [(0, self.n)], self.n
        for o in self.objects:
            out.append((base, len(o)))
            base += len(o)
        return out


def _texture(n):
    return types.SimpleNamespace(texture_=np.zeros((1, 8, n), np.float32), activation='none')


def test_scene_replays_instances_and_foreign_objects(monkeypatch):
    monkeypatch.setattr(render_mod, "PointCloudRasterizer", _FakeRaster)
    _FakeRaster.built = []
    xyz = np.random.default_rng(0).standard_normal((100, 3)).astype(np.float32)
    scene = Scene(xyz)
    scene.set_object_labels(np.arange(100) % 3)                               # labels 1, 2
    with pytest.raises(ValueError, match="no object 3"):
        scene.add_object_instance(3)
    with pytest.raises(ValueError, match="PointTexture of that size"):
        scene.add_foreign_object(xyz[:7], _texture(8))
    cut, ids = scene.extract_object(2)
    assert np.array_equal(ids, np.flatnonzero(np.arange(100) % 3 == 2)) and np.array_equal(cut, xyz[ids])
    k = scene.add_foreign_object(xyz[:7] + 1.0, _texture(7))                  # before the rasteriser exists
    assert k == 3
    P = _translation((1, 2, 3))
    h_own = scene.add_object_instance(1, P)
    r1 = scene.rasterizer()
    assert len(r1.objects) == 1 and [v[0] for v in r1.inst.values()] == [1]
    h_for = scene.add_object_instance(k, None, visible=False)                 # on the live rasteriser: no rebuild
    h_gone = scene.add_object_instance(k)
    scene.set_instance_pose(h_for, P)
    scene.set_instance_visible(h_for, True)
    scene.remove_instance(h_gone)
    assert scene.rasterizer() is r1 and len(_FakeRaster.built) == 1
    assert sorted((v[0], v[2]) for v in r1.inst.values()) == [(1, True), (3, True)]
    with pytest.raises(ValueError, match="no instance"):
        scene.set_instance_pose(h_gone, None)
    k2 = scene.add_foreign_object(xyz[:5], _texture(5))                       # a live rasteriser takes it without a rebuild
    assert k2 == 4 and len(r1.objects) == 2 and scene.rasterizer() is r1
    # delete(): everything is replayed into the new rasteriser
    scene.delete()
    r2 = scene.rasterizer()
    assert r2 is not r1 and [o.shape[0] for o in r2.objects] == [7, 5]
    assert sorted((v[0], v[2]) for v in r2.inst.values()) == [(1, True), (3, True)]
    assert np.array_equal([v for v in r2.inst.values() if v[0] == 3][0][1], P)
    scene.set_instance_visible(h_own, False)                                  # the handles still work
    assert sorted((v[0], v[2]) for v in r2.inst.values()) == [(1, False), (3, True)]
    assert scene.rasterizer().id_ranges() == [(0, 100), (100, 7), (107, 5)]
    # new labels: foreign objects follow the new numbering, instances of labels that no longer exist are dropped
    scene.set_object_labels((np.arange(100) % 5 == 0).astype(np.int32))       # one label
    r3 = scene.rasterizer()
    assert r3 is not r2 and [o.shape[0] for o in r3.objects] == [7, 5]
    assert sorted(v[0] for v in r3.inst.values()) == [1, 2]                   # the own copy of label 1; foreign object 3 is now 2
    scene.set_object_labels(None)
    assert sorted(v[0] for v in scene.rasterizer().inst.values()) == [1]      # only the foreign object's instance is left
    assert scene.edited()
    scene.set_vertices(xyz)
    assert not scene.edited() and not scene.has_foreign() and scene.instances == {}


def _ogl(scene, ss=1, temporal_average=False, fmt=FMT):
    ogl = OGL.__new__(OGL)
    net = types.SimpleNamespace(engine=lambda h, w: None)
    ogl.model = types.SimpleNamespace(ss=ss, temporal_average=temporal_average, net=net, _loaded_textures=[0],
                                      _modules={'0': _texture(100)})
    ogl.viewport_size, ogl.input_format = (64, 64), fmt
    ogl.renderer = MultiscaleRender(scene, fmt, (64, 64), out_buffer_location='torch', supersampling=ss)
    fmts = fmt.replace(' ', '').split(',')
    ogl._fast_format = len(fmts) >= 4 and render_mod.is_point_id_pyramid(fmt)
    ogl.last_path, ogl.texture_ids = None, None
    return ogl


def test_foreign_object_refusals_by_name():
    xyz = np.random.default_rng(0).standard_normal((100, 3)).astype(np.float32)
    scene = Scene(xyz)
    scene.add_foreign_object(xyz[:7], _texture(7))
    assert scene.edited() and not scene.augmented()
    with pytest.raises(NotImplementedError, match="foreign objects.*MultiscaleRender"):
        MultiscaleRender(scene, FMT, (64, 64), out_buffer_location='torch').render()
    with pytest.raises(NotImplementedError, match="input_dict.*foreign objects"):
        _ogl(scene).infer({'id': 0})
    with pytest.raises(NotImplementedError, match="temporal_average.*foreign objects"):
        _ogl(scene, temporal_average=True).infer()
    with pytest.raises(NotImplementedError, match="supersampling 2.*foreign objects"):
        _ogl(scene, ss=2).infer()
    with pytest.raises(NotImplementedError, match="input format.*foreign objects"):
        _ogl(scene, fmt="uv_1d_p1, xyz_p1_ds1").infer()
    scene.set_point_discard(np.zeros(100, bool))
    with pytest.raises(NotImplementedError, match="augmentation.*foreign objects"):
        _ogl(scene).infer()
    scene.set_point_discard(None)
    st = StitchedScene([Scene(xyz), scene])
    with pytest.raises(NotImplementedError, match="foreign objects.*part 1 of a StitchedScene"):
        st.rasterizer()
    # own-object instances are refused where labels are: GL-twin tokens and augmentation
    own = Scene(xyz)
    own.set_object_labels(np.arange(100) % 3)
    own.add_object_instance(2, _translation((1, 0, 0)))
    with pytest.raises(NotImplementedError, match="xyz"):
        MultiscaleRender(own, "uv_1d_p1, xyz_p1_ds1", (64, 64), out_buffer_location='torch').render()
    own.set_point_discard(np.zeros(100, bool))
    with pytest.raises(NotImplementedError, match="augmentation"):
        MultiscaleRender(own, FMT, (64, 64), out_buffer_location='torch').render()
    # the rasteriser's GL-twin entry names its refusal before it touches a device
    from read_amd.raster import PointCloudRasterizer
    r = PointCloudRasterizer.__new__(PointCloudRasterizer)
    r.labels, r._inst = None, {}
    with pytest.raises(NotImplementedError, match="render_gl.*add_object"):
        r.render_gl(np.eye(4), 64, 64)
