"""CPU: the C ABI of scene editing (read_splat_cells_build_ids, read_splat_forward_objects) — exported, bound, and refusing bad
arguments before any device work — plus the two host-side pieces every frame depends on: the object matrix helper and the label
bookkeeping.  Frames are checked on the GPU (tests/test_gpu_objects.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from read_amd import _lib
from read_amd.raster import MAX_LABEL, label_layout, object_matrix

FAKE = 1 << 20          # a 256-byte aligned non-null address: the calls below fail on their arguments and never touch it
NEW = ("read_splat_cells_build_ids", "read_splat_forward_objects")


def test_symbols_are_exported_and_bound():
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    assert _lib.lib().read_abi_version() == 3


def test_objects_struct_layout():
    # const float *, const int32_t *, int64_t, int (+4 pad), const int64_t *, const float *, const unsigned char *
    assert C.sizeof(_lib.SplatObjects) == 56
    assert [getattr(_lib.SplatObjects, f).offset for f in ("xyz", "ids", "n", "count", "begin", "M", "visible")] == \
        [0, 8, 16, 24, 32, 40, 48]


def test_build_ids_refuses_bad_arguments():
    L = _lib.lib()
    n = 5000
    nbytes, sbytes = L.read_splat_cells_bytes(n), L.read_splat_cells_build_scratch_bytes(n)
    for args in ((None, FAKE, FAKE, FAKE), (FAKE, None, FAKE, FAKE), (FAKE, FAKE, None, FAKE), (FAKE, FAKE, FAKE, None)):
        rc = L.read_splat_cells_build_ids(args[0], args[1], n, args[2], nbytes, args[3], sbytes, None)
        msg = L.read_last_error().decode()
        assert rc == -22 and "read_splat_cells_build_ids" in msg and "null" in msg, (args, msg)
    rc = L.read_splat_cells_build_ids(FAKE, FAKE, n, FAKE, nbytes, FAKE, sbytes - 1, None)
    msg = L.read_last_error().decode()
    assert rc == -22 and "read_splat_cells_build_ids" in msg and "scratch" in msg, msg
    rc = L.read_splat_cells_build_ids(FAKE, FAKE, 0, FAKE, nbytes, FAKE, sbytes, None)
    assert rc == -22 and "out of range" in L.read_last_error().decode()


class _Objs:
    """A read_splat_objects whose host arrays stay alive."""

    def __init__(self, begin, n=None, xyz=FAKE, ids=FAKE, M=True, visible=None):
        self.begin = None if begin is None else np.asarray(begin, np.int64)
        count = 0 if self.begin is None else len(self.begin) - 1
        self.M = np.zeros((max(count, 1), 16), np.float32) if M else None
        self.visible = None if visible is None else np.asarray(visible, np.uint8)
        n = int(self.begin[-1]) if n is None and self.begin is not None else (n or 0)
        self.s = _lib.SplatObjects(xyz, ids, n, count, None if self.begin is None else self.begin.ctypes.data,
                                   None if self.M is None else self.M.ctypes.data,
                                   None if self.visible is None else self.visible.ctypes.data)


def _call(objs, W=64, H=48, levels=5, xyz=FAKE, ids=FAKE, n_static=100, M=True, ws=FAKE, outs=True, cells=None):
    L = _lib.lib()
    Mh = np.eye(4, dtype=np.float32).reshape(16)
    idx = _lib.ptr_array([FAKE] * levels) if outs else None
    rc = L.read_splat_forward_objects(xyz, ids, cells, n_static, Mh.ctypes.data_as(C.POINTER(C.c_float)) if M else None, W, H,
                                      levels, C.byref(objs.s) if objs is not None else None, idx, None, ws, 1 << 40, None)
    return rc, L.read_last_error().decode()


@pytest.mark.parametrize("case", ["M", "objs", "ws", "outputs", "static_xyz", "static_ids", "obj_xyz", "obj_ids", "begin", "matrices"])
def test_forward_objects_refuses_null_pointers(case):
    objs = _Objs([0, 10, 30],
                 xyz=None if case == "obj_xyz" else FAKE, ids=None if case == "obj_ids" else FAKE, M=case != "matrices")
    if case == "begin":
        objs.s.begin = None
    rc, msg = _call(None if case == "objs" else objs, M=case != "M", ws=None if case == "ws" else FAKE, outs=case != "outputs",
                    xyz=None if case == "static_xyz" else FAKE, ids=None if case == "static_ids" else FAKE)
    assert rc == -22 and "read_splat_forward_objects" in msg, (case, msg)
    assert ("no outputs" in msg) if case == "outputs" else ("null" in msg), (case, msg)


def test_forward_objects_refuses_bad_ranges():
    rc, msg = _call(_Objs([0, 10, 5, 30]))
    assert rc == -22 and "not monotone at 1" in msg, msg
    rc, msg = _call(_Objs([0, 10, 30], n=31))
    assert rc == -22 and "begin[count] = 30 != objs->n = 31" in msg, msg
    rc, msg = _call(_Objs([3, 10, 30]))
    assert rc == -22 and "begin[0]" in msg, msg
    rc, msg = _call(_Objs(None, n=7))
    assert rc == -22 and "!= objs->n = 7" in msg, msg


@pytest.mark.parametrize("W,H,levels", [(64, 40, 5), (40, 64, 5), (65, 48, 2), (1216, 352, 6)])
def test_forward_objects_refuses_sizes_off_the_pyramid(W, H, levels):
    rc, msg = _call(_Objs([0, 10, 30]), W=W, H=H, levels=levels)
    assert rc == -22 and "read_splat_forward_objects" in msg, msg
    assert ("multiples of 2^(levels-1)" in msg) if levels <= 5 else ("levels" in msg), msg


def test_forward_objects_checks_precede_device_work():
    # a valid call shape, but the workspace is too small: ENOMEM, and still nothing launched (no GPU here)
    L = _lib.lib()
    objs = _Objs([0, 10, 30])
    Mh = np.eye(4, dtype=np.float32).reshape(16)
    idx = _lib.ptr_array([FAKE] * 5)
    rc = L.read_splat_forward_objects(FAKE, FAKE, None, 100, Mh.ctypes.data_as(C.POINTER(C.c_float)), 64, 48, 5, C.byref(objs.s),
                                      idx, None, FAKE, 1024, None)
    assert rc == -12 and "workspace" in L.read_last_error().decode()


def test_object_matrix_identity_is_m0_itself():
    rng = np.random.default_rng(3)
    M0 = rng.standard_normal((4, 4)).astype(np.float32)
    negzero = np.eye(4, dtype=np.float32)
    negzero[0, 1] = -0.0
    for P in (None, np.eye(4), np.eye(4, dtype=np.float32), np.eye(4).tolist(), negzero):
        out = object_matrix(M0, P)
        assert out.dtype == np.float32 and np.array_equal(out.view(np.uint32), M0.view(np.uint32))


def test_object_matrix_is_the_float32_product():
    rng = np.random.default_rng(4)
    for _ in range(50):
        M0 = rng.standard_normal((4, 4)).astype(np.float32)
        P = rng.standard_normal((4, 4)).astype(np.float32)
        want = np.empty((4, 4), np.float32)
        for i in range(4):
            for k in range(4):
                acc = np.float32(M0[i, 0] * P[0, k])
                for j in range(1, 4):
                    acc = np.float32(acc + np.float32(M0[i, j] * P[j, k]))
                want[i, k] = acc
        got = object_matrix(M0, P)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
        assert np.allclose(got, M0.astype(np.float64) @ P.astype(np.float64), rtol=1e-5, atol=1e-5)
    # a translation moves points: M0 @ P applied to x equals M0 applied to P x
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = (1.0, -2.0, 0.5)
    x = np.array([0.25, 0.5, -1.0, 1.0], np.float32)
    M0 = rng.standard_normal((4, 4)).astype(np.float32)
    assert np.allclose(object_matrix(M0, T) @ x, M0 @ (T @ x), atol=1e-5)


def test_label_layout_offsets_and_ids():
    labels = np.array([0, 2, 1, 0, 2, 2, 0, 1, 4], np.int64)            # label 3 has no points
    static_ids, obj_ids, begin = label_layout(labels)
    assert static_ids.dtype == torch.int32 and obj_ids.dtype == torch.int32 and begin.dtype == np.int64
    assert static_ids.tolist() == [0, 3, 6]
    assert obj_ids.tolist() == [2, 7, 1, 4, 5, 8]                       # label after label, ascending ids within a label
    assert begin.tolist() == [0, 2, 5, 5, 6]                             # K = 4 objects; object 3 is an empty range
    # every point appears exactly once
    assert sorted(static_ids.tolist() + obj_ids.tolist()) == list(range(labels.size))


def test_label_layout_edge_cases():
    s, o, b = label_layout(np.array([3, 1, 1, 3], np.int32))              # label 0 absent: an empty static part
    assert s.numel() == 0 and o.tolist() == [1, 2, 0, 3] and b.tolist() == [0, 2, 2, 4]
    s, o, b = label_layout(torch.zeros(5, dtype=torch.int64))             # only the static part: no objects
    assert s.tolist() == [0, 1, 2, 3, 4] and o.numel() == 0 and b.tolist() == [0]
    s, o, b = label_layout(np.zeros(0, np.int64))                         # no points at all
    assert s.numel() == 0 and o.numel() == 0 and b.tolist() == [0]
    s, o, b = label_layout(np.array([MAX_LABEL, 0]))
    assert b.shape == (MAX_LABEL + 1,) and b[-1] == 1 and b[-2] == 0
    for bad in (np.array([0, -1]), np.array([MAX_LABEL + 1]), np.array([0.0, 1.0]), np.zeros((2, 2), np.int64)):
        with pytest.raises(ValueError):
            label_layout(bad)


def test_scene_edits_refuse_tokens_that_ignore_them():
    from read_amd.render import MultiscaleRender, Scene
    xyz = np.random.default_rng(0).standard_normal((100, 3)).astype(np.float32)
    scene = Scene(xyz)
    with pytest.raises(ValueError):
        scene.set_object_pose(1, np.eye(4))                               # no labels yet
    with pytest.raises(ValueError):
        scene.set_object_labels(np.zeros(99, np.int32))
    scene.set_object_labels(np.arange(100) % 3)
    scene.set_object_pose(2, np.eye(4))
    scene.set_object_visible(1, False)
    assert scene.edited() and not scene.augmented()                       # edits keep OGL.infer on its fast path
    fmt = "uv_1d_p1, uv_1d_p1_ds1, uv_1d_p1_ds2, uv_1d_p1_ds3"
    for bad in ("xyz_p1_ds1", "colors_p1_ds1", "uv_1d_p2_ds1", "uv_1d_ps2_ds1", "depth_p1_ds1"):
        tokens = f"uv_1d_p1, {bad}"
        with pytest.raises(NotImplementedError, match=bad.split('_')[0]):
            MultiscaleRender(scene, tokens, (64, 64), out_buffer_location='torch').render()
    with pytest.raises(NotImplementedError, match="multiples of 8"):             # a pyramid the sizes cannot serve
        MultiscaleRender(scene, fmt, (68, 64), out_buffer_location='torch').render()
    scene.set_point_discard(np.zeros(100, bool))
    with pytest.raises(NotImplementedError, match="augmentation"):
        MultiscaleRender(scene, fmt, (64, 64), out_buffer_location='torch').render()
