"""CPU: read_flow_frame in the C ABI — exported, listed in _lib.SIGNATURES, and every READ_EINVAL condition of include/read_hip.h
returns its message before any device work (the library is loaded without a GPU: a launch would fail with another code)."""
import ctypes as C

import numpy as np
import pytest

from read_amd import _lib


def test_symbol_and_struct():
    L = C.CDLL(_lib.LIB_PATH)
    assert hasattr(L, "read_flow_frame") and "read_flow_frame" in _lib.SIGNATURES
    assert _lib.SIGNATURES["read_flow_frame"][1][0]._type_ is _lib.FlowArgs
    assert _lib.READ_FLOW_STATES == 8 and _lib.READ_FLOW_STATS == 4
    assert _lib.lib().read_abi_version() == 3
    names = [f[0] for f in _lib.FlowArgs._fields_]
    assert names[:9] == [f[0] for f in _lib.AnnotateArgs._fields_][:9], "the cloud, labels, foreign ranges and pool mirror the annotation's"
    assert names[-6:] == ["flow", "depth_next", "state", "counts", "stats", "unmatched"]


def _args(**kw):
    """A call with I = 2, K = 2 (one own, one foreign object) whose device pointers are small non-null numbers: nothing is dereferenced
    on the device side before the checks are through, and every check fails before device work."""
    keep = dict(obj=np.array([1, 2], np.int32), M0=np.eye(4, dtype=np.float32).reshape(16).copy(),
                M0_next=np.eye(4, dtype=np.float32).reshape(16).copy(),
                foreign=(_lib.AnnotateForeign * 1)(_lib.AnnotateForeign(100, 5, 10)))
    a = _lib.FlowArgs()
    d = 0x1000
    a.xyz, a.n, a.labels, a.K_own, a.n_foreign, a.foreign = d, 100, d, 1, 1, keep['foreign']
    a.pool_xyz, a.pool_n, a.count = d, 15, 2
    a.obj, a.M0, a.M0_next = (keep[k].ctypes.data for k in ('obj', 'M0', 'M0_next'))
    a.d_M = a.d_visible = a.d_obj_begin = a.d_obj_list = a.d_M_next = a.d_visible_next = d
    a.idx0 = a.depth0 = a.idx0_next = a.depth0_next = d
    a.flow = a.depth_next = a.state = a.counts = a.stats = a.unmatched = d
    a.W, a.H = 80, 48
    for k, v in kw.items():
        if k == 'foreign_range':
            keep['foreign'][0] = _lib.AnnotateForeign(*v)
        elif k in keep and v is not None:
            if isinstance(v, tuple):
                keep[k][v[0]] = v[1]
            else:
                keep[k][...] = v
        else:
            setattr(a, k, v)
    return a, keep


@pytest.mark.parametrize("change,word", [
    (dict(idx0=None), b"null pointer (idx0"), (dict(depth0_next=None), b"null pointer (idx0"), (dict(flow=None), b"null pointer (flow"),
    (dict(state=None), b"null pointer (flow"), (dict(counts=None), b"null pointer (flow"), (dict(unmatched=None), b"null pointer (flow"),
    (dict(flow=0x1004), b"8-byte aligned"), (dict(M0=None), b"M0 / M0_next"), (dict(M0_next=None), b"M0 / M0_next"),
    (dict(xyz=None), b"xyz is null"), (dict(pool_xyz=None), b"pool_xyz"), (dict(foreign=None), b"foreign / pool_xyz"),
    (dict(obj=None), b"host table"), (dict(d_M_next=None), b"device table"), (dict(d_visible_next=None), b"device table"),
    (dict(d_obj_list=None), b"device table"), (dict(stats=None), b"stats"),
    (dict(W=1 << 16, H=1 << 15), b"W * H"), (dict(W=0), b"W/H"), (dict(H=-3), b"W/H"),
    (dict(n=-1), b"n = -1"), (dict(count=-1), b"count = -1"), (dict(K_own=-1), b"K_own"), (dict(pool_n=-1), b"pool_n"),
    (dict(n_foreign=8), b"n_foreign = 8"), (dict(n_foreign=-1), b"n_foreign = -1"),
    (dict(obj=[1, 3]), b"object 3 outside [1, 2]"), (dict(obj=[0, 1]), b"object 0 outside"),
    (dict(n=101), b"ascend from n"),                                  # the foreign base 100 lies inside the cloud's ids
    (dict(foreign_range=(100, 5, 11)), b"past the pool"), (dict(foreign_range=(100, -1, 0)), b"ascend from n"),
    (dict(foreign_range=(2 ** 31 - 3, 5, 10)), b"ids stay in int32"),
    (dict(M0=(5, np.inf)), b"M0[5] is not finite"), (dict(M0=(0, np.nan)), b"M0[0] is not finite"),
    (dict(M0_next=(15, -np.inf)), b"M0_next[15] is not finite"),
])
def test_bad_arguments_are_refused_before_any_device_work(change, word):
    a, keep = _args(**change)
    L = _lib.lib()
    assert L.read_flow_frame(C.byref(a), None) == -22
    msg = L.read_last_error()
    assert b"read_flow_frame" in msg and word in msg, msg


def test_null_args():
    L = _lib.lib()
    assert L.read_flow_frame(None, None) == -22 and b"read_flow_frame: args is null" in L.read_last_error()
