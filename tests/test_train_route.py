"""The training step's routing and packing jobs, without a GPU: read_amd/train.py decides a layer's fragment orders and its dgrad
method in two pure functions (layer_route, dgrad_method), and ONE builder turns a route into the layer's packing jobs.

  * tests/golden/train_pack_jobs.json is the job table of the PARENT of the change that introduced them (the old _PackPlan over
    UNet() on CPU tensors, both BatchNorm forms): the builder must reproduce it job for job, in order.
  * the route table over the 99 executed layers, the off-net shapes where the methods part, and the module switches.
  * every packing entry point refuses what it refused before — all validation now lives in read_conv_pack_job_prepare.  The refused
    calls return before any launch, so they are safe without a device.
"""
import collections
import ctypes as C
import json
import os

import pytest

from read_amd import _lib
from read_amd import train as T
from read_amd.unet import UNet, layer_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIRECT, WINO, W4 = _lib.PACK_DIRECT, _lib.PACK_WINO, _lib.PACK_W4
READ_EINVAL = -22


def _executed_layers():
    return [(cin, cout, k, stride) for (path, cin, cout, k, stride, _elu) in layer_table() if not path.startswith("ConvsOut.")]


def test_job_table_matches_the_parent():
    with open(os.path.join(ROOT, "tests", "golden", "train_pack_jobs.json")) as f:
        rec = json.load(f)
    fields = rec["fields"][1:]
    assert rec["fields"][0] == "path" and set(fields) >= {"kind", "mode", "Cin", "Cout", "ksize", "kc", "Cp", "total", "nblocks", "first_block", "eps"}
    net = UNet()
    for form, identity in (("eval", False), ("identity", True)):
        want = rec["forms"][form]
        plan = T._PackPlan(net, identity)
        assert (plan.njobs, plan.total_blocks) == (want["njobs"], want["total_blocks"]) == (294, 25312)
        got = [[path] + [getattr(j, f) for f in fields] for path, j in plan.jobs]
        wrong = [i for i, (g, w) in enumerate(zip(got, want["jobs"])) if g != w]
        assert len(got) == len(want["jobs"]) and not wrong, f"{form}: job {wrong[0]} is {got[wrong[0]]}, the parent packed {want['jobs'][wrong[0]]}"
        counts = collections.Counter((j.kind, j.mode) for _p, j in plan.jobs)
        assert counts == {(_lib.PACK_PARAMS, 0): 99, (DIRECT, 0): 25, (DIRECT, 1): 15, (WINO, 0): 1, (WINO, 1): 5, (W4, 0): 73, (W4, 1): 76}
        # the entries the jobs fill: one per layer, buffers of the size the job writes
        by_out = {j.out: j.total for _p, j in plan.jobs}
        for _ts, e in plan.layers:
            for t in (e.params, e.fwd) + ((e.dgrad,) if e.dgrad is not None else ()):
                assert by_out.pop(t.data_ptr()) == t.numel()
        assert not by_out


def _counts(routes, **kw):
    return dict(collections.Counter(T.dgrad_method(r, 32, 48, **kw) for r in routes))


def test_route_table(monkeypatch):
    layers = _executed_layers()
    assert len(layers) == 99
    routes = [T.layer_route(*l) for l in layers]
    assert all(r[:4] == l for r, l in zip(routes, layers))
    assert collections.Counter(r.fwd for r in routes) == {DIRECT: 25, WINO: 1, W4: 73}
    assert collections.Counter(r.dgrad for r in routes) == {DIRECT: 15, WINO: 5, W4: 76, None: 3}
    assert all(r.fwd_kc == (16 if r.cin % 16 == 0 else 8) and r.dgrad_kc == 16 for r in routes)
    monkeypatch.setattr(T, "POLYPHASE_DGRAD", True)
    assert _counts(routes) == {'conv': 93, 'poly': 6}
    assert _counts(routes, polyphase=False) == {'conv': 93, 'dilated': 3, 'generic': 3}
    monkeypatch.setattr(T, "POLYPHASE_DGRAD", False)
    assert _counts(routes) == {'conv': 93, 'dilated': 3, 'generic': 3}
    assert [r for r in routes if r.stride == 2 and T.dgrad_method(r, 32, 48) == 'dilated'] == [r for r in routes if r.stride == 2 and r.k == 3]
    monkeypatch.setattr(T, "POLYPHASE_DGRAD", True)
    # off the net: where the methods part
    for (k, stride, cin), (H, W), want in (((3, 2, 32), (9, 13), 'generic'), ((3, 2, 32), (8, 13), 'generic'), ((3, 2, 32), (8, 12), 'poly'),
                                           ((3, 2, 8), (8, 12), 'dilated'), ((4, 2, 24), (8, 12), 'generic'), ((4, 2, 32), (8, 12), 'poly'),
                                           ((1, 1, 8), (9, 13), 'conv'), ((1, 1, 480), (8, 12), 'conv'), ((1, 1, 24), (7, 12), 'conv')):
        assert T.dgrad_method(T.layer_route(cin, 32, k, stride), H, W) == want, (k, stride, cin, H, W)
    with pytest.raises(ValueError):
        T.layer_route(12, 32, 3, 1)
    # the F(4x4) order: at least two 16-channel chunks and output channels in multiples of 8 — of the virtual layer for a dgrad
    assert T.layer_route(32, 32, 3, 1)[4:] == (W4, 16, W4, 16, None)
    assert T.layer_route(16, 32, 3, 1)[4:] == (WINO, 16, W4, 16, None)
    assert T.layer_route(8, 32, 3, 1)[4:] == (DIRECT, 8, WINO, 16, None)
    assert T.layer_route(32, 3, 3, 1)[4:] == (WINO, 16, WINO, 16, None)
    assert T.layer_route(64, 32, 1, 1)[4:] == (DIRECT, 16, DIRECT, 16, None)
    assert T.layer_route(32, 32, 4, 2)[4:] == (DIRECT, 16, None, 16, W4)
    assert T.layer_route(32, 3, 3, 2)[4:] == (DIRECT, 16, WINO, 16, WINO)
    # the switches
    monkeypatch.setattr(T, "USE_W4", False)
    off = [T.layer_route(*l) for l in layers]
    assert collections.Counter(r.fwd for r in off) == {DIRECT: 25, WINO: 74} and W4 not in {r.dgrad for r in off} | {r.poly for r in off}
    monkeypatch.setattr(T, "USE_W4", True)
    monkeypatch.setattr(T, "USE_WINOGRAD", False)
    off = [T.layer_route(*l) for l in layers]
    assert {r.fwd for r in off} == {DIRECT} and {r.dgrad for r in off} == {DIRECT, None} and {r.poly for r in off} == {None}
    assert _counts(off) == {'conv': 93, 'dilated': 3, 'generic': 3}
    monkeypatch.setattr(T, "USE_WINOGRAD", True)
    assert [T.layer_route(*l) for l in layers] == routes


def test_training_nodes_refuse_to_be_captured(monkeypatch):
    """GatedConvFn.forward is the door of every training path: under a stream capture it raises before any tensor or library call
    (a replayed node would run on the packed weights of the capture step)."""
    import torch
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    x, w, v = torch.zeros(4, 4, 8), torch.zeros(8, 8, 3, 3), torch.zeros(8)
    with pytest.raises(RuntimeError, match="cannot be captured"):
        T.GatedConvFn.apply(x, w, v, w, v, v, v, v, v, 3, 1, True)


# ---- argument checks: (entry point, arguments with P = any non-null pointer) that must come back READ_EINVAL before any launch
def _refused_calls():
    buf = (C.c_float * 16)()
    P = C.addressof(buf)
    w = lambda name, *a: (name, a)                           # noqa: E731
    calls = [
        w("read_conv_pack_params_device", 32, P, P, None, P, P, P, 1e-5, P, None),
        w("read_conv_pack_params_device", 32, P, P, P, P, P, None, 1e-5, P, None),
        w("read_conv_pack_params_device", 32, P, P, P, P, P, P, 1e-5, None, None),
        w("read_conv_pack_params_device", 0, P, P, P, P, P, P, 1e-5, P, None),
        w("read_conv_pack_weights_device", 32, 32, 3, 16, None, P, P, None),
        w("read_conv_pack_weights_device", 32, 32, 3, 16, P, P, None, None),
        w("read_conv_pack_weights_device", 32, 32, 2, 16, P, P, P, None),           # bad ksize
        w("read_conv_pack_weights_device", 32, 32, 5, 16, P, P, P, None),
        w("read_conv_pack_weights_device", 48, 32, 3, 12, P, P, P, None),           # bad kc
        w("read_conv_pack_weights_device", 32, 32, 3, 32, P, P, P, None),           # kc 32 is for 1x1 layers
        w("read_conv_pack_weights_device", 24, 32, 3, 16, P, P, P, None),           # Cin no multiple of kc
        w("read_conv_pack_weights_device", 4, 32, 3, 8, P, P, P, None),
        w("read_conv_pack_dgrad_device", 32, 32, 3, 16, P, None, P, None),
        w("read_conv_pack_dgrad_device", 32, 32, 3, 16, P, P, None, None),
        w("read_conv_pack_dgrad_device", 33, 32, 3, 16, P, P, P, None),             # odd Cin
        w("read_conv_pack_dgrad_device", 32, 32, 3, 12, P, P, P, None),             # bad kc
        w("read_conv_pack_dgrad_device", 32, 32, 1, 32, P, P, P, None),             # the dgrad entry point never took kc 32
        w("read_conv_pack_dgrad_device", 32, 32, 5, 16, P, P, P, None),             # bad ksize (the parent launched over nothing)
        w("read_conv_pack_wino_device", 32, 32, None, P, P, None),
        w("read_conv_pack_wino_device", 32, 32, P, P, None, None),
        w("read_conv_pack_wino_device", 24, 32, P, P, P, None),                     # Cin % 16
        w("read_conv_pack_wino_device", 8, 32, P, P, P, None),
        w("read_conv_pack_wino_device", 32, 0, P, P, P, None),
        w("read_conv_pack_w4_device", 32, 32, P, None, P, None),
        w("read_conv_pack_w4_device", 24, 32, P, P, P, None),
        w("read_conv_pack_w4_device", 8, 32, P, P, P, None),
        w("read_conv_pack_w4_device", 32, 0, P, P, P, None),
        w("read_conv_pack_dgrad_wino_device", 32, 32, P, P, None, None),
        w("read_conv_pack_dgrad_wino_device", 32, 32, None, P, P, None),
        w("read_conv_pack_dgrad_wino_device", 33, 32, P, P, P, None),               # odd Cin
        w("read_conv_pack_dgrad_wino_device", 32, 0, P, P, P, None),
        w("read_conv_pack_dgrad_w4_device", 32, 32, P, P, None, None),
        w("read_conv_pack_dgrad_w4_device", 32, 32, P, None, P, None),
        w("read_conv_pack_dgrad_w4_device", 33, 32, P, P, P, None),
        w("read_conv_pack_dgrad_w4_device", 32, 0, P, P, P, None),
    ]
    return buf, calls


def _bad_jobs():
    buf = (C.c_float * 16)()
    P = C.addressof(buf)

    def job(kind, mode=0, Cin=32, Cout=32, ksize=3, kc=16, **ptrs):
        j = _lib.PackJob()
        j.kind, j.mode, j.Cin, j.Cout, j.ksize, j.kc, j.eps = kind, mode, Cin, Cout, ksize, kc, 1e-5
        for name in ("wf", "wm", "bf", "bm", "gamma", "beta", "mean", "var", "out"):
            setattr(j, name, None if ptrs.get(name, P) is None else P)
        return j
    jobs = [job(_lib.PACK_PARAMS, out=None), job(_lib.PACK_PARAMS, gamma=None), job(_lib.PACK_PARAMS, var=None), job(_lib.PACK_PARAMS, Cout=0),
            job(DIRECT, wf=None), job(DIRECT, out=None), job(DIRECT, ksize=2), job(DIRECT, kc=12, Cin=48), job(DIRECT, kc=32), job(DIRECT, Cin=24),
            job(DIRECT, mode=1, Cin=33), job(DIRECT, mode=1, kc=12), job(DIRECT, mode=1, ksize=1, kc=32), job(DIRECT, mode=1, ksize=5),
            job(WINO, wm=None), job(WINO, Cin=24), job(WINO, Cin=8), job(WINO, mode=1, Cin=33),
            job(W4, out=None), job(W4, Cin=24), job(W4, mode=1, Cin=33), job(W4, Cout=0), job(7), job(-1)]
    return buf, jobs


def test_every_packing_entry_point_refuses_bad_arguments():
    L = _lib.lib()
    _keep, calls = _refused_calls()
    seen = set()
    for name, args in calls:
        assert getattr(L, name)(*args) == READ_EINVAL, (name, args)
        assert L.read_last_error().startswith(b"read_conv_pack_job_prepare: "), (name, args, L.read_last_error())
        seen.add(name)
    assert len(seen) == 7
    _keep2, jobs = _bad_jobs()
    for i, j in enumerate(jobs):
        for call in (lambda: L.read_conv_pack_job(C.byref(j), None), lambda: L.read_conv_pack_job_prepare(C.byref(j))):
            assert call() == READ_EINVAL and L.read_last_error(), ("job", i)
    assert L.read_conv_pack_job(None, None) == READ_EINVAL and L.read_conv_pack_job_prepare(None) == READ_EINVAL
    assert L.read_conv_pack_batch(None, 1, 1, None) == READ_EINVAL
    # a 1x1 layer's own weights do take the 32-channel chunk (prepare alone: it launches nothing)
    ok = _lib.PackJob()
    ok.kind, ok.mode, ok.Cin, ok.Cout, ok.ksize, ok.kc = DIRECT, 0, 64, 32, 1, 32
    ok.wf = ok.wm = ok.out = C.addressof(_keep2)
    assert L.read_conv_pack_job_prepare(C.byref(ok)) == 0 and (ok.Cp, ok.total, ok.nblocks) == (32, 64 * 2 * 32, 2)
