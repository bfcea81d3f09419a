"""Object selection, measured: device time of the four read_select_* calls on the 30 M-point slab, beside the time their bytes
would take at the copy bandwidth of the same run and the host NumPy model's time for the same call at 3 M points.  One JSON line.

    python tools/select_probe.py [--reps 20] [--out profiles/select_probe.json]

Cloud: synthetic.make_cloud(30 M); one view at 1216 x 352 (sweep pose 0), its level-0 frame from the rasteriser itself.
  copy_gbs              bytes moved per second by a device-to-device copy of 8 N bytes (8 N read + 8 N written)
  boxes_us[K]           read_select_boxes, K = 1, 16, 256, 1024 random oriented boxes that hold ~15 % of the slab together;
                        boxes_share[K] = the share of points some box holds (the rest walk all K boxes)
  near_us, vote_us      read_select_near (W H pixels) and read_select_vote (N points) of the view;  finish_us  read_select_finish
  *_floor_us            16 N (boxes), 20 N (vote), 8 N (finish) bytes at copy_gbs
  model_ms_3m           tests/select_model.py on the first 3 M points, the same call, one run each
Device times are HIP events around --reps launches enqueued behind a sleep kernel, per launch.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from read_amd import _lib, camera, synthetic  # noqa: E402
from read_amd.raster import PointCloudRasterizer  # noqa: E402
from read_amd.select import box_matrix  # noqa: E402
from tests import select_model as sm  # noqa: E402

W, H, N, N_MODEL = 1216, 352, 30_000_000, 3_000_000
KS = (1, 16, 256, 1024)
LO, HI = np.array([-60.0, -4.0, -120.0]), np.array([60.0, 12.0, -1.0])


def boxes_for(K, seed=5):
    rng = np.random.default_rng([seed, K])
    vol = 0.15 * float(np.prod(HI - LO)) / K
    out = np.empty((K, 12), np.float32)
    for k in range(K):
        u = (vol / 9.0) ** (1.0 / 3.0)
        size = np.array([3.0 * u, min(u, 14.0), 3.0 * u])
        lo, hi = LO + 0.3 * size, HI - 0.3 * size
        out[k] = box_matrix(lo + rng.random(3) * np.maximum(hi - lo, 0.0), size, yaw=rng.uniform(0, 2 * np.pi)).reshape(12)
    return out


def device_us(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(int(2e8))
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(1e3 * e0.elapsed_time(e1) / reps, 2)


def host_ms(fn):
    t0 = time.perf_counter()
    fn()
    return round((time.perf_counter() - t0) * 1e3, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    L = _lib.lib()
    st = _lib.stream_ptr()
    xyz = synthetic.make_cloud(N)
    r = PointCloudRasterizer(xyz)
    x_d = r.xyz
    out = {"tool": "select_probe", "device": torch.cuda.get_device_name(0), "W": W, "H": H, "n": N, "n_model": N_MODEL,
           "reps": a.reps, "boxes_us": {}, "boxes_share": {}, "model_ms_3m": {}}

    src = torch.empty(2 * N, dtype=torch.int32, device='cuda').zero_()
    dst = torch.empty_like(src)
    copy_us = device_us(lambda: dst.copy_(src), a.reps)
    out["copy_us_16n"] = copy_us
    out["copy_gbs"] = round(16.0 * N / copy_us * 1e-3, 1)
    del src, dst
    floor = lambda nbytes: round(nbytes / (out["copy_gbs"] * 1e3), 2)          # bytes / (GB/s) in us
    out["boxes_floor_us"], out["vote_floor_us"], out["finish_floor_us"] = floor(16.0 * N), floor(20.0 * N), floor(8.0 * N)

    labels = torch.empty(N, dtype=torch.int32, device='cuda')
    xm = xyz[:N_MODEL]
    for K in KS:
        b = boxes_for(K)
        lab = np.arange(1, K + 1, dtype=np.int32)
        b_d, l_d = torch.from_numpy(b).cuda(), torch.from_numpy(lab).cuda()
        out["boxes_us"][str(K)] = device_us(lambda: _lib.check(L.read_select_boxes(
            x_d.data_ptr(), N, b_d.data_ptr(), l_d.data_ptr(), K, None, labels.data_ptr(), st), "read_select_boxes"), a.reps)
        out["boxes_share"][str(K)] = round(float((labels != 0).float().mean()), 4)
        want = None

        def model():
            nonlocal want
            want = sm.label_boxes(xm, b, lab)
        out["model_ms_3m"][f"boxes_{K}"] = host_ms(model)
        assert np.array_equal(labels[:N_MODEL].cpu().numpy(), want), f"K = {K}: kernel and model differ"
        print(f"# K = {K}: {out['boxes_us'][str(K)]} us, model {out['model_ms_3m'][f'boxes_{K}']} ms", file=sys.stderr, flush=True)

    # one view: the rasteriser's own level 0, a label image of two rectangles
    M = camera.total_matrix(synthetic.make_proj(W, H), synthetic.sweep_pose(0))[0].reshape(16)
    Mp = M.ctypes.data_as(C.POINTER(C.c_float))
    idx, dep = r.render(M, W, H, 1)
    mask = np.zeros((H, W), np.int32)
    mask[60:300, 100:500], mask[100:340, 600:1100] = 1, 2
    m_d = torch.from_numpy(mask).cuda()
    near = torch.empty(W * H, dtype=torch.float32, device='cuda')
    state = torch.zeros(N, dtype=torch.int32, device='cuda')
    scale, slack = float(np.float32(1.05)), 0.25
    out["near_us"] = device_us(lambda: _lib.check(L.read_select_near(
        x_d.data_ptr(), N, Mp, W, H, idx[0].data_ptr(), dep[0].data_ptr(), near.data_ptr(), st), "read_select_near"), a.reps)
    state.zero_()
    _lib.check(L.read_select_vote(x_d.data_ptr(), N, Mp, W, H, near.data_ptr(), m_d.data_ptr(), scale, slack, state.data_ptr(), st),
               "read_select_vote")
    first = state.clone()
    out["seen_share"] = round(float((first != 0).float().mean()), 4)
    state.zero_()                                                # timed from zero: a few more launches than 255 views would wrap
    out["vote_us"] = device_us(lambda: _lib.check(L.read_select_vote(
        x_d.data_ptr(), N, Mp, W, H, near.data_ptr(), m_d.data_ptr(), scale, slack, state.data_ptr(), st), "read_select_vote"),
        min(a.reps, 200))
    out["finish_us"] = device_us(lambda: _lib.check(L.read_select_finish(
        first.data_ptr(), N, 1, 1, 2, None, labels.data_ptr(), st), "read_select_finish"), a.reps)
    i0, d0 = idx[0].cpu().numpy(), dep[0].cpu().numpy()
    res = {}
    out["model_ms_3m"]["near"] = host_ms(lambda: res.update(near=sm.near_image(xyz, M, i0, d0)))
    assert np.array_equal(res["near"].view(np.uint32), near.cpu().numpy().view(np.uint32)), "near: kernel and model differ"
    out["model_ms_3m"]["vote"] = host_ms(lambda: res.update(
        state=sm.vote(np.zeros(N_MODEL, np.uint32), xm, M, W, H, res["near"], mask, np.float32(1.05), np.float32(slack))))
    assert np.array_equal(res["state"], first[:N_MODEL].cpu().numpy().view(np.uint32)), "vote: kernel and model differ"
    out["model_ms_3m"]["finish"] = host_ms(lambda: res.update(labels=sm.finish(res["state"], 1, (1, 2))))
    assert np.array_equal(res["labels"], labels[:N_MODEL].cpu().numpy()), "finish: kernel and model differ"
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
