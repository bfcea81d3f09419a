"""Scene editing, third verb (add), measured: what the rasteriser pays for I instances of one object, and what the gather over
several descriptor tables pays against the plain gather.  One JSON line.

    python tools/instances_probe.py [--laps 3] [--out profiles/instances_probe.json]

Scene: 30 M points of synthetic.make_cloud at 1216 x 352 on the first 64 poses of the sweep, every camera announced one frame ahead
(the scene of tools/objects_probe.py); ONE object of 25 k points (the points nearest to a random centre), its original hidden,
drawn as I = 0 / 16 / 64 / 256 instances, every instance re-posed every frame (a turn about the object's centre and a drift).
  raster_us[I]         rasteriser per frame, HIP events around a lap of 64 pre-bound calls (PointCloudRasterizer.bind) enqueued
                       behind a sleep kernel: device time, mean of --laps laps.  I = 0 is the baseline of this probe (the instance
                       path with nothing to draw); profiles/objects_probe.json holds the parent's 16-object frame for comparison
  host_ms_per_frame[I] host time to enqueue one frame (I set_instance_pose calls, the I matrices, the call), untimed lap
  slot3_us[I]          read_splat_profile_last slot 3 of one frame: pass B + the ceil(I / 32) range launches
  gather_us            read_gather_forward over the last frame's pyramid, and read_gather_forward_tables with the same table cut
                       into T = 1, 2 and 8 id ranges (views, nothing copied); HIP events around 200 launches behind a sleep kernel,
                       mean of --laps laps; gather_floor_us = the bytes a gather must move (4 + 4 C + 4 C per pixel) at 8 TB/s
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
from read_amd.texture import gather_pyramid, gather_tables_pyramid, texture_to_rows  # noqa: E402

W, H, N, POSES, OBJ_POINTS = 1216, 352, 30_000_000, 64, 25_000
COUNTS = (0, 16, 64, 256)
HBM_TBS = 8.0


def object_label(xyz, seed=7):
    c = xyz[np.random.default_rng(seed).integers(xyz.shape[0])]
    labels = np.zeros(xyz.shape[0], np.int32)
    labels[np.argpartition(((xyz - c) ** 2).sum(1), OBJ_POINTS)[:OBJ_POINTS]] = 1
    return labels


def instance_pose(f, i, c):
    a = 0.05 * f * (1 + i % 3) + 0.4 * i
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    P = np.eye(4)
    P[:3, :3] = R
    P[:3, 3] = c - R @ c + np.array([0.02 * f + 0.7 * (i % 16) - 5.0, 0.3 * (i // 64), -0.01 * f - 0.9 * ((i // 16) % 4)])
    return P.astype(np.float32)


def sleep_cycles_per_ms():
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(int(1e7))
    torch.cuda.synchronize()
    e0.record()
    torch.cuda._sleep(int(1e8))
    e1.record()
    torch.cuda.synchronize()
    return 1e8 / e0.elapsed_time(e1)


def lap_device_us(frame, laps):
    """-> (device us per frame, per lap, host ms per frame to enqueue).  The sleep kernel in front of a lap lasts 1.5 x the host
    time the untimed lap took to enqueue (at least 0.5 s), so the lap is device time however many instances the host walks."""
    t0 = time.perf_counter()
    for k in range(POSES):                                      # one untimed lap: lists, seeds and marks settled
        frame(k)
    host_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    cycles = int(max(500.0, 1.5 * host_ms) * sleep_cycles_per_ms())
    per = []
    for _ in range(laps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(cycles)
        e0.record()
        for k in range(POSES):
            frame(k)
        e1.record()
        torch.cuda.synchronize()
        per.append(1e3 * e0.elapsed_time(e1) / POSES)
    return round(float(np.mean(per)), 2), [round(x, 2) for x in per], round(host_ms / POSES, 3)


def launches_us(fn, laps, n=200):
    fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(laps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(int(1e9))
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        per.append(1e3 * e0.elapsed_time(e1) / n)
    return round(float(np.mean(per)), 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--laps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    xyz = synthetic.make_cloud(N)
    labels = object_label(xyz)
    cent = xyz[labels == 1].astype(np.float64).mean(0)
    proj = synthetic.make_proj(W, H)
    totals = [camera.total_matrix(proj, synthetic.sweep_pose(k))[0] for k in range(POSES)]
    out = {"tool": "instances_probe", "device": torch.cuda.get_device_name(0), "W": W, "H": H, "n": N, "poses": POSES,
           "object_points": OBJ_POINTS, "laps": a.laps, "raster_us": {}, "raster_us_laps": {}, "slot3_us": {}, "launches": {},
           "host_ms_per_frame": {}}
    parent = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "objects_probe.json")
    if os.path.exists(parent):
        p = json.load(open(parent))
        out["parent_objects_probe"] = {k: p[k] for k in ("raster_us_objects", "raster_us_no_labels") if k in p}

    r = PointCloudRasterizer(xyz, labels=labels)
    r.set_object_visible(1, False)
    idx, dep = r.render(totals[0], W, H)
    call = r.bind(W, H, 5, (idx, dep), totals)
    handles = []
    L = _lib.lib()
    for count in COUNTS:
        while len(handles) < count:
            handles.append(r.add_instance(1))
        if count == 0:
            r.remove_instance(r.add_instance(1))                # the instance path with nothing to draw
        table = [[instance_pose(f, i, cent) for i in range(count)] for f in range(POSES)]

        def frame(k):
            for h, P in zip(handles, table[k]):
                r.set_instance_pose(h, P)
            call(k, (k + 1) % POSES)
        out["raster_us"][str(count)], out["raster_us_laps"][str(count)], out["host_ms_per_frame"][str(count)] = \
            lap_device_us(frame, a.laps)
        out["launches"][str(count)] = (count + 31) // 32
        _lib.check(L.read_tuning_set(b"splat_prof", 1), "read_tuning_set")
        frame(0)
        frame(1)
        ms5 = (C.c_float * 5)()
        _lib.check(L.read_splat_profile_last(ms5), "read_splat_profile_last")
        _lib.check(L.read_tuning_set(b"splat_prof", 0), "read_tuning_set")
        out["slot3_us"][str(count)] = round(1e3 * float(ms5[3]), 2)

    # the gathers over the last frame's pyramid
    rows = texture_to_rows(torch.from_numpy(synthetic.make_descriptors(N)).cuda())
    feat = gather_pyramid(rows, idx)
    px = sum(int(i.numel()) for i in idx)
    out["gather_floor_us"] = round(px * (4 + 2 * 4 * rows.shape[1]) / (HBM_TBS * 1e12) * 1e6, 2)
    out["gather_us"] = {"plain": launches_us(lambda: gather_pyramid(rows, idx, out=feat), a.laps)}
    for T in (1, 2, 8):
        cuts = [N * t // T for t in range(T + 1)]
        tabs = [(rows[lo:hi], lo, 'none') for lo, hi in zip(cuts[:-1], cuts[1:])]
        ref = [f.clone() for f in feat]
        got = gather_tables_pyramid(tabs, idx)
        assert all(torch.equal(x, y) for x, y in zip(got, ref)), f"T = {T}: the table gather differs from the plain gather"
        out["gather_us"][f"tables_{T}"] = launches_us(lambda: gather_tables_pyramid(tabs, idx, out=feat), a.laps)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
