"""The LiDAR sweep, measured: what a 64 x 2048 sweep of the whole cloud costs, beside the nearest existing pass.

    python tools/lidar_probe.py [--laps 3] [--out profiles/lidar_probe.json]

Cloud: the 30 M-point slab (synthetic.make_cloud) on the first 64 poses of the sweep, one process.  Sensor: 64 beams evenly over
-24.8 .. 2 degrees, 2048 columns over 360 degrees, returns from 0.5 to 120 m.
  sweep_us            one sweep with the see-through filter (window (1, 2), rel 0.05), every output written: HIP events around a
                      lap of 64 sweep_lidar calls enqueued behind a sleep kernel, so the lap is device time; mean of --laps laps
  sweep_nofilter_us   the same with window (0, 0)
  tail_us             the three image launches alone (filter + unpack + counts, scan, scatter + reset): a sweep of no points
  pano_us             render_pano at levels = 1 on a 2048 x 64 image of the same cloud, steady state (warm-started frames)
  pano_no_seeds_us    the same with read_tuning_set("splat_seeds", 0): the panorama pass as the sweep runs it, without a warm start
  floor_us            the byte floor 12 N / 8 TB/s, the same for both passes
  returns             kept returns of the first pose, with and without the filter
No threshold is set on any of these."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from read_amd import _lib, camera, lidar, synthetic  # noqa: E402
from read_amd.raster import PointCloudRasterizer  # noqa: E402

N, POSES = 30_000_000, 64
BEAMS, COLUMNS = 64, 2048


def lap_us(call, laps):
    for k in range(POSES):                                       # one untimed lap
        call(k)
    torch.cuda.synchronize()
    per = []
    for _ in range(laps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(int(1.5e9))
        e0.record()
        for k in range(POSES):
            call(k)
        e1.record()
        torch.cuda.synchronize()
        per.append(1e3 * e0.elapsed_time(e1) / POSES)
    return round(float(np.mean(per)), 2), [round(x, 2) for x in per]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--laps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lidar_probe.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    L = _lib.lib()
    xyz = synthetic.make_cloud(N)
    views = [synthetic.sweep_pose(k) for k in range(POSES)]
    out = {"tool": "lidar_probe", "device": torch.cuda.get_device_name(0), "n": N, "poses": POSES, "laps": a.laps,
           "beams": BEAMS, "columns": COLUMNS, "floor_us": round(12.0 * N / 8e12 * 1e6, 2)}
    r = PointCloudRasterizer(xyz, cells=False)
    elev = np.linspace(-24.8, 2.0, BEAMS)
    for name, window in (("sweep_nofilter", (0, 0)), ("sweep", (1, 2))):
        sensor = lidar.LidarSensor(elev, COLUMNS, window=window)
        cams = [sensor.camera(v) for v in views]
        sw = r.sweep_lidar(sensor, cams[0])
        out.setdefault("returns", {})[name] = sw.count
        out[name + "_us"], out[name + "_us_laps"] = lap_us(lambda k: r.sweep_lidar(sensor, cams[k], out=sw), a.laps)
    ws = r._lidar_workspace(BEAMS, COLUMNS)
    out["tail_us"], out["tail_us_laps"] = lap_us(lambda k: lidar.sweep(sensor, cams[k], None, None, 0, None, ws, sw), a.laps)
    W, H = COLUMNS, BEAMS
    proj = synthetic.make_proj(W, H)
    pcams = [camera.pano_camera(proj, v, 360.0) for v in views]
    idx, dep = r.render_pano(pcams[0], W, H, 1)
    out["pano_covered_pixels"] = int((dep[0] != 0).sum())
    call = lambda k: r.render_pano(pcams[k], W, H, 1, out=(idx, dep))
    out["pano_us"], out["pano_us_laps"] = lap_us(call, a.laps)
    _lib.check(L.read_tuning_set(b"splat_seeds", 0))
    try:
        out["pano_no_seeds_us"], out["pano_no_seeds_us_laps"] = lap_us(call, a.laps)
    finally:
        _lib.check(L.read_tuning_set(b"splat_seeds", 1))
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
