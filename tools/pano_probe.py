"""The panorama camera, measured: what the rasteriser costs per frame when the whole cloud is read under a cylindrical camera.

    python tools/pano_probe.py [--laps 3] [--out profiles/pano_probe.json]

Cloud: the 30 M-point slab (synthetic.make_cloud) on the first 64 poses of the sweep.  Per configuration (2432 x 352 at 360
degrees, 1216 x 352 at 120 degrees):
  steady_us       rasteriser per frame, steady state (every frame warm-started from its predecessor's winners): HIP events around
                  a lap of 64 render_pano calls enqueued behind a sleep kernel, so the lap is device time; mean of --laps laps
  first_us        the first frame on a fresh workspace (no seeds), HIP events around the one call; mean of three workspaces
  no_seeds_us     the steady lap with read_tuning_set("splat_seeds", 0): what the warm start is worth
  floor_us        the byte floor 12 N / 8 TB/s
and, in the same run, pinhole_cells_us: the pinhole cell path at 1216 x 352 (pre-bound calls, cameras announced one frame ahead).
No threshold is set on any of these."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from read_amd import _lib, camera, synthetic  # noqa: E402
from read_amd.raster import PointCloudRasterizer  # noqa: E402

N, POSES = 30_000_000, 64
CONFIGS = ((2432, 352, 360.0), (1216, 352, 120.0))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pano_probe.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    L = _lib.lib()
    xyz = synthetic.make_cloud(N)
    views = [synthetic.sweep_pose(k) for k in range(POSES)]
    out = {"tool": "pano_probe", "device": torch.cuda.get_device_name(0), "n": N, "poses": POSES, "laps": a.laps,
           "floor_us": round(12.0 * N / 8e12 * 1e6, 2), "configs": []}
    r = PointCloudRasterizer(xyz)
    for W, H, hfov in CONFIGS:
        proj = synthetic.make_proj(W, H)
        cams = [camera.pano_camera(proj, v, hfov) for v in views]
        idx, dep = r.render_pano(cams[0], W, H)
        cfg = {"W": W, "H": H, "hfov_deg": hfov}
        covered = int((dep[0] != 0).sum())
        cfg["covered_pixels"] = covered
        first = []
        for _ in range(3):
            r._workspaces.clear()
            r._workspace(1, W, H)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r.render_pano(cams[0], W, H, out=(idx, dep))
            e1.record()
            torch.cuda.synchronize()
            first.append(1e3 * e0.elapsed_time(e1))
        cfg["first_us"], cfg["first_us_runs"] = round(float(np.mean(first)), 2), [round(x, 2) for x in first]
        call = lambda k: r.render_pano(cams[k], W, H, out=(idx, dep))
        cfg["steady_us"], cfg["steady_us_laps"] = lap_us(call, a.laps)
        _lib.check(L.read_tuning_set(b"splat_seeds", 0))
        try:
            cfg["no_seeds_us"], cfg["no_seeds_us_laps"] = lap_us(call, a.laps)
        finally:
            _lib.check(L.read_tuning_set(b"splat_seeds", 1))
        out["configs"].append(cfg)
        r._workspaces.clear()
        del idx, dep
        torch.cuda.empty_cache()
    W, H = 1216, 352
    proj = synthetic.make_proj(W, H)
    totals = [camera.total_matrix(proj, v)[0] for v in views]
    idx, dep = r.render(totals[0], W, H)
    bound = r.bind(W, H, 5, (idx, dep), totals)
    us, laps = lap_us(lambda k: bound(k, (k + 1) % POSES), a.laps)
    out["pinhole_cells_us"], out["pinhole_cells_us_laps"], out["pinhole_W"], out["pinhole_H"] = us, laps, W, H
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
