"""The lens cameras, measured: what the rasteriser costs per frame when the whole cloud is read under a distorted pinhole or a
fisheye, beside the panorama camera and the pinhole's plain path in the same run.

    python tools/lens_probe.py [--laps 3] [--n 30000000] [--out profiles/lens_probe.json]

Cloud: the bench cloud, the 30 M-point slab (synthetic.make_cloud), on the first 64 poses of the sweep, 1216 x 352.  Every figure is
device time per frame: HIP events on the launch stream around a whole lap of 64 calls enqueued behind a sleep kernel; one untimed
lap first, then the mean of --laps laps.  Per camera (brown: model 0, a 90-degree forward camera; fisheye: model 1 under a
200-degree field mask; pano: 360 degrees; pinhole_plain: read_splat_forward_cells on a rasteriser built without cells, the plain
pass that also reads the whole cloud):
  steady_us       every frame warm-started from its predecessor's winners
  no_seeds_us     the same lap with read_tuning_set("splat_seeds", 0): what the warm start is worth
  first_us        the first frame on a fresh workspace (no seeds), events around the one call; mean of three workspaces
  covered_pixels  level-0 pixels drawn by pose 0
and floor_us, the byte floor 12 N / 8 TB/s.  No threshold is set on any of these."""
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

POSES, W, H = 64, 1216, 352
LENSES = {"brown": (0, (-0.28, 0.07, 0.0006, -0.0004, -0.008), 0.5, None),
          "fisheye": (1, (-0.03, 0.002, -0.0005, 0.00003), 0.26, float(np.deg2rad(100.0)))}


def lens_proj(fx_share):
    K = np.array([[fx_share * W, 0, W / 2.0], [0, fx_share * W, H / 2.0], [0, 0, 1.0]])
    return camera.get_proj_matrix(K, (W, H), 0.1, 1000.0).astype(np.float32)


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


def measure(r, call, laps, L):
    """-> the figures of one camera; ``call(k)`` renders pose k into preallocated outputs."""
    cfg = {}
    first = []
    for _ in range(3):
        r._workspaces.clear()
        r._workspace(1, W, H)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call(0)
        e1.record()
        torch.cuda.synchronize()
        first.append(1e3 * e0.elapsed_time(e1))
    cfg["first_us"], cfg["first_us_runs"] = round(float(np.mean(first)), 2), [round(x, 2) for x in first]
    cfg["steady_us"], cfg["steady_us_laps"] = lap_us(call, laps)
    _lib.check(L.read_tuning_set(b"splat_seeds", 0))
    try:
        cfg["no_seeds_us"], cfg["no_seeds_us_laps"] = lap_us(call, laps)
    finally:
        _lib.check(L.read_tuning_set(b"splat_seeds", 1))
    return cfg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--laps", type=int, default=3)
    ap.add_argument("--n", type=int, default=30_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lens_probe.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    L = _lib.lib()
    xyz = synthetic.make_cloud(a.n)
    views = [synthetic.sweep_pose(k) for k in range(POSES)]
    out = {"tool": "lens_probe", "device": torch.cuda.get_device_name(0), "n": a.n, "poses": POSES, "laps": a.laps, "W": W, "H": H,
           "floor_us": round(12.0 * a.n / 8e12 * 1e6, 2), "cameras": {}}
    r = PointCloudRasterizer(xyz, cells=False)                   # every camera below reads the whole cloud: no cell blob
    idx, dep = r.render(camera.total_matrix(synthetic.make_proj(W, H), views[0])[0], W, H)
    for name, (model, coeffs, fx_share, limit) in LENSES.items():
        cams = [camera.lens_camera(lens_proj(fx_share), v, model, coeffs, limit) for v in views]
        cfg = measure(r, lambda k: r.render_lens(cams[k], W, H, out=(idx, dep)), a.laps, L)
        r.render_lens(cams[0], W, H, out=(idx, dep))
        cfg.update(model=model, coeffs=list(coeffs), limit=float(cams[0][18]), covered_pixels=int((dep[0] != 0).sum()))
        out["cameras"][name] = cfg
    proj = synthetic.make_proj(W, H)
    panos = [camera.pano_camera(proj, v, 360.0) for v in views]
    cfg = measure(r, lambda k: r.render_pano(panos[k], W, H, out=(idx, dep)), a.laps, L)
    r.render_pano(panos[0], W, H, out=(idx, dep))
    cfg.update(hfov_deg=360.0, covered_pixels=int((dep[0] != 0).sum()))
    out["cameras"]["pano"] = cfg
    totals = [camera.total_matrix(proj, v)[0] for v in views]
    cfg = measure(r, lambda k: r.render(totals[k], W, H, out=(idx, dep)), a.laps, L)
    r.render(totals[0], W, H, out=(idx, dep))
    cfg.update(covered_pixels=int((dep[0] != 0).sum()))
    out["cameras"]["pinhole_plain"] = cfg
    line = json.dumps(out)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
