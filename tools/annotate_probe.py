"""Frame annotations, measured: what read_annotate_frame (csrc/annotate.hip) costs beside the frame it describes.  One JSON line.

    python tools/annotate_probe.py [--laps 3] [--out profiles/annotate_probe.json]

Scene: the setting of tools/instances_probe.py — 30 M points of synthetic.make_cloud at 1216 x 352, ONE object of 25 k points (the
points nearest to a random centre), its original hidden, drawn as I = 0 / 16 / 64 instances posed as that probe's frame 0.
  raster_us[I]     the rasteriser per frame: HIP events around a lap over the first 64 sweep poses (pre-bound calls, cameras
                   announced) enqueued behind a sleep kernel, mean of --laps laps
  annotate_us[I]   read_annotate_frame on pose 0's frame — the init launch, the pixel pass and ceil(I / 32) extents launches — with
                   every argument marshalled and every table uploaded once (Annotation.refresh): HIP events around 200 calls behind
                   a sleep kernel, mean of --laps laps
  floor_us[I]      the bytes the two passes must move at 8 TB/s: 16 B per pixel (idx, depth in; obj, inst out) + 12 B per drawn point
  unmatched[I]     the counter of that frame (0: frame and list belong together)
  object_pixels[I] pixels an instance won in that frame.  Inside the slab (about 70 points per pixel) the copies win next to none, so
                   the pixel pass above walks no instance list; the *_front fields repeat annotate_us, unmatched and object_pixels
                   with the I copies moved to 10 m in front of pose 0's camera, side by side and overlapping, where a pixel of the
                   object walks up to I matrices
Nothing is gated on any of these numbers."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from read_amd import camera, synthetic  # noqa: E402
from read_amd.raster import PointCloudRasterizer  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from instances_probe import H, N, OBJ_POINTS, POSES, W, instance_pose, lap_device_us, launches_us, object_label  # noqa: E402

COUNTS = (0, 16, 64)
HBM_TBS = 8.0


def front_pose(i, count, c):
    P = np.eye(4)
    P[:3, 3] = np.array([-6.0 + 12.0 * (i + 0.5) / count, 0.5 * (i % 3), -10.0 - 0.05 * i]) - c
    return P.astype(np.float32)


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
    out = {"tool": "annotate_probe", "device": torch.cuda.get_device_name(0), "W": W, "H": H, "n": N, "poses": POSES,
           "object_points": OBJ_POINTS, "laps": a.laps, "raster_us": {}, "annotate_us": {}, "floor_us": {}, "extents_launches": {},
           "unmatched": {}, "object_pixels": {}, "annotate_us_front": {}, "unmatched_front": {}, "object_pixels_front": {}}
    r = PointCloudRasterizer(xyz, labels=labels)
    r.set_object_visible(1, False)
    idx, dep = r.render(totals[0], W, H)
    call = r.bind(W, H, 5, (idx, dep), totals)
    handles = []
    for count in COUNTS:
        while len(handles) < count:
            handles.append(r.add_instance(1, instance_pose(0, len(handles), cent)))
        out["raster_us"][str(count)] = lap_device_us(lambda k: call(k, (k + 1) % POSES), a.laps)[0]
        call(0)                                                  # pose 0's frame stays in (idx, dep)
        ann = r.annotate(totals[0], W, H, idx[0], dep[0])
        out["unmatched"][str(count)] = int(ann.unmatched.item())
        out["object_pixels"][str(count)] = int((ann.objects >= 1).sum().item())
        out["annotate_us"][str(count)] = launches_us(ann.refresh, a.laps)
        out["extents_launches"][str(count)] = (count + 31) // 32
        if count:
            for i, h in enumerate(handles):
                r.set_instance_pose(h, front_pose(i, count, cent))
            call(0)
            ann = r.annotate(totals[0], W, H, idx[0], dep[0])
            out["unmatched_front"][str(count)] = int(ann.unmatched.item())
            out["object_pixels_front"][str(count)] = int((ann.objects >= 1).sum().item())
            out["annotate_us_front"][str(count)] = launches_us(ann.refresh, a.laps)
            for i, h in enumerate(handles):
                r.set_instance_pose(h, instance_pose(0, i, cent))
        out["floor_us"][str(count)] = round((16 * W * H + 12 * count * OBJ_POINTS) / (HBM_TBS * 1e12) * 1e6, 2)
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
