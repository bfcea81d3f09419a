"""Frame flow, measured: what read_flow_frame (csrc/flow.hip) costs beside the frames it connects.  One JSON line.

    python tools/flow_probe.py [--laps 3] [--out profiles/flow_probe.json]

Scene: the setting of tools/annotate_probe.py — 30 M points of synthetic.make_cloud at 1216 x 352, ONE object of 25 k points, its
original hidden, drawn as I = 0 / 16 / 64 instances.  State A is sweep pose 0 with the copies posed as instances_probe's frame 0, state
B sweep pose 1 with the copies posed as its frame 1.
  raster_us[I]     the rasteriser per frame: HIP events around a lap over the first 64 sweep poses (pre-bound calls, cameras
                   announced) enqueued behind a sleep kernel, mean of --laps laps
  annotate_us[I]   read_annotate_frame on state A's frame (Annotation.refresh), HIP events around 200 calls behind a sleep kernel
  flow_us[I]       read_flow_frame from A to B — the init launch and the pixel pass — with every argument marshalled and every table
                   uploaded once (FrameFlow.refresh), measured the same way in the same run
  floor_us[I]      the bytes the pixel pass must move at 8 TB/s: 24 B per pixel (idx, depth in; flow, depth_next, state out) + 12 B of
                   point per filled pixel + 8 B of B's frame per pixel that lands inside it
  counts[I]        the eight state counts of that call;  unmatched[I]: its counter (0: frame and list belong together)
  object_pixels[I] pixels an instance drew in A.  Inside the slab the copies win next to none; the *_front fields repeat flow_us,
                   annotate_us, counts, unmatched and object_pixels with the I copies moved to 10 m in front of the camera, side by side
                   and overlapping (interleaved point by point: a wave holds many instances), shifted by 0.2 m in B
Nothing is gated on any of these numbers."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from read_amd import camera, flow, synthetic  # noqa: E402
from read_amd.raster import PointCloudRasterizer  # noqa: E402
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from annotate_probe import front_pose  # noqa: E402
from instances_probe import H, N, OBJ_POINTS, POSES, W, instance_pose, lap_device_us, launches_us, object_label  # noqa: E402

COUNTS = (0, 16, 64)
HBM_TBS = 8.0


def measure(r, totals, out, key, suffix, laps):
    """State A = the current poses under totals[0]; the caller then moves to state B.  -> the closure that finishes the pair."""
    idx_a, dep_a = r.render(totals[0], W, H, 1)
    sa = r.frame_state(totals[0], W, H, idx_a[0], dep_a[0])
    ann = r.annotate(totals[0], W, H, idx_a[0], dep_a[0])
    out["annotate_us" + suffix][key] = launches_us(ann.refresh, laps)

    def finish():
        idx_b, dep_b = r.render(totals[1], W, H, 1)
        sb = r.frame_state(totals[1], W, H, idx_b[0], dep_b[0])
        f = r.flow(sa, sb)
        counts = f.counts.cpu().numpy()
        out["unmatched" + suffix][key] = int(f.unmatched.item())
        out["counts" + suffix][key] = [int(c) for c in counts]
        out["object_pixels" + suffix][key] = int(f.stats[:, 0].sum().item()) if f.stats.numel() else 0
        out["flow_us" + suffix][key] = launches_us(f.refresh, laps)
        filled = W * H - int(counts[flow.EMPTY])
        landed = int(counts[flow.VISIBLE] + counts[flow.OCCLUDED])
        out["floor_us" + suffix][key] = round((24 * W * H + 12 * filled + 8 * landed) / (HBM_TBS * 1e12) * 1e6, 2)
    return finish


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
    fields = ("annotate_us", "flow_us", "floor_us", "counts", "unmatched", "object_pixels")
    out = {"tool": "flow_probe", "device": torch.cuda.get_device_name(0), "W": W, "H": H, "n": N, "poses": POSES,
           "object_points": OBJ_POINTS, "laps": a.laps, "raster_us": {}}
    out.update({f + s: {} for f in fields for s in ("", "_front")})
    r = PointCloudRasterizer(xyz, labels=labels)
    r.set_object_visible(1, False)
    idx, dep = r.render(totals[0], W, H)
    call = r.bind(W, H, 5, (idx, dep), totals)
    handles = []
    for count in COUNTS:
        while len(handles) < count:
            handles.append(r.add_instance(1, instance_pose(0, len(handles), cent)))
        key = str(count)
        for i, h in enumerate(handles):
            r.set_instance_pose(h, instance_pose(0, i, cent))
        out["raster_us"][key] = lap_device_us(lambda k: call(k, (k + 1) % POSES), a.laps)[0]
        finish = measure(r, totals, out, key, "", a.laps)
        for i, h in enumerate(handles):
            r.set_instance_pose(h, instance_pose(1, i, cent))
        finish()
        if count:
            for i, h in enumerate(handles):
                r.set_instance_pose(h, front_pose(i, count, cent))
            finish = measure(r, totals, out, key, "_front", a.laps)
            for i, h in enumerate(handles):
                P = front_pose(i, count, cent)
                P[0, 3] += 0.2
                r.set_instance_pose(h, P)
            finish()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
