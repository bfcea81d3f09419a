"""Edited frames, parent against this tree: device and host cost per frame of the laps the two editing probes share.  One JSON line.

    python tools/edited_frames_probe.py [--root TREE] [--laps 5]

TREE (default: this checkout) is the checkout whose ``read_amd`` and ``tools`` are measured — run it once on a checkout of the
parent commit and once on this one, in one session.  The scenes, pose tables and lap method are those of TREE's
tools/objects_probe.py (16 objects of 25 k points, all re-posed every frame through set_object_pose) and
tools/instances_probe.py (one object, its original hidden, I = 16 and 64 instances all re-posed through set_instance_pose),
imported from TREE; the probes' other sections (whole FrameRenderer frames, the OGL routes, the gathers) are not run.
Per lap of 64 pre-bound calls (PointCloudRasterizer.bind) enqueued behind a sleep kernel, after one untimed lap:
  device_us   rasteriser per frame, HIP events around the lap
  host_ms     host time to enqueue one frame (the setter calls, the matrices, the struct, the foreign call): wall clock around
              the enqueue loop — what instances_probe.py reports as host_ms_per_frame, here per lap
"""
import json
import os
import sys
import time

ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1] if "--root" in sys.argv
                       else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LAPS = int(sys.argv[sys.argv.index("--laps") + 1]) if "--laps" in sys.argv else 5
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import instances_probe as ip  # noqa: E402
import objects_probe as op  # noqa: E402
import read_amd  # noqa: E402
from read_amd import camera, synthetic  # noqa: E402
from read_amd.raster import PointCloudRasterizer  # noqa: E402

assert os.path.abspath(read_amd.__file__).startswith(ROOT + os.sep), read_amd.__file__
W, H, N, POSES = op.W, op.H, op.N, op.POSES


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def laps(frame, n):
    t0 = time.perf_counter()
    for k in range(POSES):
        frame(k)
    warm_ms = (time.perf_counter() - t0) * 1e3
    torch.cuda.synchronize()
    cycles = int(max(500.0, 1.5 * warm_ms) * ip.sleep_cycles_per_ms())
    dev, host = [], []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(cycles)
        e0.record()
        t0 = time.perf_counter()
        for k in range(POSES):
            frame(k)
        host.append((time.perf_counter() - t0) * 1e3 / POSES)
        e1.record()
        torch.cuda.synchronize()
        dev.append(1e3 * e0.elapsed_time(e1) / POSES)
    return {"device_us": [round(x, 2) for x in dev], "device_us_mean": round(float(np.mean(dev)), 2),
            "host_ms": [round(x, 4) for x in host], "host_ms_mean": round(float(np.mean(host)), 4)}


def main():
    torch.cuda.set_device(0)
    out = {"tool": "edited_frames_probe", "root": ROOT, "laps": LAPS, "device": torch.cuda.get_device_name(0)}
    xyz = synthetic.make_cloud(N)
    proj = synthetic.make_proj(W, H)
    totals = [camera.total_matrix(proj, synthetic.sweep_pose(k))[0] for k in range(POSES)]
    note("cloud made")

    labels = op.object_labels(xyz)
    cents = {k: xyz[labels == k].astype(np.float64).mean(0) for k in range(1, op.OBJECTS + 1)}
    table = [op.object_poses(f, cents) for f in range(POSES)]
    r = PointCloudRasterizer(xyz, labels=labels)
    idx, dep = r.render(totals[0], W, H)
    call = r.bind(W, H, 5, (idx, dep), totals)

    def frame(k):
        for j, P in table[k].items():
            r.set_object_pose(j, P)
        call(k, (k + 1) % POSES)
    out["objects_16"] = laps(frame, LAPS)
    note("objects_16", out["objects_16"])
    del r, call, idx, dep, labels
    torch.cuda.empty_cache()

    labels = ip.object_label(xyz)
    cent = xyz[labels == 1].astype(np.float64).mean(0)
    r = PointCloudRasterizer(xyz, labels=labels)
    r.set_object_visible(1, False)
    idx, dep = r.render(totals[0], W, H)
    call = r.bind(W, H, 5, (idx, dep), totals)
    handles = []
    for count in (16, 64):
        while len(handles) < count:
            handles.append(r.add_instance(1))
        tab = [[ip.instance_pose(f, i, cent) for i in range(count)] for f in range(POSES)]

        def frame(k):
            for h, P in zip(handles, tab[k]):
                r.set_instance_pose(h, P)
            call(k, (k + 1) % POSES)
        out[f"instances_{count}"] = laps(frame, LAPS)
        note(f"instances_{count}", out[f"instances_{count}"])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
