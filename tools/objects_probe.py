"""Scene editing, measured: what a frame costs when objects of a fitted scene are re-posed every frame.  One JSON line.

    python tools/objects_probe.py [--laps 3] [--raster-only]

Scene: 30 M points of synthetic.make_cloud at 1216 x 352 on the first 64 poses of the sweep, every camera announced one frame ahead;
16 objects of 25 k points each (the points nearest to 16 random centres), every object re-posed every frame (a turn about its
centre and a drift).
  raster_us            rasteriser per frame, HIP events around a lap of 64 pre-bound calls (PointCloudRasterizer.bind); the GPU is
                       held by a sleep kernel while the lap is enqueued, so the lap is device time; mean of --laps laps
                       (no_labels: the unlabelled cloud; objects: the labelled cloud, 16 set_object_pose calls per frame)
  frame_ms             whole frame one at a time (FrameRenderer.render_total, frames_in_flight 1, host wall clock around the call
                       and a synchronisation), mean over a lap, same two ways (objects: the 16 poses set before each frame)
  today_discard_ms     the route without this feature for HIDING the objects: Scene.set_point_discard + OGL.infer (the dict path,
                       five GL-twin passes), per frame, wall clock
  today_set_vertices_ms  the route for MOVING them: the moved cloud through Scene.set_vertices + OGL.infer (new rasteriser: upload,
                       cell build, no warm start), per frame, wall clock
--raster-only: only the objects lap (for a rocprofv3 --kernel-trace --stats run that lists range_splat_kernel<PinholeCam>).
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from read_amd import camera, synthetic  # noqa: E402
from read_amd.frame import FrameRenderer  # noqa: E402
from read_amd.raster import PointCloudRasterizer  # noqa: E402

W, H, N, POSES, OBJECTS, OBJ_POINTS = 1216, 352, 30_000_000, 64, 16, 25_000


def object_labels(xyz, seed=7):
    rng = np.random.default_rng(seed)
    labels = np.zeros(xyz.shape[0], np.int32)
    for k in range(1, OBJECTS + 1):
        c = xyz[rng.integers(xyz.shape[0])]
        d = ((xyz - c) ** 2).sum(1)
        d[labels != 0] = np.inf
        labels[np.argpartition(d, OBJ_POINTS)[:OBJ_POINTS]] = k
    return labels


def object_poses(f, cents):
    out = {}
    for k, c in cents.items():
        a = 0.05 * f * (1 + k % 3)
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        P = np.eye(4)
        P[:3, :3] = R
        P[:3, 3] = c - R @ c + np.array([0.02 * f, 0.0, -0.01 * f * k])
        out[k] = P.astype(np.float32)
    return out


def lap_device_us(call, poses_of=None, setter=None, laps=3):
    """Mean device time per frame of a lap; the whole lap is enqueued behind a sleep kernel."""
    for k in range(POSES):                                      # one untimed lap: lists, seeds and marks settled
        if setter:
            for j, P in poses_of(k).items():
                setter(j, P)
        call(k, (k + 1) % POSES)
    torch.cuda.synchronize()
    per = []
    for _ in range(laps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(int(1.5e9))
        e0.record()
        for k in range(POSES):
            if setter:
                for j, P in poses_of(k).items():
                    setter(j, P)
            call(k, (k + 1) % POSES)
        e1.record()
        torch.cuda.synchronize()
        per.append(1e3 * e0.elapsed_time(e1) / POSES)
    return round(float(np.mean(per)), 2), [round(x, 2) for x in per]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--laps", type=int, default=3)
    ap.add_argument("--raster-only", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    xyz = synthetic.make_cloud(N)
    labels = object_labels(xyz)
    cents = {k: xyz[labels == k].astype(np.float64).mean(0) for k in range(1, OBJECTS + 1)}
    pose_table = [object_poses(f, cents) for f in range(POSES)]
    proj = synthetic.make_proj(W, H)
    totals = [camera.total_matrix(proj, synthetic.sweep_pose(k))[0] for k in range(POSES)]
    out = {"tool": "objects_probe", "device": torch.cuda.get_device_name(0), "W": W, "H": H, "n": N, "poses": POSES,
           "objects": OBJECTS, "object_points": OBJ_POINTS, "laps": a.laps}

    r_obj = PointCloudRasterizer(xyz, labels=labels)
    idx, dep = r_obj.render(totals[0], W, H)
    call = r_obj.bind(W, H, 5, (idx, dep), totals)
    out["raster_us_objects"], out["raster_us_objects_laps"] = lap_device_us(call, lambda k: pose_table[k], r_obj.set_object_pose,
                                                                            a.laps)
    if a.raster_only:
        print(json.dumps(out), flush=True)
        return
    del r_obj, call, idx, dep
    r = PointCloudRasterizer(xyz)
    idx, dep = r.render(totals[0], W, H)
    call = r.bind(W, H, 5, (idx, dep), totals)
    out["raster_us_no_labels"], out["raster_us_no_labels_laps"] = lap_device_us(call, laps=a.laps)
    del r, call, idx, dep
    torch.cuda.empty_cache()

    # whole frame, one at a time
    from read_amd.unet import weight_spec
    desc = synthetic.make_descriptors(N)
    state = synthetic.make_unet_state(weight_spec())
    for name, lab in (("no_labels", None), ("objects", labels)):
        fr = FrameRenderer(xyz, desc, state, W, H, proj_matrix=proj, object_labels=lab)
        times = []
        for rep in range(2):                                    # lap 0 warms up
            for k in range(POSES):
                t0 = time.perf_counter()
                if lab is not None:
                    for j, P in pose_table[k].items():
                        fr.set_object_pose(j, P)
                fr.render_total(totals[k], next_total=totals[(k + 1) % POSES])
                torch.cuda.synchronize()
                if rep:
                    times.append((time.perf_counter() - t0) * 1e3)
        out[f"frame_ms_{name}"] = round(float(np.mean(times)), 4)
        del fr
        torch.cuda.empty_cache()

    # today's routes, through OGL as a viewer would call it
    from read_amd.net_texture import NetAndTexture
    from read_amd.ogl import OGL
    from read_amd.render import Scene
    from read_amd.texture import PointTexture
    from read_amd.unet import UNet
    net = UNet()
    net.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in state.items()})
    tex = PointTexture(8, N, init_method='rand')
    model = NetAndTexture(net, {0: tex})
    model.load_textures(0)
    fmt = "uv_1d_p1, uv_1d_p1_ds1, uv_1d_p1_ds2, uv_1d_p1_ds3, uv_1d_p1_ds4"
    scene = Scene(xyz)
    scene.set_proj_matrix(proj)
    ogl = OGL.from_model(scene, model, fmt, (W, H))
    hide = labels != 0
    frames = 8

    def timed(prepare):
        ts = []
        for k in range(frames + 2):
            scene.set_camera_view(synthetic.sweep_pose(k))
            t0 = time.perf_counter()
            prepare(k)
            ogl.infer()
            torch.cuda.synchronize()
            if k >= 2:
                ts.append((time.perf_counter() - t0) * 1e3)
        return round(float(np.mean(ts)), 3)

    out["today_discard_ms"] = timed(lambda k: scene.set_point_discard(hide))
    out["today_discard_path"] = ogl.last_path
    scene.set_point_discard(None)
    moved = xyz.copy()
    obj_idx = {j: np.flatnonzero(labels == j) for j in range(1, OBJECTS + 1)}

    def move(k):
        for j, P in pose_table[k].items():
            p = xyz[obj_idx[j]]
            moved[obj_idx[j]] = (p @ P[:3, :3].T + P[:3, 3]).astype(np.float32)
        scene.set_vertices(moved)
    out["today_set_vertices_ms"] = timed(move)
    out["today_set_vertices_path"] = ogl.last_path
    scene.set_vertices(xyz)
    scene.set_object_labels(labels)

    def edit(k):
        for j, P in pose_table[k].items():
            scene.set_object_pose(j, P)
    out["ogl_edit_ms"] = timed(edit)
    out["ogl_edit_path"] = ogl.last_path
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
