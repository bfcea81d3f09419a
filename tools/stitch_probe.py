"""Scene stitching, measured: the stitched gather against the plain gather, and a stitched frame against a single-scene frame.
One JSON line (kept as profiles/stitch_probe.json).

    python tools/stitch_probe.py [--laps 5] [--reps 200] [--points 3000000] [--frame-points 10000000] [--no-frames]

Kernel part: 1216 x 352, five levels, C = 8.  Four street clouds (synthetic.make_street_cloud, seeds 11..14, --points each) are
rasterised once at pose 8 of the sweep; their pyramids and four random descriptor tables are the inputs of every variant:
  a        read_gather_forward on part 0 (its own index pyramid)
  b1/b2/b4 read_stitch_gather_forward with S = 1, 2, 4, features only
  c2       S = 2 with every output (merged index, depth and part images as well)
The variants alternate inside one process: one untimed lap of all of them, then --laps laps; a lap of a variant is --reps launches
between two HIP events, enqueued while a sleep kernel holds the GPU, so the lap is device time.  Per variant: mean / min / max
microseconds per launch over the laps, and its byte floor sum_l px_l * (8 S + 4 C + 4 C [+ 9 with the merged images]) — 4 + 4 C +
4 C for (a) — at 8 TB/s.  The working set of a variant (tens of MB) stays in the 256 MB Infinity Cache between launches, so these
are cache-resident times for every variant alike; the floors are HBM floors, given for scale.
Frame part: FrameRenderer on one 10 M-point street cloud, FrameRenderer on the concatenation of two (the second placed 160 m down
the street), StitchedFrameRenderer on the two with that placement; 64 poses of the sweep, each camera announced one frame ahead,
host wall clock around render_total + a synchronisation, the second of two laps."""
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
from read_amd.frame import FrameRenderer  # noqa: E402
from read_amd.raster import PointCloudRasterizer  # noqa: E402
from read_amd.stitch import StitchedFrameRenderer  # noqa: E402
from read_amd.texture import _ACT  # noqa: E402

W, H, LEVELS, CH, POSES = 1216, 352, 5, 8, 64
HBM_BYTES_PER_US = 8e6          # 8 TB/s


def byte_floor(S, merged, plain=False):
    px = sum((W >> l) * (H >> l) for l in range(LEVELS))
    per = (4 if plain else 8 * S) + 4 * CH + 4 * CH + (9 if merged else 0)
    return px * per


def bound_plain(rows, idx, feat):
    L, levels = _lib.lib(), len(idx)
    counts = (C.c_int64 * levels)(*[int(i.numel()) for i in idx])
    ip, fp = _lib.ptr_array([i.data_ptr() for i in idx]), _lib.ptr_array([f.data_ptr() for f in feat])
    args = (rows.data_ptr(), rows.shape[0], rows.shape[1], levels, ip, counts, fp, 0)
    return lambda: _lib.check(L.read_gather_forward(*args, _lib.stream_ptr()), "read_gather_forward")


def bound_stitch(tables, pyramids, feat, merged=None):
    """Every ctypes argument built once; merged: None or (idx, depth, part) output pyramids."""
    L, S, levels = _lib.lib(), len(tables), len(feat)
    keep, parts, base = [], (_lib.StitchPart * S)(), 0
    for s in range(S):
        ip = _lib.ptr_array([t.data_ptr() for t in pyramids[s][0]])
        dp = _lib.ptr_array([t.data_ptr() for t in pyramids[s][1]])
        keep += [ip, dp]
        parts[s].idx_levels, parts[s].depth_levels = ip, dp
        parts[s].rows_nc, parts[s].n, parts[s].id_base, parts[s].activation = tables[s].data_ptr(), tables[s].shape[0], base, _ACT["none"]
        base += tables[s].shape[0]
    counts = (C.c_int64 * levels)(*[int(f.numel()) // CH for f in feat])
    arr = lambda ts: _lib.ptr_array([t.data_ptr() for t in ts])
    outs = [arr(m) for m in merged] if merged else [None, None, None]
    fp = arr(feat)

    def call():
        _lib.check(L.read_stitch_gather_forward(parts, S, CH, levels, counts, outs[0], outs[1], outs[2], fp, _lib.stream_ptr()),
                   "read_stitch_gather_forward")
    call.keep = (keep, parts, counts, outs, fp)
    return call


def lap_us(call, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda._sleep(int(2e8))
    e0.record()
    for _ in range(reps):
        call()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / reps


def kernel_part(out, a):
    proj = synthetic.make_proj(W, H)
    M = camera.total_matrix(proj, synthetic.sweep_pose(8))[0]
    pyramids, tables = [], []
    for s in range(4):
        r = PointCloudRasterizer(synthetic.make_street_cloud(a.points, 11 + s))
        idx, dep = r.render(M, W, H, LEVELS)
        pyramids.append(([t.clone() for t in idx], [t.clone() for t in dep]))
        tables.append(torch.rand((a.points, CH), device="cuda", generator=torch.Generator("cuda").manual_seed(s)))
        del r
    torch.cuda.empty_cache()
    sizes = camera.level_sizes(W, H, LEVELS)
    img = lambda dtype, tail=(): [torch.empty((1, h, w) + tail, dtype=dtype, device="cuda") for (w, h) in sizes]
    feat = img(torch.float32, (CH,))
    merged = (img(torch.int32), img(torch.float32), img(torch.uint8))
    variants = {
        "a": (bound_plain(tables[0], pyramids[0][0], feat), byte_floor(1, False, plain=True)),
        "b1": (bound_stitch(tables[:1], pyramids[:1], feat), byte_floor(1, False)),
        "b2": (bound_stitch(tables[:2], pyramids[:2], feat), byte_floor(2, False)),
        "b4": (bound_stitch(tables, pyramids, feat), byte_floor(4, False)),
        "c2": (bound_stitch(tables[:2], pyramids[:2], feat, merged), byte_floor(2, True)),
    }
    # S = 1 computes what the plain gather computes
    variants["a"][0]()
    want = [f.clone() for f in feat]
    variants["b1"][0]()
    torch.cuda.synchronize()
    out["b1_equals_a"] = all(torch.equal(x, y) for x, y in zip(want, feat))
    covered = [float(((p[0][0] != 0) | (p[1][0].view(torch.int32) != 0)).float().mean()) for p in pyramids]
    out["covered_level0"] = [round(c, 3) for c in covered]
    laps = {k: [] for k in variants}
    for lap in range(a.laps + 1):                                # lap 0 warms every variant up and is not kept
        for k, (call, _) in variants.items():
            t = lap_us(call, a.reps)
            if lap:
                laps[k].append(t)
    out["variants"] = {}
    for k, (_, floor) in variants.items():
        v = laps[k]
        out["variants"][k] = {"us_mean": round(float(np.mean(v)), 3), "us_min": round(min(v), 3), "us_max": round(max(v), 3),
                              "us_laps": [round(x, 3) for x in v], "floor_bytes": floor,
                              "floor_us_at_8TBps": round(floor / HBM_BYTES_PER_US, 3)}
    va, vb = out["variants"]["a"], out["variants"]["b1"]
    out["a_spread_us"] = round(va["us_max"] - va["us_min"], 3)
    out["b1_minus_a_us"] = round(vb["us_mean"] - va["us_mean"], 3)
    out["b1_within_a_spread"] = bool(abs(vb["us_mean"] - va["us_mean"]) <= va["us_max"] - va["us_min"])


def frame_ms(fr, totals):
    times = []
    for rep in range(2):                                          # lap 0 warms up
        for k in range(POSES):
            t0 = time.perf_counter()
            fr.render_total(totals[k], next_total=totals[(k + 1) % POSES])
            torch.cuda.synchronize()
            if rep:
                times.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.mean(times)), 4)


def frame_part(out, a):
    from read_amd.unet import weight_spec
    n = a.frame_points
    proj = synthetic.make_proj(W, H)
    totals = [camera.total_matrix(proj, synthetic.sweep_pose(k))[0] for k in range(POSES)]
    state = synthetic.make_unet_state(weight_spec())
    clouds = [synthetic.make_street_cloud(n, 21), synthetic.make_street_cloud(n, 22)]
    desc = [synthetic.make_descriptors(n, seed=31), synthetic.make_descriptors(n, seed=32)]
    P = np.eye(4, dtype=np.float32)
    P[2, 3] = -160.0                                              # the second segment continues the street
    moved = clouds[1].copy()
    moved[:, 2] += np.float32(-160.0)
    out["frame_points_per_part"] = n
    for name, make in (
            ("frame_ms_single_scene", lambda: FrameRenderer(clouds[0], desc[0], state, W, H)),
            ("frame_ms_concatenated", lambda: FrameRenderer(np.concatenate([clouds[0], moved]), np.concatenate(desc, 1), state, W, H)),
            ("frame_ms_stitched", lambda: StitchedFrameRenderer([{'xyz': clouds[0], 'texture_cn': desc[0]},
                                                                 {'xyz': clouds[1], 'texture_cn': desc[1], 'pose': P}], state, W, H))):
        fr = make()
        out[name] = frame_ms(fr, totals)
        del fr
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--laps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--points", type=int, default=3_000_000)
    ap.add_argument("--frame-points", type=int, default=10_000_000)
    ap.add_argument("--no-frames", action="store_true")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    out = {"tool": "stitch_probe", "device": torch.cuda.get_device_name(0), "W": W, "H": H, "levels": LEVELS, "C": CH,
           "points_per_part": a.points, "laps": a.laps, "reps": a.reps}
    kernel_part(out, a)
    if not a.no_frames:
        frame_part(out, a)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
