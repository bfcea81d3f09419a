"""Host vs device build of the cell-ordered cloud (read_splat_cells_build_host vs read_splat_cells_build): one JSON line.

    python tools/cells_build_probe.py [--reps 10]

Clouds: 30 M points of synthetic.make_cloud and 10 M of synthetic.make_street_cloud.  For each:
  host_ms            median of 3 host builds: the builder's own thread count (min(32, hardware threads)) on 16 CPUs (the process
                     is pinned to 16 of the CPUs it may use, as a GPU job's share of a box; --host-cpus changes that)
  device_ms          median of >= 10 warm device builds, HIP events around the C call on the stream (blob and scratch allocated
                     once, outside the timed region)
  device_wall_ms     the same calls on the host clock (launches + the call's closing read of the non-finite index and sync)
  bytes_equal        the device blob equals the host blob byte for byte (every byte a build defines: all but the chunk lists)
  equal_up_to_zero_sign  ... with the min / max fields (header box, chunk boxes) compared by value
Needs the GPU; the host builds need ~2 GB of host memory at 30 M points.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from read_amd import _lib, synthetic  # noqa: E402
from read_amd.raster import build_cells  # noqa: E402


def compare(dev, host, n):
    """(bytes equal, equal up to the sign of zero in the min / max fields), both over the bytes a build defines."""
    nc = (n + 1023) // 1024
    aabb = 256 + nc * 1024 * 16
    lists = aabb + nc * 32
    minmax = np.zeros(len(host), bool)
    minmax[16:40] = True
    box = np.zeros((nc, 32), bool)
    box[:, :24] = True
    minmax[aabb:lists] = box.reshape(-1)
    defined = np.ones(len(host), bool)
    defined[lists:len(host) - ((nc + 255) // 256) * 256] = False      # chunk lists: per-frame scratch, not written by a build
    same = (dev == host) | ~defined
    if same.all():
        return True, True
    if (~same & ~minmax).any():
        return False, False
    return False, bool(np.array_equal(dev[minmax].view(np.float32), host[minmax].view(np.float32)))


def probe(name, xyz, reps):
    n = xyz.shape[0]
    L = _lib.lib()
    host_ms = []
    for _ in range(3):
        t0 = time.perf_counter()
        host = build_cells(xyz)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    t = torch.from_numpy(xyz).cuda()
    nbytes, sbytes = L.read_splat_cells_bytes(n), L.read_splat_cells_build_scratch_bytes(n)
    blob = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    scratch = torch.empty(sbytes, dtype=torch.uint8, device="cuda")
    st = _lib.stream_ptr()

    def build():
        _lib.check(L.read_splat_cells_build(t.data_ptr(), n, blob.data_ptr(), nbytes, scratch.data_ptr(), sbytes, st),
                   "read_splat_cells_build")
    for _ in range(3):
        build()
    torch.cuda.synchronize()
    ev_ms, wall_ms = [], []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        w0 = time.perf_counter()
        build()
        w1 = time.perf_counter()
        e1.record()
        torch.cuda.synchronize()
        ev_ms.append(e0.elapsed_time(e1))
        wall_ms.append((w1 - w0) * 1e3)
    exact, up_to_zero_sign = compare(blob.cpu().numpy(), host, n)
    return {
        "cloud": name, "n": n, "blob_bytes": nbytes, "scratch_bytes": sbytes,
        "host_ms": round(float(np.median(host_ms)), 2), "host_ms_all": [round(x, 2) for x in host_ms],
        "device_ms": round(float(np.median(ev_ms)), 3), "device_ms_min": round(float(np.min(ev_ms)), 3),
        "device_ms_max": round(float(np.max(ev_ms)), 3), "device_wall_ms": round(float(np.median(wall_ms)), 3),
        "reps": reps, "speedup_host_over_device": round(float(np.median(host_ms) / np.median(ev_ms)), 1),
        "bytes_equal": exact, "equal_up_to_zero_sign": up_to_zero_sign,
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-cpus", type=int, default=16)
    a = ap.parse_args()
    reps = max(10, a.reps)
    cpus = sorted(os.sched_getaffinity(0))[:max(1, a.host_cpus)]
    os.sched_setaffinity(0, cpus)
    out = {
        "tool": "cells_build_probe", "device": torch.cuda.get_device_name(0),
        "arch": torch.cuda.get_device_properties(0).gcnArchName.split(":")[0],
        "host_threads": min(32, max(1, os.cpu_count() or 1)), "host_cpus": len(cpus),
        "results": [probe("make_cloud", synthetic.make_cloud(30_000_000), reps),
                    probe("make_street_cloud", synthetic.make_street_cloud(10_000_000), reps)],
    }
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
