"""Golden digests of the rasteriser pin: the reference's own DepthProject source compiled for the CPU and run serially
(oracle/_ref, built by oracle/build_ref.sh where the reference checkout is present) on seeded clouds and camera poses.

    python tests/golden/make_ref_raster_golden.py

Writes tests/golden/raster_ref_serial.json: the cases (W, H, N, f), the cloud seed, the sweep poses and, per case and pose,
the SHA-256 of the reference's index map (float ids, as pcpr.forward returns them) and of its depth map (float32 bytes),
with the number of covered pixels.  The maps themselves (2 MB) are not stored: the pin is bit-exact, so equal digests are
the same assertion.  tests/test_oracle_raster.py::test_oracle_equals_reference_source_run_serially checks the oracle.
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))

from oracle import ref_c                        # noqa: E402
from read_amd import camera, synthetic          # noqa: E402

CASES = [(256, 256, 100_000, 256.0), (1216, 352, 300_000, 720.0), (40, 24, 3_000, 30.0)]
SEED = 3
POSES = [0, 21]


def sha256(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()


def main():
    if not ref_c.available():
        sys.exit("oracle/_ref/libpcpr_ref.so is not built (python -m oracle.build where the reference checkout is present)")
    cases = []
    for (W, H, N, f) in CASES:
        xyz = synthetic.make_cloud(N, seed=SEED)
        Ms = camera.total_matrix(synthetic.make_proj(W, H, f=f), np.stack([synthetic.sweep_pose(k) for k in POSES]))
        ri, rd = ref_c.pcpr_ref_forward(xyz, Ms, W, H)
        cases.append({"W": W, "H": H, "N": N, "f": f,
                      "maps": [{"index_sha256": sha256(ri[b]), "depth_sha256": sha256(rd[b]), "covered": int((ri[b] > 0).sum())}
                               for b in range(len(POSES))]})
    path = os.path.join(HERE, "raster_ref_serial.json")
    with open(path, "w") as fh:
        json.dump({"seed": SEED, "poses": POSES, "cases": cases}, fh, indent=1)
        fh.write("\n")
    print(path)


if __name__ == "__main__":
    main()
