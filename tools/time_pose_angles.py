#!/usr/bin/env python3
"""Times the angle-space pose kernels (csrc/pose_angles.hip) and ``AnglePoseCamera.project`` at the reference's evaluation sizes:
64 sequences x 50 frames (one test batch) and 50 x 16 x 50 (50 sampled behaviours of 16 sequences).

    python tools/time_pose_angles.py [--launches 200] [--repeats 15] [--commit HASH] [--out FILE]

What is measured: HIP events around ``--launches`` back-to-back calls of one function on the current stream, after a warm-up of
the same shape; the time per call of that window; ``--repeats`` windows, of which the median, the minimum and the maximum are
reported.  A call includes its host side (argument checks, the output allocation, the ctypes launch): at these sizes the
kernels are short enough that the host's launch rate, not the device, can be what a window measures, so ``host_us`` gives
the same loop's wall-clock time per call without waiting for the device.  Prints one JSON line; ``--out`` appends it to a file.
There is no earlier path to compare with: the parent has none and the reference's host loops are not part of this repository.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from behavior_driven_video_synthesis_amd import pose_angles as A  # noqa: E402
from behavior_driven_video_synthesis_amd.render import AnglePoseCamera  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=200)
ap.add_argument("--repeats", type=int, default=15)
ap.add_argument("--commit", default="", help="the commit the numbers belong to (recorded as given)")
ap.add_argument("--out", default="")
a = ap.parse_args()

# the skeleton and the statistics of the test fixture: the package holds none of its own
z = np.load(os.path.join(ROOT, "tests", "golden", "g12_pose_angles.npz"))
meta = json.loads(bytes(z["__meta__"]).decode())
tree = A.KinematicTree({"parent": z["tree.parent"], "offset": z["tree.offset"], "expmapInd": list(z["tree.expmapInd"]),
                        "posInd": {"ids": z["tree.posInd"]}})
stats = A.AngleStats(z["stats.mean"], z["stats.std"], meta["ignore"])
use = [d for d in range(stats.dim) if d not in set(meta["ignore"])]
ext = np.concatenate([np.eye(3), np.array([[0.0], [0.0], [5200.0]])], axis=1)
cam = AnglePoseCamera(z["stats.mean"], z["stats.std"], use, tree, ext, (1145.0, 512.5, 1143.8, 515.4), (1000, 1002), 256)
r0, t0 = torch.eye(3, dtype=torch.float64, device="cuda"), torch.zeros(3, dtype=torch.float64, device="cuda")   # on the device: no copy per call
horizons = [2, 4, 8, 10]


def timed(fn):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    per_call, host = [], []
    for _ in range(a.repeats):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        h0 = time.perf_counter()
        start.record()
        for _ in range(a.launches):
            fn()
        end.record()
        host.append((time.perf_counter() - h0) / a.launches * 1e6)
        end.synchronize()
        per_call.append(start.elapsed_time(end) / a.launches * 1e3)
    return {"median_us": round(statistics.median(per_call), 2), "min_us": round(min(per_call), 2), "max_us": round(max(per_call), 2),
            "host_us": round(statistics.median(host), 2)}


g = torch.Generator().manual_seed(0)
out = {"commit": a.commit, "device": torch.cuda.get_device_name(0), "launches_per_window": a.launches, "windows": a.repeats,
       "unit": "microseconds per call: HIP events around a window of back-to-back calls; host_us: the loop without the device wait",
       "sizes": {}}
for tag, (b, t) in {"64x50": (64, 50), "800x50": (50 * 16, 50)}.items():
    norm = torch.randn(b, t, stats.n_use, generator=g).cuda()
    gt = torch.randn(b, t, stats.n_use, generator=g).cuda()
    angles = (torch.randn(b, t, stats.dim, generator=g) * 0.5).cuda()
    flat = norm.reshape(b * t, -1)
    out["sizes"][tag] = {
        "convert_to_3d": timed(lambda: A.convert_to_3d(angles, tree)),
        "convert_to_3d_normalised": timed(lambda: A.convert_to_3d(norm, tree, stats=stats)),
        "revert_coordinate_space": timed(lambda: A.revert_coordinate_space(angles, r0, t0)),
        "euler_error": timed(lambda: A.euler_error(norm, gt, stats, horizons)),
        "angle_pose_camera_project": timed(lambda: cam.project(flat)),
    }
line = json.dumps(out)
print(line)
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
