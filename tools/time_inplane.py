#!/usr/bin/env python3
"""Time the part-normalised appearance input (csrc/inplane.hip) and record its measured accuracy:

  * the two launches alone at N = 16, 256 x 256 -> 64 x 64, P = 10 (Market parts): vunet_inplane_transforms, vunet_inplane_warp,
    and ``part_crops`` (both, with the three output allocations),
  * one Market-size training step (128 x 128, batch 2, 30-channel 64 x 64 appearance input) replayed from its hipGraph with the
    crops cut INSIDE the step (batch carries ``inplane_keypoints``) against the same step fed a ready ``pose_img_inplane``,
  * the maxima of checks A to C of tests/test_hip_inplane.py over its cases, against the float64 restatement (tests/inplane_ref.py).

Device events around windows of many calls after a warm-up; the routes of a pair alternate in the same process, ``--rounds``
windows each, and the median and the spread (min .. max) of the windows are printed.  Needs the GPU; there is no fallback.

    python tools/time_inplane.py --out profiles/inplane_time.txt
"""
import argparse
import copy
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls     # us per call


def compare(named, calls, rounds, warm=20):
    for _, fn in named:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n, _ in named}
    for _ in range(rounds):
        for n, fn in named:                    # alternating
            times[n].append(window(fn, calls))
    return {n: (statistics.median(v), min(v), max(v)) for n, v in times.items()}


def accuracy(lines):
    import inplane_ref as R
    import test_hip_inplane as T
    from behavior_driven_video_synthesis_amd import inplane
    worst = {"A source points [px] (bound 1e-9)": 0.0, "A corner round trip [px] (bound 1e-4)": 0.0,
             "B warp on the oracle's Minv (bound 2e-6)": 0.0, "C part_crops end to end (bound 2e-4)": 0.0}
    keys = list(worst)
    for model, s_out, big in T.CASES:
        img, kps, (minv_r, src_r, valid_r), crops = T._case(model, s_out, big)
        parts = T.MODELS[model]
        minv, src, valid = inplane.part_transforms(T._dev(kps), parts, s_out, img.shape[2])
        minv, src = minv.cpu().numpy(), src.cpu().numpy()
        assert np.array_equal(valid.cpu().numpy(), valid_r)
        rt = max(float(np.abs(R.apply_h(minv[i, q], R.dst_points(kind, s_out)) - src[i, q]).max())
                 for i in range(kps.shape[0]) for q, (kind, _) in enumerate(parts))
        b = inplane.warp_parts(T._dev(img), T._dev(minv_r), T._dev(valid_r), s_out).cpu().numpy().astype(np.float64)
        c = inplane.part_crops(T._dev(img), T._dev(kps), parts, s_out).cpu().numpy().astype(np.float64)
        for k, v in zip(keys, (float(np.abs(src - src_r).max()), rt, float(np.abs(b - crops).max()), float(np.abs(c - crops).max()))):
            worst[k] = max(worst[k], v)
    lines.append(f"# measured maxima over the {len(T.CASES)} cases of tests/test_hip_inplane.py (valid flags equal in all of them)")
    for k, v in worst.items():
        lines.append(f"{k:<46} {v:.3e}")
    print("\n".join(lines[-5:]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--no-accuracy", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_inplane needs an MI355X")
    from behavior_driven_video_synthesis_amd import inplane
    lines = [f"# tools/time_inplane.py: {a.calls} calls per window, {a.rounds} windows per route, alternating; us per call: median "
             f"(min .. max); {torch.cuda.get_device_name(0)}"]

    def row(title, res):
        for n, (med, lo, hi) in res.items():
            lines.append(f"{title:<40} {n:<34} {med:9.1f} us  ({lo:.1f} .. {hi:.1f})")
        print("\n".join(lines[-len(res):]), flush=True)

    # ---- the two launches alone: N = 16, 256^2 -> 64^2, P = 10
    g = torch.Generator().manual_seed(0)
    img = (torch.rand(16, 3, 256, 256, generator=g) * 2 - 1).cuda()
    kps = (torch.rand(16, 18, 2, generator=g) * 250 + 3).cuda()
    parts = inplane.MARKET_PARTS
    minv, _, valid = inplane.part_transforms(kps, parts, 64, 256)
    row("N = 16, 256^2 -> 64^2, P = 10", compare([("vunet_inplane_transforms", lambda: inplane.part_transforms(kps, parts, 64, 256)),
                                                   ("vunet_inplane_warp", lambda: inplane.warp_parts(img, minv, valid, 64)),
                                                   ("part_crops (both)", lambda: inplane.part_crops(img, kps, parts, 64))],
                                                  a.calls, a.rounds))

    # ---- the Market-size step from its hipGraph: crops inside against ready crops
    if not a.no_step:
        from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import DEFAULT_CONFIG, ShapePoseNet, synthetic_batch
        cfg = copy.deepcopy(DEFAULT_CONFIG)
        cfg["data"].update(dataset="Market", spatial_size=128, box_factor=1, bottleneck_factor=1, inplane_normalize=True)
        cfg["training"].update(batch_size=2, train_regressor=False)
        tr = ShapePoseNet(cfg, device="cuda:0", n_channels_x=30, total_steps=150000, vgg_synthetic=True, hip_graph=True)
        base = synthetic_batch(2, 128, "cuda:0", seed=42)
        k2 = (torch.rand(2, 18, 2, generator=g) * 120 + 4).cuda()
        inside = dict(base, inplane_keypoints=k2)
        ready = dict(base, pose_img_inplane=inplane.part_crops(base["pose_img"], k2, parts, 64, 128))
        for _ in range(8):                      # the init batches, the eager device-schedule steps and both captures
            tr.train_fn(inside)
            tr.train_fn(ready)
        torch.cuda.synchronize()
        assert len(tr._graphs) == 2, len(tr._graphs)
        row("Market 128^2 bs 2 step (hipGraph)", compare([("crops inside the step", lambda: tr.train_fn(inside)),
                                                          ("ready pose_img_inplane", lambda: tr.train_fn(ready))],
                                                         max(a.calls // 4, 10), a.rounds, warm=5))
    if not a.no_accuracy:
        accuracy(lines)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
