#!/usr/bin/env python3
"""Time the random appearance augmentation (csrc/appearance_aug.hip) at the trainers' sizes, N = 16 frames:

  * the launch in the DeepFashion form (256 x 256 frames, RandomAffine's draws, fill white, the window is the frame) and in the
    Market form (128 x 128 frames, reflect pad 64, a random rotation, the centre 128 x 128 of the padded image), fp32 out,
  * the same batches through Pillow on ONE host thread (``Image.transform(AFFINE, BILINEAR)`` per frame, for Market after
    ``np.pad(mode="reflect")`` and followed by the crop; then the ToTensor arithmetic in NumPy) plus the upload of the fp32 result
    -- the per-step host cost the route takes out of the loader; skipped, and said so, where PIL is absent,
  * the 256^2 batch-16 training step replayed from its hipGraph fed frames + matrices (``pose_img_u8`` + ``pose_img_aug``: the
    launch inside the recording, the matrices copied into their static buffer every step) against the same step fed a ready
    ``pose_img_inplane``.  The difference is the price of the feature.

Device events around windows of many calls after a warm-up; the routes of a pair alternate in the same process, ``--rounds``
windows each, and the median and the spread (min .. max) of the windows are printed.  The outputs of the two routes are checked
to be the same bytes before anything is timed.  Needs the GPU; there is no fallback.

    python tools/time_appearance_aug.py --out profiles/appearance_aug_time.txt
"""
import argparse
import copy
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 16


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


def pillow_batch(frames, mats, args, rounds):
    """Seconds per batch on one host thread including the upload, (median, min, max) over ``rounds`` runs, and the images; None
    without PIL."""
    try:
        from PIL import Image
    except ImportError:
        return None, None
    p, (ox, oy), fill = args["pad"], args["origin"], args["fill"]
    oh, ow = args["out_hw"] if args["out_hw"] is not None else frames.shape[1:3]
    out, times = None, []
    for _ in range(rounds):
        t = time.perf_counter()
        u8 = []
        for f, m in zip(frames, mats):
            f = np.pad(f, ((p, p), (p, p), (0, 0)), mode="reflect") if p else f
            im = Image.fromarray(f, "RGB").transform((f.shape[1], f.shape[0]), Image.AFFINE, tuple(m), Image.BILINEAR, fillcolor=fill)
            u8.append(np.asarray(im)[oy:oy + oh, ox:ox + ow])
        out = np.stack(u8).transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0) * np.float32(2.0) - np.float32(1.0)
        torch.from_numpy(out).cuda()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    return (statistics.median(times), min(times), max(times)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_appearance_aug needs an MI355X")
    from behavior_driven_video_synthesis_amd import appearance_aug as A
    from behavior_driven_video_synthesis_amd.ops import _call, _p, _stream
    lines = [f"# tools/time_appearance_aug.py: N = {N}; {a.calls} calls per window, {a.rounds} windows per route, alternating; "
             f"us per call: median (min .. max); {torch.cuda.get_device_name(0)}"]

    def row(title, res, unit="us", scale=1.0):
        d = 3 if unit == "ms" else 1
        for n, (med, lo, hi) in res.items():
            lines.append(f"{title:<34} {n:<64} {med * scale:10.{d}f} {unit}  ({lo * scale:.{d}f} .. {hi * scale:.{d}f})")
        print("\n".join(lines[-len(res):]), flush=True)

    g = np.random.default_rng(0)
    forms, launches = {}, []
    for kind, side in (("deepfashion", 256), ("market", 128)):
        frames_np = g.integers(0, 256, size=(N, side, side, 3), dtype=np.uint8)
        hw = np.array([[side, side]] * N, dtype=np.int32)
        aug = A.AppearanceAug(kind, seed=1, crop=128, size=side)
        mats_np, args = aug.draw(hw), aug.launch_args(side, (side, side))
        frames, mats, hw_d = torch.from_numpy(frames_np).cuda(), torch.from_numpy(mats_np).cuda(), torch.from_numpy(hw).cuda()
        images, status = A.affine_images(frames, mats, hw_d, size=side, **args)
        assert not status.cpu().numpy().any() and tuple(images.shape) == (N, 3, side, side)
        host, ref = pillow_batch(frames_np, mats_np, args, 5)
        if host is None:
            lines.append(f"{kind}: Pillow on one host thread: not measured (PIL does not import here)")
        else:
            assert np.array_equal(images.cpu().numpy(), ref), f"{kind}: the kernel's images differ from Pillow's"
            lines.append(f"# {kind}: images of the kernel == Pillow {__import__('PIL').__version__}'s, bit for bit, on this batch")
            row("host, one thread + upload", {f"{kind}: Pillow transform + ToTensor arithmetic, {side}^2": host}, "ms", 1e3)
        forms[kind] = (frames, mats, hw_d, args, side)
        pad = args["pad"]
        form = f"{kind} form ({side}^2" + (f", pad {pad})" if pad else ")")
        (ox, oy), (oh, ow), fill = args["origin"], args["out_hw"] or (side, side), args["fill"]
        out, st = torch.empty_like(images), torch.empty_like(status)
        launches.append((f"vunet_appearance_affine, {form}",
                         lambda f=frames, m=mats, h=hw_d, s=side, p=pad, o=(ox, oy, oh, ow), c=fill, out=out, st=st:
                         _call("vunet_appearance_affine", _p(f), _p(h), _p(m), N, s, s, p, *o, *c, _p(out), None, _p(st), _stream())))
        launches.append((f"affine_images (+ allocations), {form}",
                         lambda f=frames, m=mats, h=hw_d, s=side, k=args: A.affine_images(f, m, h, size=s, **k)))
    row("launch", compare(launches, a.calls, a.rounds))

    # ---- the flagship step from its hipGraph: frames + matrices against a ready pose_img_inplane
    if not a.no_step:
        from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import DEFAULT_CONFIG, ShapePoseNet, synthetic_batch
        cfg = copy.deepcopy(DEFAULT_CONFIG)
        cfg["training"].update(train_regressor=False)
        cfg["data"]["appearance_aug"] = "deepfashion"
        size = cfg["data"]["spatial_size"]
        frames, mats, hw_d, args, _ = forms["deepfashion"]
        tr = ShapePoseNet(cfg, device="cuda:0", total_steps=150000, vgg_synthetic=True, hip_graph=True)
        base = synthetic_batch(N, size, "cuda:0", seed=42)
        ready = dict(base, pose_img_inplane=A.affine_images(frames, mats, hw_d, size=size, **args)[0])
        raw = dict(base, pose_img_u8=frames, pose_img_aug=mats)
        for _ in range(8):                      # the init batches, the eager device-schedule steps and both captures
            tr.train_fn(raw)
            tr.train_fn(ready)
        torch.cuda.synchronize()
        assert len(tr._graphs) == 2, len(tr._graphs)
        res = compare([("frames + matrices (pose_img_aug), launch inside", lambda: tr.train_fn(raw)),
                       ("ready fp32 pose_img_inplane", lambda: tr.train_fn(ready))], max(a.calls // 10, 5), a.rounds, warm=3)
        row(f"{size}^2 bs {N} step (hipGraph)", res, "ms", 1e-3)
        d = res["frames + matrices (pose_img_aug), launch inside"][0] - res["ready fp32 pose_img_inplane"][0]
        lines.append(f"# the feature's price in the step: {d:+.1f} us = {100 * d / res['ready fp32 pose_img_inplane'][0]:+.2f} % of the step "
                     "(the box-to-box spread of the benchmark is 0.65 %, README)")
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
