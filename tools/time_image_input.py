#!/usr/bin/env python3
"""Time the raw-frame input route (csrc/image_input.hip) at the trainers' size, N = 16 frames of 1000 x 1002 -> 256 x 256:

  * the launches: vunet_image_input_tables alone, vunet_image_input_resample (horizontal + vertical pass) alone, and
    ``frames_to_images`` (all three, with its two output allocations),
  * the same batch through Pillow on ONE host thread (``Image.fromarray(f).resize((256, 256), Image.BICUBIC)`` per frame, then the
    ToTensor arithmetic in NumPy) -- the host cost the route takes out of the loader; skipped, and said so, where PIL is absent,
  * the 256^2 batch-16 training step replayed from its hipGraph fed raw frames (``pose_img_u8``: the three launches inside the
    recording) against the same step fed the ready fp32 ``pose_img``.

Device events around windows of many calls after a warm-up; the routes of a pair alternate in the same process, ``--rounds``
windows each, and the median and the spread (min .. max) of the windows are printed.  The outputs of the two routes are checked
to be the same bytes before anything is timed.  Needs the GPU; there is no fallback.

    python tools/time_image_input.py --out profiles/image_input_time.txt
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, H, W, S = 16, 1000, 1002, 256


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


def pillow_batch(frames, rounds):
    """Seconds per batch on one host thread, (median, min, max) over ``rounds`` runs, and the images; None without PIL."""
    try:
        from PIL import Image
    except ImportError:
        return None, None
    out, times = None, []
    for _ in range(rounds):
        t = time.perf_counter()
        u8 = np.stack([np.asarray(Image.fromarray(f, "RGB").resize((S, S), Image.BICUBIC)) for f in frames])
        out = u8.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0) * np.float32(2.0) - np.float32(1.0)
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
        raise SystemExit("time_image_input needs an MI355X")
    from behavior_driven_video_synthesis_amd import image_input as I
    from behavior_driven_video_synthesis_amd.ops import _call, _p, _stream
    lines = [f"# tools/time_image_input.py: N = {N}, {H} x {W} x 3 uint8 -> {S}^2; {a.calls} calls per window, {a.rounds} windows per "
             f"route, alternating; us per call: median (min .. max); {torch.cuda.get_device_name(0)}"]

    def row(title, res, unit="us", scale=1.0):
        d = 3 if unit == "ms" else 1
        for n, (med, lo, hi) in res.items():
            lines.append(f"{title:<34} {n:<44} {med * scale:10.{d}f} {unit}  ({lo * scale:.{d}f} .. {hi * scale:.{d}f})")
        print("\n".join(lines[-len(res):]), flush=True)

    frames_np = np.random.default_rng(0).integers(0, 256, size=(N, H, W, 3), dtype=np.uint8)
    frames = torch.from_numpy(frames_np).cuda()
    geom = torch.tensor([[H, W, 0, 0, W, H]] * N, dtype=torch.int32).cuda()
    images, status = I.frames_to_images(frames, geom, S)
    assert not status.cpu().numpy().any()

    # ---- Pillow on one host thread, and the same bytes from both routes
    host, ref = pillow_batch(frames_np, 3)
    if host is None:
        lines.append("Pillow on one host thread: not measured (PIL does not import here)")
    else:
        assert np.array_equal(images.cpu().numpy(), ref), "the kernels' images differ from Pillow's"
        lines.append(f"# images of the kernels == Pillow {__import__('PIL').__version__}'s, bit for bit, on this batch")
        row("host, one thread", {"Pillow resize + ToTensor arithmetic, 16 frames": host}, "ms", 1e3)

    # ---- the launches
    coef, bounds, inter = I._scratch_for(N, H, W, S, frames.device)
    kmax = int(coef.shape[3])
    out = torch.empty_like(images)

    def tables():
        _call("vunet_image_input_tables", _p(geom), N, H, W, S, kmax, _p(coef), _p(bounds), _p(status), _stream())

    def resample():
        _call("vunet_image_input_resample", _p(frames), _p(geom), N, H, W, S, kmax, _p(coef), _p(bounds), _p(status), _p(inter), _p(out),
              None, _stream())

    res = compare([("vunet_image_input_tables", tables), ("vunet_image_input_resample (h + v pass)", resample),
                   ("frames_to_images (all three)", lambda: I.frames_to_images(frames, geom, S))], a.calls, a.rounds)
    row("launches", res)
    moved = N * (H * W * 3 + 2 * H * S * 3 + S * S * 3 * 4)      # frames read, intermediate written and read, fp32 written
    lines.append(f"# resample: {moved / 1e6:.1f} MB moved per call (frames in, uint8 intermediate out and in, fp32 out) -> "
                 f"{moved / res['vunet_image_input_resample (h + v pass)'][0] / 1e3:.1f} GB/s")
    print(lines[-1], flush=True)

    # ---- the flagship step from its hipGraph: raw frames against ready tensors
    if not a.no_step:
        from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import DEFAULT_CONFIG, ShapePoseNet, synthetic_batch
        import copy
        cfg = copy.deepcopy(DEFAULT_CONFIG)
        cfg["training"].update(train_regressor=False)
        size = cfg["data"]["spatial_size"]
        tr = ShapePoseNet(cfg, device="cuda:0", total_steps=150000, vgg_synthetic=True, hip_graph=True)
        base = synthetic_batch(N, size, "cuda:0", seed=42)
        ready = dict(base, pose_img=I.frames_to_images(frames, geom, size)[0])
        raw = {k: v for k, v in base.items() if k != "pose_img"}
        raw.update(pose_img_u8=frames, pose_img_geom=geom)
        for _ in range(8):                      # the init batches, the eager device-schedule steps and both captures
            tr.train_fn(raw)
            tr.train_fn(ready)
        torch.cuda.synchronize()
        assert len(tr._graphs) == 2, len(tr._graphs)
        res = compare([("raw frames (pose_img_u8), resize inside", lambda: tr.train_fn(raw)),
                       ("ready fp32 pose_img", lambda: tr.train_fn(ready))], max(a.calls // 10, 5), a.rounds, warm=3)
        row(f"{size}^2 bs {N} step (hipGraph)", res, "ms", 1e-3)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
