#!/usr/bin/env python3
"""Time the image model's scoring path (csrc/person_crop.hip, csrc/inception_score.hip, ``ShapePoseNet.evaluate``):

  * the three new launches alone: vunet_kp_boxes (16 x 17 x 2), vunet_box_crop (16 x 3 x 256^2 -> 256^2),
    vunet_inception_input_boxes (-> 299^2), and vunet_inception_score at 8000 x 1000 logits, 10 splits,
  * the crop fused into the Inception input against the two launches it replaces (crop_and_resize, then inception_input),
  * the crop against the same batch through its plain-torch restatement on the device (``F.grid_sample`` on a grid built from
    the boxes with torch ops),
  * the score's statistic against today's host path for the same logits (float64 softmax on the device, copy, scipy),
  * one ``evaluate(crop="person")`` over 64 images (batches of 16, 256^2, BASELINE-size VunetAlter, synthetic InceptionV3) against
    the same work composed from the public functions: compute_ssim, model(...) / model.transfer, bounding_box_batch, and the host
    inception_score on the stored crops.

Device events around windows of many calls after a warm-up (the paths that end on the host end in their own copy); the routes of
a pair alternate in the same process, ``--rounds`` windows each, and the median and the spread (min .. max) of the windows are
printed.  Needs the GPU; there is no fallback.

    python tools/time_image_eval.py --out profiles/image_eval_time.txt
"""
import argparse
import copy
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls     # us per call


def compare(named, calls, rounds, warm=10):
    for _, fn in named:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n, _ in named}
    for _ in range(rounds):
        for n, fn in named:                    # alternating
            times[n].append(window(fn, calls))
    return {n: (statistics.median(v), min(v), max(v)) for n, v in times.items()}


def torch_crop(img, boxes, size):
    """The REFERENCE crop with plain torch on the device: the sampled pixel coordinates from the boxes, normalised for
    ``F.grid_sample(align_corners=False)``."""
    n, _, hs, ws = img.shape
    b = boxes.to(torch.float32)
    idx = torch.arange(size, device=img.device, dtype=torch.float32)
    u = (b[:, 0:1] + idx[None] * b[:, 2:3] / (size - 1)) * ws / (ws - 1) - 0.5
    v = (b[:, 1:2] + idx[None] * b[:, 3:4] / (size - 1)) * hs / (hs - 1) - 0.5
    gx = ((2.0 * u + 1.0) / ws - 1.0)[:, None, :].expand(n, size, size)
    gy = ((2.0 * v + 1.0) / hs - 1.0)[:, :, None].expand(n, size, size)
    return torch.nn.functional.grid_sample(img, torch.stack([gx, gy], dim=-1), mode="bilinear", padding_mode="zeros", align_corners=False)


def head_commit():
    """The commit of the tree, where it is a git checkout (``--commit`` names it where it is not)."""
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-evaluate", action="store_true")
    ap.add_argument("--commit", default=None, help="the commit the tree was made from (default: git rev-parse HEAD)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_image_eval needs an MI355X")
    from behavior_driven_video_synthesis_amd import person_crop
    from behavior_driven_video_synthesis_amd.lib import metrics
    from behavior_driven_video_synthesis_amd.lib.utils import bounding_box_batch
    from behavior_driven_video_synthesis_amd.models.inception import InceptionV3, inception_input
    lines = [f"# tools/time_image_eval.py: {a.calls} calls per window (fewer where noted), {a.rounds} windows per route, alternating; us per "
             f"call: median (min .. max); {torch.cuda.get_device_name(0)}; working tree on commit {a.commit or head_commit()}"]

    def row(title, res):
        for n, (med, lo, hi) in res.items():
            lines.append(f"{title:<44} {n:<44} {med:11.1f} us  ({lo:.1f} .. {hi:.1f})")
        print("\n".join(lines[-len(res):]), flush=True)

    g = torch.Generator().manual_seed(0)
    img = (torch.rand(16, 3, 256, 256, generator=g) * 2 - 1).cuda()
    kps = (torch.rand(16, 17, 2, generator=g) * 200 + 20).cuda()
    boxes, valid = person_crop.keypoint_boxes(kps)
    logits = (4.0 * torch.randn(8000, 1000, generator=g)).cuda()

    # ---- the launches alone
    row("N = 16, 3 x 256^2 -> 256^2 -> 299^2", compare([
        ("vunet_kp_boxes", lambda: person_crop.keypoint_boxes(kps)),
        ("vunet_box_crop", lambda: person_crop.crop_and_resize(img, boxes, 256, valid)),
        ("vunet_inception_input (of a stored crop)", lambda: inception_input(img)),
        ("vunet_inception_input_boxes (fused)", lambda: person_crop.inception_input_boxes(img, boxes, 256, valid)),
        ("crop_and_resize + inception_input (two)", lambda: inception_input(person_crop.crop_and_resize(img, boxes, 256, valid))),
        ("plain torch crop (F.grid_sample)", lambda: torch_crop(img, boxes, 256))], a.calls, a.rounds))
    same = torch.equal(person_crop.inception_input_boxes(img, boxes, 256, valid), inception_input(person_crop.crop_and_resize(img, boxes, 256, valid)))
    diff = float((torch_crop(img, boxes, 256) - person_crop.crop_and_resize(img, boxes, 256, valid)).abs().max())
    lines.append(f"# fused input bit-identical to the two launches at this size: {same}; plain torch crop - kernel crop, max abs: {diff:.3e}")

    # ---- the statistic
    def host_stat():
        return metrics.inception_score_from_probs(torch.softmax(logits.double(), dim=1).cpu().numpy(), 10)
    row("8000 x 1000 logits, 10 splits", compare([("inception_score_device (4 launches + copy)", lambda: metrics.inception_score_device(logits, 10)),
                                                  ("device softmax, copy, host statistic", host_stat)], max(a.calls // 20, 3), a.rounds, warm=2))
    d, h = metrics.inception_score_device(logits, 10), host_stat()
    lines.append(f"# device (mean, std) {d}; host {h}; relative difference of the mean {abs(d[0] - h[0]) / abs(h[0]):.3e}")

    # ---- evaluate over 64 images against the composed path
    if not a.no_evaluate:
        from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import DEFAULT_CONFIG, ShapePoseNet, synthetic_batch
        cfg = copy.deepcopy(DEFAULT_CONFIG)
        size = cfg["data"]["spatial_size"]
        tr = ShapePoseNet(cfg, device="cuda:0", total_steps=1000, vgg_synthetic=True, hip_graph=False)
        net = InceptionV3(seed=3).cuda()
        batches = []
        for i in range(4):
            b = synthetic_batch(16, size, "cuda:0", seed=60 + i)
            b["keypoints"] = (torch.rand(16, 17, 2, generator=g) * 0.8 + 0.1).cuda()
            batches.append(b)

        def composed():
            model = tr.vunet
            ssim = metrics.compute_ssim(model, batches)
            model.eval()
            recs, trs = [], []
            with torch.no_grad():
                for b in batches:
                    rec = model(b["pose_img"], b["stickman"])[0]
                    t = model.transfer(b["pose_img"], b["stickman"])
                    k = b["keypoints"] * float(size)
                    recs.append(bounding_box_batch(k, rec, None, size))
                    trs.append(bounding_box_batch(k, t, None, size))
            return ssim, metrics.inception_score(torch.cat(recs), net, batch_size=16, resize=True), \
                metrics.inception_score(torch.cat(trs), net, batch_size=16, resize=True)
        row("64 images (4 x 16), 256^2, crop='person'", compare([("ShapePoseNet.evaluate", lambda: tr.evaluate(batches, net, crop="person")),
                                                               ("composed from the public functions", composed)], 2, a.rounds, warm=1))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
