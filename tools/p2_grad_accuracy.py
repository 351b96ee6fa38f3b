#!/usr/bin/env python3
"""Accuracy of the perceptual loss's opt-in p2 modes against the default (needs an MI355X).

    python tools/p2_grad_accuracy.py [--sizes 128x256,256x256] [--seeds 9,10] [--modes f16,f16grad]

lib.losses.vgg_loss on a full-width synthetic VGG19 (seed 78), batch 2, target and prediction uniform in [-1, 1] from the row's
seed -- the setup of tests/test_hip_p2_f16.py::_loss_and_gradient.  Per row: the maximum relative difference of the six loss
terms against "split", and the relative L2 distance of d loss / d pred from "split"'s.  The "fp32path" rows are the distance of the
fp32-tensor path (enable_p2(False)) from "split": what two fp32-accurate evaluations of this gradient differ by."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from behavior_driven_video_synthesis_amd.lib.losses import vgg_loss  # noqa: E402
from behavior_driven_video_synthesis_amd.models import imagenet_pretrained as ip  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="128x256,256x256")
ap.add_argument("--seeds", default="9,10")
ap.add_argument("--modes", default="f16,f16grad")
ap.add_argument("--batch", type=int, default=2)
args = ap.parse_args()
sizes = [tuple(int(v) for v in s.split("x")) for s in args.sizes.split(",")]
seeds = [int(s) for s in args.seeds.split(",")]
modes = args.modes.split(",")


def loss_and_gradient(pv, target, pred0, mode):
    prev = ip.set_p2_precision(mode)
    try:
        p = pred0.clone().requires_grad_(True)
        ld = vgg_loss(pv, target, p)
        torch.stack([v.sum() for v in ld.values()]).sum().backward()
        return {k: float(v) for k, v in ld.items()}, p.grad.double().cpu()
    finally:
        ip.set_p2_precision(prev)


pv = ip.PerceptualVGG(ip.vgg19(seed=78, width_div=1, synthetic=True, pretrained=True), [1.0, 0.5, 1.5, 1.0, 2.0, 1.0]).cuda()
print(f"full-width synthetic VGG19 (seed 78), batch {args.batch}; against \"split\": max relative difference of the loss terms, "
      "relative L2 of d loss / d pred")
print(f"{'size':>9s} {'seed':>4s} {'mode':>8s} {'loss terms':>11s} {'gradient':>10s}")
for hh, ww in sizes:
    for seed in seeds:
        g = torch.Generator().manual_seed(seed)
        target = (torch.rand(args.batch, 3, hh, ww, generator=g) * 2 - 1).cuda()
        pred0 = (torch.rand(args.batch, 3, hh, ww, generator=g) * 2 - 1).cuda()
        if pv._p2_engine(pred0) is None:
            print(f"{hh:4d}x{ww:<4d} {seed:4d}  the p2 engine declines this geometry: every mode runs the per-layer three-product path")
            continue
        ls, gs = loss_and_gradient(pv, target, pred0, "split")
        rows = [(m,) + loss_and_gradient(pv, target, pred0, m) for m in modes]
        ip.enable_p2(False)
        try:
            rows.append(("fp32path",) + loss_and_gradient(pv, target, pred0, "split"))
        finally:
            ip.enable_p2(True)
        for m, lm, gm in rows:
            loss_rel = max(abs(lm[k] - ls[k]) / abs(ls[k]) for k in ls)
            print(f"{hh:4d}x{ww:<4d} {seed:4d} {m:>8s} {loss_rel:11.3e} {float((gm - gs).norm() / gs.norm()):10.3e}")
