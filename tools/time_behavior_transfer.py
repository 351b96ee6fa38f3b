#!/usr/bin/env python3
"""Time the two qualitative video calls of ``render.py`` at the reference configuration (config/behavior_net.yaml: H = 1024, 51
pose dimensions, 50 frames; lib/logging.py:103-, :909-): one pair of sequences, 6 interpolation steps -> 12 roll-outs of 50
poses, 12 x 51 rendered frames at 256 x 256.  ``interpolation_video`` is split into its parts -- the slerp launch, the batched
roll-out, the projection, the render -- and timed whole, next to ``transfer_video`` (one row) and to the reference's loop
structure on the same engines: per step and direction a device -> host copy of both codes, numpy's slerp, a host -> device
copy and a batch-1 roll-out.  Random weights (no checkpoint here).  Prints one JSON line.

    python tools/time_behavior_transfer.py [--reps 5] [--size 256]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    """Median wall time in ms of ``fn`` (device work included), after two warm-up calls (graph recording)."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(out)


def host_slerp(val, low, high):
    """The spherical blend on the host, where the reference's loop computes it (lib/utils.py:920-925)."""
    c = float(np.dot(low, high)) / (float(np.linalg.norm(low)) * float(np.linalg.norm(high)))
    omega = math.acos(min(1.0, max(-1.0, c)))
    so = math.sin(omega)
    w = (1.0 - val, val) if so == 0.0 else (math.sin((1.0 - val) * omega) / so, math.sin(val * omega) / so)
    return (w[0] * low + w[1] * high).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", type=int, default=256)
    args = ap.parse_args()
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import DEFAULT_CONFIG
    from behavior_driven_video_synthesis_amd.models.pose_behavior_rnn import ResidualBehaviorNet
    from behavior_driven_video_synthesis_amd.models.vunets import VunetAlter
    from behavior_driven_video_synthesis_amd.render import PoseCamera, interpolation_video, render_sequence, transfer_video
    from behavior_driven_video_synthesis_amd.seq import slerp_codes
    torch.manual_seed(0)
    dev = "cuda:0"
    pairs, s, t, h, n = 1, 6, 50, 1024, 51
    net = ResidualBehaviorNet(n, information_bottleneck=True, decoder_arch="lstm", linear_in_decoder=False, dim_hidden_b=h).to(dev).eval()
    with torch.no_grad():
        net.decoder.n_out.weight.mul_(0.05)                 # small steps: the figure stays in the image
    kw = dict(DEFAULT_CONFIG["architecture"])
    kw.update(DEFAULT_CONFIG["data"])
    kw["spatial_size"] = args.size
    vunet = VunetAlter(n_channels_x=3, dropout_prob=0.05, **kw).to(dev).eval()
    g = torch.Generator().manual_seed(0)
    seq1 = (0.5 * torch.randn(pairs, t, n, generator=g)).to(dev)
    seq2 = (0.5 * torch.randn(pairs, t, n, generator=g)).to(dev)
    app = (torch.rand(1, 3, args.size, args.size, generator=g) * 2 - 1).to(dev)
    mean = (torch.randn(n, generator=g) * 250).numpy()
    std = (40 + 40 * torch.rand(n, generator=g)).numpy()
    ext = np.concatenate([np.eye(3), np.array([[0.0], [0.0], [5000.0]])], axis=1)
    cam = PoseCamera(mean, std, list(range(n)), ext, (1145.0, 500.0, 1145.0, 500.0), (1000, 1000), args.size, device=dev)
    steps = np.linspace(0, 1, s)
    res = {"pairs": pairs, "steps": s, "frames": t, "dim_hidden_b": h, "n_kps": n, "spatial_size": args.size}
    with torch.no_grad():
        mu = net.engine().infer_b(torch.cat([seq1, seq2]), None)[1]
        mu1, mu2 = mu[:pairs].contiguous(), mu[pairs:].contiguous()
        res["encode_ms"] = timed(lambda: net.engine().infer_b(torch.cat([seq1, seq2]), None), args.reps)
        res["slerp_launch_ms"] = timed(lambda: slerp_codes(mu1, mu2, steps), 20 * args.reps)
        codes = slerp_codes(mu1, mu2, steps).reshape(2 * pairs * s, h)
        starts = torch.stack([seq1[:, :1], seq2[:, :1]]).unsqueeze(2).expand(2, pairs, s, 1, n).reshape(2 * pairs * s, 1, n)
        res["roll_out_ms"] = timed(lambda: net.generate_seq(codes, starts, len=t, start_frame=0), args.reps)
        poses = torch.cat([starts, net.generate_seq(codes, starts, len=t, start_frame=0)[0]], dim=1)
        res["projection_ms"] = timed(lambda: cam.project(poses.reshape(-1, n)), 20 * args.reps)
        kps = cam.project(poses.reshape(-1, n)).reshape(2 * pairs * s, t + 1, -1, 2)
        res["render_ms"] = timed(lambda: [render_sequence(vunet, app, k, spatial_size=args.size, dtype="bf16", share_appearance=True)
                                          for k in kps], args.reps)
        res["interpolation_video_ms"] = timed(lambda: interpolation_video(net, vunet, app, seq1, seq2, cam, steps=steps), args.reps)
        res["interpolation_poses_only_ms"] = timed(lambda: interpolation_video(net, None, None, seq1, seq2, cam, steps=steps), args.reps)
        res["transfer_video_ms"] = timed(lambda: transfer_video(net, vunet, app, seq2, seq1, cam), args.reps)
        res["transfer_poses_only_ms"] = timed(lambda: transfer_video(net, None, None, seq2, seq1, cam), args.reps)

        def loop():
            """The reference's structure (lib/logging.py:994-1022): codes to the host, slerp there, back, one batch-1 roll-out."""
            for v in steps:
                for lo, hi, data in ((mu1, mu2, seq1), (mu2, mu1, seq2)):
                    b = torch.tensor(host_slerp(v, lo.squeeze(dim=0).cpu().numpy(), hi.squeeze(dim=0).cpu().numpy()), device=dev)
                    net.generate_seq(b.unsqueeze(dim=0), data, len=t, start_frame=0)
        res["loop_structure_codes_and_roll_outs_ms"] = timed(loop, args.reps)
    res["speedup_codes_and_roll_outs_vs_loop"] = res["loop_structure_codes_and_roll_outs_ms"] / (res["slerp_launch_ms"] + res["roll_out_ms"])
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
