#!/usr/bin/env python3
"""Time one evaluation batch of ``BehaviorNet.evaluate`` at the reference configuration (config/behavior_net.yaml: H = 1024,
15 flow blocks; experiments/behavior_net.py:1112-1301): 64 rows, skip 4 -> 16 scored sequences, 50 samples, 50 frames.
Split into the batched sampling (800 rows: 13 chunks of flow reverse + roll-out), the two metric kernels and the transfer
metrics; and, for comparison, the reference's loop structure on the same engines -- 50 sequential 16-row passes, each
copied to the host and un-normalised there per sequence (revert_output_format).  Random weights (no checkpoint here).
Prints one JSON line.

    python tools/time_behavior_eval.py [--reps 5]
"""
import argparse
import json
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    from behavior_driven_video_synthesis_amd import behavior_eval as E
    from behavior_driven_video_synthesis_amd.experiments.behavior_net import BehaviorNet
    torch.manual_seed(0)
    dev = "cuda:0"
    bn = BehaviorNet(None, n_kps=51, device=dev)
    rows, skip, s, t, h = 64, 4, 50, 50, 1024
    g = torch.Generator().manual_seed(0)
    kps = (0.5 * torch.randn(rows, t + 1, 51, generator=g)).to(dev)
    fut = (0.5 * torch.randn(rows, t + 1, 51, generator=g)).to(dev)
    pair = (0.5 * torch.randn(rows, t + 1, 51, generator=g)).to(dev)
    match = (0.5 * torch.randn(rows, t + 1, 51, generator=g)).to(dev)
    mean = (torch.randn(96, generator=g) * 300).double().numpy()
    std = (50 + 200 * torch.rand(96, generator=g)).double().numpy()
    ignore = list(range(45))
    stats = E.PoseStats(mean, std, ignore, device=dev)
    x_s, target_s = kps[:, :-1].contiguous(), kps[:, 1:].contiguous()
    start = target_s[::skip].contiguous()
    n_seq = start.shape[0]
    res = {"rows": rows, "skip": skip, "n_samples": s, "seq_len": t, "dim_hidden_b": h, "n_flows": 15}
    with torch.no_grad():
        samples = {}

        def sample():
            samples["x"] = E.sample_behaviors(bn.net, bn.latent_flow, start, s, t, start_frame=t - 1)
        res["sampling_ms"] = timed(sample, args.reps)
        future = fut[::skip].contiguous()
        res["metric_kernels_ms"] = timed(lambda: E.sample_metrics(samples["x"], future, stats), 20 * args.reps)
        x_t, x_rel = pair[:, :-1].contiguous(), match[:, :-1].contiguous()
        res["transfer_ms"] = timed(lambda: E.transfer_metrics(bn.net, x_s, x_t, x_rel), args.reps)
        res["evaluate_batch_ms"] = timed(lambda: bn.evaluate([{"keypoints": kps, "future_keypoints": fut, "paired_keypoints": pair,
                                                               "matched_keypoints": match}], stats, n_samples=s, skip=skip).summary(),
                                         args.reps)
        use = np.array([d for d in range(96) if d not in set(ignore)])

        def loop():
            """The reference's structure (:1182-1217): one 16-row flow reverse + roll-out per sample, each result copied to the
            host and un-normalised there sequence by sequence."""
            for _ in range(s):
                b = bn.latent_flow.reverse(torch.randn(n_seq, h, device=dev)).reshape(n_seq, h)
                seq_s, *_ = bn.net.generate_seq(b, start, len=t, start_frame=t - 1)
                for x in seq_s.cpu().numpy():
                    full = np.zeros((t, 96), dtype=np.float32)
                    full[:, use] = x
                    _ = full * std.reshape(1, 96) + mean.reshape(1, 96)
        res["loop_structure_sampling_ms"] = timed(loop, max(2, args.reps // 2))
    res["speedup_sampling_vs_loop"] = res["loop_structure_sampling_ms"] / res["sampling_ms"]
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
