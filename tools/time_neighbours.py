#!/usr/bin/env python3
"""Time the two nearest-neighbour scans of ``neighbours.TrainBank`` (csrc/seq_nn.hip) at the reference's figure: Q = 100
queries against a training set of ``--n`` sequences, codes of H = 1024, sequences of T = 51 frames of J = 17 joints (the dataset
is not here, so its size is an argument; random values).  Next to each scan, in the same run, the plain torch expression on the
GPU, one query at a time as the reference's loop: ``(bank - q).norm(dim=1).argmin()`` in code space, and in pose space the
un-normalised, root-centred float64 bank (built once, outside the timing, as the reference builds ``seqs_aligned`` once) with
``(xq - bank).norm(dim=-1).sum(dim=(1, 2)).argmin()``.  The bank traffic of a scan is N x row bytes x ceil(Q / QT); its rate is
printed next to the guide's measured float4 copy rate of the device.  Prints one JSON line.

    python tools/time_neighbours.py [--n 200000] [--q 100] [--reps 5]
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

COPY_RATE = 6.29e12      # bytes/s: the measured float4 copy rate of an MI355X (8.0 TB/s is the specification's peak)


def timed(fn, reps):
    """Median wall time in ms of ``fn`` (device work included), after one warm-up call."""
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
    ap.add_argument("--n", type=int, default=200000)
    ap.add_argument("--q", type=int, default=100)
    ap.add_argument("--h", type=int, default=1024)
    ap.add_argument("--t", type=int, default=51)
    ap.add_argument("--j", type=int, default=17)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-queries", type=int, default=10, help="queries the torch expressions are timed on (scaled to --q)")
    args = ap.parse_args()
    from behavior_driven_video_synthesis_amd import neighbours as NB
    from behavior_driven_video_synthesis_amd.behavior_eval import PoseStats
    dev = "cuda:0"
    n, q, h, t, j = args.n, args.q, args.h, args.t, args.j
    d = 3 * j
    g = torch.Generator(device=dev).manual_seed(0)
    codes = torch.randn(n, h, device=dev, generator=g)
    seqs = 0.5 * torch.randn(n, t, d, device=dev, generator=g)
    mu = torch.randn(q, h, device=dev, generator=g)
    xs = 0.5 * torch.randn(q, t, d, device=dev, generator=g)
    rng = np.random.RandomState(0)
    stats = PoseStats(rng.randn(d) * 250.0, 40.0 + 40.0 * rng.rand(d), [], device=dev)
    bank = NB.TrainBank(codes, seqs, stats)
    res = {"n": n, "q": q, "h": h, "t": t, "j": j, "qt_codes": NB.QT_CODES, "qt_poses": NB.QT_POSES}
    with torch.no_grad():
        ci, _ = bank.nearest_codes(mu)
        pi, _ = bank.nearest_poses(xs, 0)
        res["codes_ms"] = timed(lambda: bank.nearest_codes(mu), args.reps)
        res["poses_ms"] = timed(lambda: bank.nearest_poses(xs, 0), args.reps)
        for key, row_bytes, qt in (("codes", 4 * h, NB.QT_CODES), ("poses", 4 * t * d, NB.QT_POSES)):
            traffic = n * row_bytes * -(-q // qt)
            res[f"{key}_bank_bytes_per_s"] = traffic / (1e-3 * res[f"{key}_ms"])
            res[f"{key}_fraction_of_copy_rate"] = res[f"{key}_bank_bytes_per_s"] / COPY_RATE
        res["copy_rate_bytes_per_s"] = COPY_RATE
        tq = max(1, min(q, args.torch_queries))

        def torch_codes():
            return torch.stack([(codes - mu[a]).norm(dim=1).argmin() for a in range(tq)])
        res["torch_codes_ms"] = timed(torch_codes, args.reps) * q / tq
        res["torch_codes_agree"] = int((torch_codes() == ci[:tq]).sum())
        del codes
        # the reference's seqs_aligned, float64, built once; chunks bound the float64 temporaries of the per-query expression
        u = (seqs.double() * stats.std + stats.mean).reshape(n, t, j, 3)
        aligned = u - u[:, :, :1]
        del u
        xa = (xs.double() * stats.std + stats.mean).reshape(q, t, j, 3)
        xa = xa - xa[:, :, :1]
        step = 25000

        def torch_poses():
            out = []
            for a in range(tq):
                sums = torch.cat([(xa[a] - aligned[s:s + step]).norm(dim=-1).sum(dim=(1, 2)) for s in range(0, n, step)])
                out.append(sums.argmin())
            return torch.stack(out)
        res["torch_poses_ms"] = timed(torch_poses, args.reps) * q / tq
        res["torch_poses_agree"] = int((torch_poses() == pi[:tq]).sum())
        res["torch_queries_timed"] = tq
    res["codes_speedup_vs_torch"] = res["torch_codes_ms"] / res["codes_ms"]
    res["poses_speedup_vs_torch"] = res["torch_poses_ms"] / res["poses_ms"]
    res["device"] = torch.cuda.get_device_name(0)
    print(json.dumps({k: (float(f"{v:.5g}") if isinstance(v, float) else v) for k, v in res.items()}))


if __name__ == "__main__":
    main()
