#!/usr/bin/env python3
"""Time the FID statistic on the device (csrc/fid.hip, fid_device.py) at the reference's size, 8000 x 2048 features in both sets:

  * the centring launch pair (vunet_fid_center) and one dot product over 8000 x 2048 (vunet_f64_dot),
  * vunet_f64_gemm in the three forms the iteration uses -- TN (X^T X, 2048 x 2048 x 8000), NN (X G, 8000 x 2048 x 2048), NT
    (X X^T on a wide 1024 x 2048 operand) -- with the rate 2 M N K / time against the vendor's peak figure for FP64 on the
    matrix cores (78.6 TFLOP/s, AMD's MI355X data sheet: a vendor figure, not measured here),
  * ``fid_device`` as a whole, with its iteration counts, against the host route for the same features: the per-batch
    ``.double().cpu().numpy()`` copies of ``compute_fid`` (250 batches of 32 per set), ``np.mean`` / ``np.cov`` and
    ``scipy.linalg.sqrtm`` (``lib.metrics.fid_from_features``) on the threads this process may use.

Device events around windows of calls after a warm-up for the launches; the wall clock around synchronised calls for the routes
that end on the host.  No bound was set beforehand.  Needs the GPU; there is no fallback.

    python tools/time_fid.py --out profiles/fid_time.txt
"""
import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_F64_MATRIX_TFLOPS = 78.6      # vendor figure (MI355X data sheet, FP64 matrix)


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls     # us per call


def timed(fn, calls, rounds, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    v = [window(fn, calls) for _ in range(rounds)]
    return statistics.median(v), min(v), max(v)


def wall(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, time.perf_counter() - t


def features(n, d, shift, seed):
    """Correlated, rectified, column-scaled features (the construction of tests/fid_ref.py at size): fp32 [n, d] on the device."""
    g = torch.Generator().manual_seed(seed)
    r = torch.randn(n, d + 1, generator=g, dtype=torch.float64)
    c = torch.randn(n, 1, generator=g, dtype=torch.float64)
    scale = torch.ldexp(torch.ones(d, dtype=torch.float64), -((torch.arange(d) * 8) // (d - 1)))[None]
    return torch.relu(scale * (r[:, :d] + 0.5 * r[:, 1:] + 0.5 * c) + shift * scale).float().cuda()


def head_commit():
    try:
        return subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True, text=True).stdout.strip() or "unknown"
    except OSError:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=8000)
    ap.add_argument("--d", type=int, default=2048)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-host", action="store_true", help="skip the host route (scipy.linalg.sqrtm at 2048 takes a while)")
    ap.add_argument("--commit", default=None, help="the commit the tree was made from (default: git rev-parse HEAD)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_fid needs an MI355X")
    from behavior_driven_video_synthesis_amd import fid_device as F
    from behavior_driven_video_synthesis_amd.lib import metrics
    n, d = a.n, a.d
    lines = [f"# tools/time_fid.py: {n} x {d} features in both sets; launches: {a.calls} calls per window, {a.rounds} windows, us per call: "
             f"median (min .. max); {torch.cuda.get_device_name(0)}; working tree on commit {a.commit or head_commit()}",
             f"# TFLOP/s = 2 M N K / time; the percentage is of {PEAK_F64_MATRIX_TFLOPS} TFLOP/s, the vendor's FP64 matrix peak (a data-sheet "
             "figure, not measured here)"]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    gt, gen = features(n, d, 0.5, 1), features(n, d, 0.75, 2)
    mu, y = F._center(gt)
    work = torch.empty(256, device="cuda", dtype=torch.float64)
    out1 = torch.empty(1, device="cuda", dtype=torch.float64)
    med, lo, hi = timed(lambda: F._center(gt), a.calls, a.rounds)
    say(f"{'vunet_fid_center (mean + centre), fp32 in':<58} {med:11.1f} us  ({lo:.1f} .. {hi:.1f})")
    med, lo, hi = timed(lambda: F._dot(y, y, work, out1), a.calls, a.rounds)
    say(f"{'vunet_f64_dot over N x D':<58} {med:11.1f} us  ({lo:.1f} .. {hi:.1f})")

    x = y / float(torch.linalg.matrix_norm(y))
    gram = torch.empty(d, d, device="cuda", dtype=torch.float64)
    xn = torch.empty_like(x)
    wide = x[:min(1024, n)].contiguous()
    gw = torch.empty(wide.shape[0], wide.shape[0], device="cuda", dtype=torch.float64)
    for title, (m_, n_, k_), fn in (
            (f"vunet_f64_gemm TN  X^T X   {d} x {d} x {n}", (d, d, n), lambda: F.gemm_f64(x, x, trans_a=True, alpha=-0.5, diag=1.5, out=gram)),
            (f"vunet_f64_gemm NN  X G     {n} x {d} x {d}", (n, d, d), lambda: F.gemm_f64(x, gram, out=xn)),
            (f"vunet_f64_gemm NT  X X^T   {wide.shape[0]} x {wide.shape[0]} x {d}", (wide.shape[0], wide.shape[0], d),
             lambda: F.gemm_f64(wide, wide, trans_b=True, alpha=-0.5, diag=1.5, out=gw))):
        med, lo, hi = timed(fn, a.calls, a.rounds)
        tf = 2.0 * m_ * n_ * k_ / (med * 1e-6) / 1e12
        say(f"{title:<58} {med:11.1f} us  ({lo:.1f} .. {hi:.1f})  {tf:6.2f} TFLOP/s  {100 * tf / PEAK_F64_MATRIX_TFLOPS:5.1f} % of the vendor peak")

    # ---- the whole statistic
    F.fid_device(gt[:256], gen[:256])                       # warm-up of every launch
    dev = []
    for _ in range(3):
        res, t = wall(lambda: F.fid_device(gt, gen))
        dev.append(t)
    say(f"{'fid_device, whole statistic (features on the device)':<58} {statistics.median(dev) * 1e3:11.1f} ms  ({min(dev) * 1e3:.1f} .. "
        f"{max(dev) * 1e3:.1f}); iterations {res.iters}, converged {res.converged}, fid {res.fid!r}")
    if not a.no_host:
        threads = os.environ.get("OMP_NUM_THREADS", f"unset ({os.cpu_count()} cpus)")

        def copies():
            return [np.concatenate([f[i:i + 32].detach().double().cpu().numpy() for i in range(0, n, 32)], axis=0) for f in (gt, gen)]
        (hg, hn), t_copy = wall(copies)
        t0 = time.perf_counter()
        m1, c1, m2, c2 = np.mean(hg, axis=0), np.cov(hg, rowvar=False), np.mean(hn, axis=0), np.cov(hn, rowvar=False)
        t_cov = time.perf_counter() - t0
        t0 = time.perf_counter()
        host = metrics._calculate_fid(m1, c1, m2, c2)
        t_sqrtm = time.perf_counter() - t0
        say(f"{'host route, once (OMP_NUM_THREADS = ' + threads + ')':<58} {(t_copy + t_cov + t_sqrtm) * 1e3:11.1f} ms  = per-batch copies "
            f"{t_copy * 1e3:.1f} + mean / np.cov {t_cov * 1e3:.1f} + _calculate_fid (sqrtm) {t_sqrtm * 1e3:.1f}; fid {host!r}")
        say(f"# device - host, relative: {abs(res.fid - host) / abs(host):.3e}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
