#!/usr/bin/env python3
"""Time the latent diagnostics' launches (csrc/seq_latent.hip) on the GPU, beside the reference's host loop.

* ``vunet_seq_ks_norm`` at 20 000 x 1024 (the reference's n_max_umap_samples x dim_hidden_b) in column-major (the collector's
  layout) and in row-major layout, and at 2 000 x 1024;
* ``vunet_seq_latent_nll`` at 64 and 1024 rows x 1024, with the reference draw;
* the host comparator: lib/logging.py:2551-2556, ``scipy.stats.kstest(column, "norm")`` over the same columns in a Python loop on
  one host thread (without the device-to-host copy the reference makes first), when scipy is installed.

Device events around windows of launches after a warm-up, several windows in one process, median (min .. max).  The result is
also checked: the launch's statistic against scipy's on the columns the host loop ran.

    python tools/time_latent_diag.py [--out profiles/latent_diag_time.txt] [--windows 7] [--host-columns 1024]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def windows(fn, per_window, n_windows):
    """us per call: device events around ``per_window`` calls, ``n_windows`` times, after a warm-up window."""
    for _ in range(max(2, per_window // 2)):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(n_windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per_window):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / per_window)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "latent_diag_time.txt"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--host-columns", type=int, default=1024, help="columns the scipy loop runs over (its time scales linearly)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_latent_diag.py measures on the GPU: no device found")
    from behavior_driven_video_synthesis_amd import latent_diag as L
    from behavior_driven_video_synthesis_amd.ops import _call, _p, _stream
    dev = torch.device("cuda:0")
    lines = [f"# tools/time_latent_diag.py on {torch.cuda.get_device_name(0)}: device events, {args.windows} windows after a warm-up, "
             f"median (min .. max)"]
    g = torch.Generator().manual_seed(20)
    c = 1024
    host = {}
    for n, per_window in ((20000, 20), (2000, 100)):
        x = torch.randn(n, c, generator=g)
        host[n] = x.numpy()
        rows = x.to(dev)
        cols = rows.t().contiguous()
        stat = torch.empty(3, c, device=dev, dtype=torch.float64)
        p = torch.empty(c, device=dev, dtype=torch.float64)
        for name, buf, col_major in (("column-major", cols, 1), ("row-major", rows, 0)):
            def launch():
                _call("vunet_seq_ks_norm", _p(buf), buf.stride(0), col_major, n, c, 0, _p(stat), _p(p), None, _stream())
            med, lo, hi = windows(launch, per_window, args.windows)
            lines.append(f"vunet_seq_ks_norm {n:6d} x {c} {name:12s}: {med:9.1f} us per launch ({lo:.1f} .. {hi:.1f}), "
                         f"{med / c:6.3f} us per column, {per_window} launches per window")
        host[n] = (host[n], L.ks_normal(cols, col_major=True))
    # torch.sort + the statistic alone (the route of columns longer than the LDS cap), at the same size for comparison
    n = 20000
    rows = torch.from_numpy(host[n][0]).to(dev)
    stat = torch.empty(3, c, device=dev, dtype=torch.float64)
    p = torch.empty(c, device=dev, dtype=torch.float64)

    def sort_route():
        s = torch.sort(rows, dim=0)[0]
        _call("vunet_seq_ks_norm", _p(s), s.stride(0), 0, n, c, 1, _p(stat), _p(p), None, _stream())
    med, lo, hi = windows(sort_route, 20, args.windows)
    lines.append(f"torch.sort + vunet_seq_ks_norm(sorted=1) {n} x {c} row-major: {med:9.1f} us per call ({lo:.1f} .. {hi:.1f})")
    for b in (64, 1024):
        z, ld, nz = torch.randn(b, c, device=dev), torch.randn(b, device=dev), torch.randn(b, c, device=dev)
        per_row = torch.empty(2, b, device=dev, dtype=torch.float64)
        sc = torch.empty(4, device=dev, dtype=torch.float64)

        def launch():
            _call("vunet_seq_latent_nll", _p(z), c, _p(ld), _p(nz), b, c, _p(per_row), _p(sc), _stream())
        med, lo, hi = windows(launch, 200, args.windows)
        lines.append(f"vunet_seq_latent_nll {b:5d} x {c} with noise (two launches): {med:9.1f} us per call ({lo:.1f} .. {hi:.1f})")
    try:
        from scipy import stats
        import scipy
    except Exception:
        lines.append("host comparator: scipy is not installed, not measured")
    else:
        torch.set_num_threads(1)
        hc = min(args.host_columns, c)
        for n in (20000, 2000):
            x, ks = host[n]
            t0 = time.perf_counter()
            ps = np.asarray([], dtype=float)
            ds = []
            for sdim in range(hc):                       # lib/logging.py:2551-2556
                d, pv = stats.kstest(x[:, sdim], "norm")
                ps = np.append(ps, pv)
                ds.append(d)
            dt = time.perf_counter() - t0
            err = float(np.max(np.abs(ks.statistic.cpu().numpy()[:hc] - np.array(ds))))
            lines.append(f"host loop of scipy {scipy.__version__} kstest, {n:6d} x {hc} columns, one thread: {dt * 1e3:9.1f} ms "
                         f"({dt * 1e6 / hc:.1f} us per column; x {c / hc:.0f} for all {c} = {dt * 1e3 * c / hc:.0f} ms); "
                         f"max |D_launch - D_scipy| = {err:.1e}; mean p {np.mean(ps):.4f}, launch's p_mean('exact') "
                         f"{float(np.mean(ks.pvalues('exact')[:hc])):.4f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
