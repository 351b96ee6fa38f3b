#!/usr/bin/env python
"""Time the inference-only Inception-v3 (models/inception.py) on the GPU: FIDInceptionModel at batch 8 and 32 (from 256 x 256
images, through the resize) and InceptionV3 at batch 32 (299 x 299), seeded random weights.

Per configuration: the time of a whole forward (host clock around CALLS forwards that end in a synchronise; median, min and max
over WINDOWS windows), per image; the convolutions' FLOPs counted from the plan's descriptors over that time, as a fraction of
the 157 TFLOP/s fp32-matrix peak (a whole-forward rate over peak, not a kernel's share of peak); and the ten slowest launches,
each timed with a pair of device events around it (mean over EVENT_RUNS forwards; the event pair adds its own few microseconds
to every launch, so the sum exceeds the forward time).

For the one overlapping shape class -- square 3 x 3, pad 1, channels in 32s, a 32-wide map -- ``vunet_convg`` against
``ops.fused_conv`` (the generator's convolution, in the precision the process runs it with), alternating.
Last, the two tile forms of ``vunet_convg`` forced on layer shapes of the network: the measurements the ``tile = 0`` rule
(include/vunet_inception.h) is read off.

    python tools/time_inception.py [--out profiles/inception_time.txt]
"""
import argparse
import ctypes
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

PEAK_FP32_MATRIX = 157e12
CALLS, WINDOWS, EVENT_RUNS = 10, 7, 5


def conv_flops(plan, upto_features):
    total, per = 0, {}
    for st in plan.steps:
        if st.fn != "conv" or (upto_features and st.layer == "fc"):
            continue
        d = st.desc
        per[st.label] = 2 * d.N * d.Ho * d.Wo * d.M * d.C * d.KH * d.KW
        total += per[st.label]
    return total, per


def windows(fn):
    out = []
    for _ in range(WINDOWS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / CALLS)
    return statistics.median(out), min(out), max(out)


def time_model(name, net, x, resize_mode, upto_features, lines):
    from behavior_driven_video_synthesis_amd import _lib
    run = lambda on_step=None: net._run(x, resize_mode=resize_mode, upto_features=upto_features, on_step=on_step)  # noqa: E731
    for _ in range(3):
        run()
    med, lo, hi = windows(run)
    n = x.shape[0]
    plan, _ = net._bound_plan(x, resize_mode)
    flops, per = conv_flops(plan, upto_features)
    lines.append(f"{name}: batch {n}, input {tuple(x.shape[2:])}: {med * 1e3:.3f} ms per forward ({lo * 1e3:.3f} .. {hi * 1e3:.3f}), "
                 f"{med / n * 1e6:.1f} us per image; {flops / n / 2e9:.2f} GMAC per image in the convolutions -> "
                 f"{flops / med / 1e12:.1f} TFLOP/s = {flops / med / PEAK_FP32_MATRIX * 100:.1f} % of the 157 TFLOP/s fp32-matrix peak "
                 f"(whole forward, {len(plan.steps)} launches, arena {plan.arena_floats * 4 / 2 ** 20:.0f} MiB)")
    acc = {}
    for _ in range(EVENT_RUNS):
        evs = []

        def on_step(st, done):
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            evs.append((st, done, e))
        run(on_step)
        torch.cuda.synchronize()
        for (st, _, e0), (_, _, e1) in zip(evs[0::2], evs[1::2]):
            acc.setdefault(st.label, [st, 0.0])[1] += e0.elapsed_time(e1) / EVENT_RUNS
    lines.append(f"  ten slowest launches (device events, ms; sum of all {sum(v[1] for v in acc.values()):.3f} ms):")
    for label, (st, ms) in sorted(acc.items(), key=lambda kv: -kv[1][1])[:10]:
        if st.fn == "conv":
            d = st.desc
            tile = _lib.lib().vunet_convg_tile(ctypes.byref(d))
            grid = (-(-d.N * d.Ho * d.Wo // tile), -(-d.M // tile))
            lines.append(f"    {label:28s} {ms:8.4f}  {d.C:4d} -> {d.M:4d}  {d.KH}x{d.KW} s{d.stride_h} on {d.H}x{d.W}  tile {tile} grid {grid}  "
                         f"{per.get(label, 0) / (ms * 1e-3) / 1e12:6.1f} TFLOP/s")
        else:
            lines.append(f"    {label:28s} {ms:8.4f}  ({st.fn})")


def time_overlap(lines):
    """vunet_convg vs ops.fused_conv: 3 x 3, pad 1, stride 1, channels in 32s, a 32 x 32 map."""
    from behavior_driven_video_synthesis_amd import ops
    from behavior_driven_video_synthesis_amd.lib.modules import Conv2d
    from behavior_driven_video_synthesis_amd.models import inception as I
    lines.append(f"vunet_convg against ops.fused_conv (conv precision {ops.conv_precision()!r}), 3x3 pad 1, 32 x 32 map, us per launch "
                 f"(median of {WINDOWS} windows of {CALLS * 10} launches, alternating):")
    lines.append("  (host clock per call: below ~50 us ops.fused_conv's figure is its host path -- an autograd Function and a config per "
                 "call --, not its kernel; the larger cases compare the kernels)")
    for n, c in ((8, 32), (8, 64), (8, 128), (32, 64), (32, 128), (64, 128)):
        m = Conv2d(c, c, 3, padding=1).cuda()
        x = torch.randn(n, c, 32, 32, device="cuda")
        wp = I.pack_weight(torch.randn(c, c, 3, 3, dtype=torch.float64) / (9 * c) ** 0.5).cuda()
        b = torch.zeros(c, device="cuda")
        y = torch.empty(n, c, 32, 32, device="cuda")
        d = I.ConvgDesc(n, c, 32, 32, c, 32, 32, 3, 3, 1, 1, 1, 1, c, 0, c, 0, 0, wp.shape[0], wp.shape[1], 0)

        def convg():
            for _ in range(10):
                ops._call("vunet_convg", ctypes.byref(d), ops._p(x), ops._p(wp), ops._p(b), ops._p(y), ops._stream())

        def fused():
            with torch.no_grad():
                for _ in range(10):
                    m.fused(x)
        for _ in range(3):
            convg()
            fused()
        a, f = [], []
        for _ in range(WINDOWS):
            a.append(windows_once(convg))
            f.append(windows_once(fused))
        ta, tf = statistics.median(a) / 10, statistics.median(f) / 10
        lines.append(f"  N {n:2d}, {c:3d} -> {c:3d}: vunet_convg {ta * 1e6:7.1f}   ops.fused_conv {tf * 1e6:7.1f}   ratio convg / fused {ta / tf:.2f}")


def time_tiles(lines):
    """The two tile forms of vunet_convg on layer shapes of the network, forced: what the tile = 0 rule is read off."""
    from behavior_driven_video_synthesis_amd import ops
    from behavior_driven_video_synthesis_amd.models import inception as I
    cases = [("8x8 2048->320 1x1", 2048, 320, (1, 1), (0, 0), 8), ("8x8 448->384 3x3", 448, 384, (3, 3), (1, 1), 8),
             ("8x8 384->384 1x3", 384, 384, (1, 3), (0, 1), 8), ("17x17 768->192 1x1", 768, 192, (1, 1), (0, 0), 17),
             ("17x17 160->160 1x7", 160, 160, (1, 7), (0, 3), 17), ("17x17 192->192 7x1", 192, 192, (7, 1), (3, 0), 17),
             ("35x35 288->64 1x1", 288, 64, (1, 1), (0, 0), 35), ("35x35 96->96 3x3", 96, 96, (3, 3), (1, 1), 35),
             ("35x35 48->64 5x5", 48, 64, (5, 5), (2, 2), 35), ("73x73 64->80 1x1", 64, 80, (1, 1), (0, 0), 73),
             ("73x73 80->192 3x3", 80, 192, (3, 3), (0, 0), 73), ("147x147 32->64 3x3", 32, 64, (3, 3), (1, 1), 147),
             ("149x149 32->32 3x3", 32, 32, (3, 3), (0, 0), 149)]
    lines.append(f"vunet_convg, tile forced to 64 and to 32, us per launch (median of {WINDOWS} windows of {CALLS * 2} launches); '*' = what tile = 0 picks:")
    for n in (8, 32):
        for name, c, m, k, p, hw in cases:
            x = torch.randn(n, c, hw, hw, device="cuda")
            wp = I.pack_weight(torch.randn(m, c, *k, dtype=torch.float64) / (c * k[0] * k[1]) ** 0.5).cuda()
            ho, wo = hw + 2 * p[0] - k[0] + 1, hw + 2 * p[1] - k[1] + 1
            y, b = torch.empty(n, m, ho, wo, device="cuda"), torch.zeros(m, device="cuda")
            res = {}
            for tile in (64, 32):
                d = I.ConvgDesc(n, c, hw, hw, m, ho, wo, k[0], k[1], 1, 1, p[0], p[1], c, 0, m, 0, 1, wp.shape[0], wp.shape[1], tile)

                def fn():
                    for _ in range(2):
                        ops._call("vunet_convg", ctypes.byref(d), ops._p(x), ops._p(wp), ops._p(b), ops._p(y), ops._stream())
                fn()
                res[tile] = statistics.median(windows_once(fn) for _ in range(WINDOWS)) / 2
            d.tile = 0
            from behavior_driven_video_synthesis_amd import _lib
            pick = _lib.lib().vunet_convg_tile(ctypes.byref(d))
            tiles64 = -(-n * ho * wo // 64) * -(-m // 64)
            flops = 2 * n * ho * wo * m * c * k[0] * k[1]
            lines.append(f"  N {n:2d}  {name:20s} {tiles64:6d} tiles of 64x64   T64 {res[64] * 1e6:7.1f}{'*' if pick == 64 else ' '}  T32 {res[32] * 1e6:7.1f}"
                         f"{'*' if pick == 32 else ' '}  {flops / res[pick] / 1e12:5.1f} TFLOP/s")


def windows_once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / CALLS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_inception.py needs the GPU: a timing taken without one says nothing")
    from behavior_driven_video_synthesis_amd.models.imagenet_pretrained import FIDInceptionModel, InceptionV3
    lines = [f"# tools/time_inception.py on {torch.cuda.get_device_name(0)}: seeded random weights; {CALLS} forwards per window, {WINDOWS} "
             f"windows; median (min .. max)"]
    fid, v3 = FIDInceptionModel().cuda(), InceptionV3().cuda()
    g = torch.Generator().manual_seed(0)
    for n in (8, 32):
        x = (torch.rand(n, 3, 256, 256, generator=g) * 2 - 1).cuda()
        time_model("FIDInceptionModel", fid, x, "fid", True, lines)
        fid._plans.clear()
    x = torch.randn(32, 3, 299, 299, generator=g).cuda()
    time_model("InceptionV3", v3, x, None, False, lines)
    v3._plans.clear()
    time_overlap(lines)
    time_tiles(lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
