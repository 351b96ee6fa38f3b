#!/usr/bin/env python3
"""Time the JPEG decode (csrc/jpeg_entropy.h, csrc/jpeg.hip) at the reference's frame size, N = 16 frames of 1000 x 1002 (W x H),
4:2:0, quality 75 and 95, synthetic smooth content encoded here with Pillow:

  * the host entropy decode of the batch (``vunet_jpeg_entropy_decode`` into one buffer) on 1, 4 and 8 threads, wall clock,
  * the one upload (descriptors, tables, coefficients) and each of the two launches, device events, with bytes per second,
  * ``decode_batch`` as a whole (8 threads, wall clock to the synchronised end),
  * the same batch through Pillow on ONE host thread (``Image.open(..).convert("RGB")`` + ``np.asarray`` per frame) plus the upload
    of the uint8 stack -- what the loader pays today,
  * the 256^2 batch-16 training step replayed from its hipGraph fed JPEG bytes (``pose_img_jpeg``: the decode issued ahead of every
    replay) against the same step fed a ready device-resident ``pose_img_u8``.  The difference is what the decode costs a step
    whose loader does not hide it.

Device events around windows of many calls after a warm-up; the routes of a pair alternate in the same process, ``--rounds``
windows each, and the median and the spread (min .. max) are printed.  The decoded bytes are checked against Pillow's before
anything is timed.  Needs the GPU and, to make the streams, PIL; there is no fallback.

    python tools/time_jpeg.py --out profiles/jpeg_time.txt

``--entropy device`` (or ``both``) times the device entropy route (csrc/jpeg_huff_dec.hip, ``decode_batch(.., entropy="device")``)
on the same streams instead of (or after) the above: each of its entry points (device events around every call of a decode), the
rounds and launches the sync took, the one upload, ``decode_batch`` through the host route (8 threads) against the device route,
alternating call by call in one process, and the graph step fed bytes through each route against the resident stack.
``--table LABEL`` prints one line per quality for the library that is loaded (``VUNET_HIP_LIB``): the subsequence / workgroup size
table is made of such lines, one build per pair of constants.

    python tools/time_jpeg.py --entropy device --out profiles/jpeg_huffdec_time.txt
"""
import argparse
import copy
import ctypes
import io
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, H, W = 16, 1002, 1000


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls     # us per call


def compare(named, calls, rounds, warm=5):
    for _, fn in named:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n, _ in named}
    for _ in range(rounds):
        for n, fn in named:                    # alternating
            times[n].append(window(fn, calls))
    return {n: (statistics.median(v), min(v), max(v)) for n, v in times.items()}


def wall(fn, rounds):
    """Milliseconds per call, (median, min, max) of ``rounds`` calls, each to its synchronised end."""
    times = []
    for _ in range(rounds):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times), min(times), max(times)


def frames(seed):
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    out = []
    for _ in range(N):
        a, b, c = g.uniform(20, 90, 3)
        img = np.stack([np.sin(xx / a + k) * 70 + np.cos(yy / b - k) * 50 + np.sin((xx + yy) / c) * 20 + 128 for k in range(3)], axis=2)
        out.append(np.clip(img + g.normal(0, 2.0, img.shape), 0, 255).astype(np.uint8))
    return out


def device_route(a, J, batches, lines, row):
    """The device entropy route on ``batches`` {quality: streams}: see the module's docstring."""
    from PIL import Image
    real_call, spans = J._call, {}

    def traced(name, *args):
        e = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        e[0].record()
        real_call(name, *args)
        e[1].record()
        spans.setdefault(name, []).append(e)
    for q, streams in batches.items():
        want = np.stack([np.asarray(Image.open(io.BytesIO(s)).convert("RGB")) for s in streams])
        out, hw = J.decode_batch(streams, tag=("device", q), entropy="device")
        stats = J.last_stats()
        assert hw.tolist() == [[H, W]] * N and np.array_equal(out.cpu().numpy(), want), f"quality {q}: the device route's bytes differ from Pillow's"
        assert stats["host_fallbacks"] == 0, stats
        (bufs,) = [b for k, b in J._buffers.items() if k[2] == ("device", q)]
        nbytes, scan = bufs.entropy.upload_bytes, sum(len(s) for s in streams)
        if a.table:
            for _ in range(3):
                J.decode_batch(streams, tag=("device", q), entropy="device")
            med, lo, hi = wall(lambda: J.decode_batch(streams, tag=("device", q), entropy="device"), a.rounds)
            lines.append(f"table  {a.table:<28} quality {q}: decode_batch entropy=device {med:8.3f} ms  ({lo:.3f} .. {hi:.3f})  rounds {stats['rounds']}, "
                         f"launches {stats['launches']}, subsequences {stats['subsequences']}")
            print(lines[-1], flush=True)
            continue
        lines.append(f"# quality {q}: {scan / N / 1024:.0f} KiB per stream; decode_batch(entropy=\"device\") == Pillow, bit for bit; sync: {stats['rounds']} rounds "
                     f"in {stats['launches']} launches, {stats['subsequences']} subsequences ({-(-stats['subsequences'] // 64)} waves), 0 host fallbacks")
        print(lines[-1], flush=True)
        # ---- every entry point of one decode, device events around each call
        J._call = traced
        try:
            for i in range(3 + a.rounds):
                if i == 3:
                    spans.clear()
                J.decode_batch(streams, tag=("device", q), entropy="device")
        finally:
            J._call = real_call
        torch.cuda.synchronize()
        for name, events in spans.items():
            calls = len(events) // a.rounds                     # of one decode; their times are summed
            per = [sum(x.elapsed_time(y) for x, y in events[r * calls:(r + 1) * calls]) * 1e3 for r in range(a.rounds)]
            row("launch", f"quality {q}: {name}" + (f" ({calls} calls, {stats['launches']} launches)" if calls > 1 else ""),
                (statistics.median(per), min(per), max(per)), "us")
        res = compare([("upload", lambda: bufs.dev[:nbytes].copy_(bufs.stage[:nbytes], non_blocking=True))], a.calls, a.rounds)
        row("upload", f"quality {q}: descriptors + tables + rows + scan bytes, pinned", res["upload"], "us",
            f"  {nbytes / 1e6:.2f} MB, {nbytes / res['upload'][0] / 1e3:.1f} GB/s")
        # ---- the two routes, alternating call by call
        routes = {"host": lambda: J.decode_batch(streams, tag=("host", q)), "device": lambda: J.decode_batch(streams, tag=("device", q), entropy="device")}
        times = {k: [] for k in routes}
        for k, fn in routes.items():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            for k, fn in routes.items():
                t = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t) * 1e3)
        for k, v in times.items():
            row("decode_batch, to the sync", f"quality {q}: entropy=\"{k}\"" + (", 8 threads" if k == "host" else ""),
                (statistics.median(v), min(v), max(v)), "ms")
        assert np.array_equal(out.cpu().numpy(), want)
    if a.table or a.no_step:
        return
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import DEFAULT_CONFIG, ShapePoseNet, synthetic_batch
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["training"].update(train_regressor=False)
    size = cfg["data"]["spatial_size"]
    tr = ShapePoseNet(cfg, device="cuda:0", total_steps=150000, vgg_synthetic=True, hip_graph=True)
    base = synthetic_batch(N, size, "cuda:0", seed=42)
    base.pop("pose_img")
    ready = dict(base, pose_img_u8=J.decode_batch(batches[75], tag="ready")[0].clone())

    def fed(q, mode):
        batch = dict(base, pose_img_jpeg=batches[q])

        def step():
            tr.config["data"]["jpeg_entropy"] = mode            # (read at every step)
            return tr.train_fn(batch)
        return step
    named = [("ready device-resident pose_img_u8", lambda: tr.train_fn(ready))]
    named += [(f"pose_img_jpeg, quality {q}, entropy=\"{mode}\"", fed(q, mode)) for q in (75, 95) for mode in ("host", "device")]
    for _ in range(8):
        for _, fn in named:
            fn()
    torch.cuda.synchronize()
    res = compare(named, max(a.calls // 4, 5), a.rounds, warm=2)
    for n, r in res.items():
        row(f"{size}^2 bs {N} step (hipGraph)", n, tuple(v * 1e-3 for v in r), "ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--entropy", choices=("host", "device", "both"), default="host")
    ap.add_argument("--table", default=None, help="print one line per quality for the loaded library, labelled so, and stop")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_jpeg needs an MI355X")
    try:
        from PIL import Image
    except ImportError:
        raise SystemExit("time_jpeg needs PIL to encode its frames")
    from behavior_driven_video_synthesis_amd import _lib, jpeg_decode as J
    from behavior_driven_video_synthesis_amd.ops import _call, _p, _stream
    lines = [f"# tools/time_jpeg.py: N = {N} frames of {W} x {H}, 4:2:0; {a.calls} calls per window, {a.rounds} windows per route, "
             f"alternating; median (min .. max); {torch.cuda.get_device_name(0)}; Pillow {__import__('PIL').__version__}"]

    def row(title, name, res, unit, extra=""):
        med, lo, hi = res
        lines.append(f"{title:<30} {name:<58} {med:10.3f} {unit}  ({lo:.3f} .. {hi:.3f}){extra}")
        print(lines[-1], flush=True)

    raw = frames(0)
    batches = {}
    if a.entropy != "host" or a.table:
        lines[0] = lines[0].replace("tools/time_jpeg.py:", f"tools/time_jpeg.py --entropy {a.entropy}:") + \
            f"; subsequences of {J.SUBSEQ_BYTES} bytes, workgroups of {J.GROUP}"
        for q in (75, 95):
            batches[q] = []
            for f in raw:
                buf = io.BytesIO()
                Image.fromarray(f, "RGB").save(buf, "JPEG", quality=q, subsampling=2)
                batches[q].append(buf.getvalue())
        device_route(a, J, batches, lines, row)
    for q in (75, 95) if a.entropy != "device" and not a.table else ():
        streams = []
        for f in raw:
            buf = io.BytesIO()
            Image.fromarray(f, "RGB").save(buf, "JPEG", quality=q, subsampling=2)
            streams.append(buf.getvalue())
        batches[q] = streams
        kb = sum(len(s) for s in streams) / N / 1024
        # ---- the bytes first
        want = np.stack([np.asarray(Image.open(io.BytesIO(s)).convert("RGB")) for s in streams])
        out, hw = J.decode_batch(streams, tag=q)
        assert hw.tolist() == [[H, W]] * N and np.array_equal(out.cpu().numpy(), want), f"quality {q}: the decoder's bytes differ from Pillow's"
        lines.append(f"# quality {q}: {kb:.0f} KiB per stream; decode_batch == Pillow, bit for bit, on this batch")
        # ---- host entropy decode alone
        infos = [J._parse_c(s) for s in streams]
        ncoef = infos[0].ncoef
        coef, qtab = np.empty(N * ncoef, dtype=np.int16), np.empty(N * 192, dtype=np.uint16)
        fn = _lib.lib().vunet_jpeg_entropy_decode

        def one(i):
            return fn(streams[i], len(streams[i]), ctypes.byref(infos[i]), coef.ctypes.data + 2 * i * ncoef, qtab.ctypes.data + 384 * i)
        for t in (1, 4, 8):
            with ThreadPoolExecutor(max_workers=t) as ex:
                assert not any(ex.map(one, range(N)))
                row("host entropy decode", f"quality {q}, {t} thread{'s' if t > 1 else ''}, batch of {N}",
                    wall(lambda: list(ex.map(one, range(N))), a.rounds), "ms")
        # ---- upload and launches
        (bufs,) = [b for k, b in J._buffers.items() if k[2] == q]
        m, nbytes, q_off, c_off, count, _ = bufs.layout             # (the plan of the call above)
        base, host = bufs.dev.data_ptr(), ctypes.c_void_p(bufs.stage.data_ptr())
        args = (ctypes.c_void_p(base + c_off), count, ctypes.c_void_p(base + q_off), N * 192, ctypes.c_void_p(base), host, m)
        res = compare([("upload", lambda: bufs.dev[:nbytes].copy_(bufs.stage[:nbytes], non_blocking=True)),
                       ("idct", lambda: _call("vunet_jpeg_idct", *args, _p(bufs.planes), count, _stream())),
                       ("rgb", lambda: _call("vunet_jpeg_to_rgb", _p(bufs.planes), count, args[4], host, m, N, H, W, _p(out), _stream()))],
                      a.calls, a.rounds)
        moved = {"upload": nbytes, "idct": 3 * count, "rgb": count + 3 * N * H * W}
        names = {"upload": f"quality {q}: descriptors + tables + coefficients, pinned", "idct": f"quality {q}: vunet_jpeg_idct",
                 "rgb": f"quality {q}: vunet_jpeg_to_rgb"}
        for k, r in res.items():
            row("upload" if k == "upload" else "launch", names[k], r, "us", f"  {moved[k] / 1e6:.1f} MB, {moved[k] / r[0] / 1e3:.1f} GB/s")
        assert np.array_equal(out.cpu().numpy(), want)
        row("decode_batch, 8 threads", f"quality {q}: entropy + upload + 2 launches, to the sync", wall(lambda: J.decode_batch(streams, tag=q), a.rounds), "ms")

        def pillow():
            torch.from_numpy(np.stack([np.asarray(Image.open(io.BytesIO(s)).convert("RGB")) for s in streams])).cuda()
        row("host, one thread + upload", f"quality {q}: Pillow Image.open + convert + asarray", wall(pillow, a.rounds), "ms")

    # ---- the flagship step from its hipGraph: JPEG bytes against a ready pose_img_u8
    if not a.no_step and a.entropy != "device" and not a.table:
        from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import DEFAULT_CONFIG, ShapePoseNet, synthetic_batch
        cfg = copy.deepcopy(DEFAULT_CONFIG)
        cfg["training"].update(train_regressor=False)
        size = cfg["data"]["spatial_size"]
        tr = ShapePoseNet(cfg, device="cuda:0", total_steps=150000, vgg_synthetic=True, hip_graph=True)
        base = synthetic_batch(N, size, "cuda:0", seed=42)
        base.pop("pose_img")
        ready = dict(base, pose_img_u8=J.decode_batch(batches[75], tag="ready")[0].clone())
        named = [("ready device-resident pose_img_u8", lambda: tr.train_fn(ready))]
        for q in (75, 95):
            named.append((f"pose_img_jpeg, quality {q}, decode ahead of the replay", lambda b=dict(base, pose_img_jpeg=batches[q]): tr.train_fn(b)))
        for _ in range(8):                      # the init batches, the eager device-schedule steps and the capture
            for _, fn in named:
                fn()
        torch.cuda.synchronize()
        res = compare(named, max(a.calls // 4, 5), a.rounds, warm=2)
        for n, r in res.items():
            row(f"{size}^2 bs {N} step (hipGraph)", n, tuple(v * 1e-3 for v in r), "ms")
        lines.append(f"# graphs recorded: {len(tr._graphs)} (the JPEG batches replay the recording of their stack shape)")
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
