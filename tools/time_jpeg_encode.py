#!/usr/bin/env python3
"""Time the JPEG encode (csrc/jpeg_enc.hip, csrc/jpeg_huff.hip, csrc/jpeg_huff_enc.h) at two batch shapes, 50 frames of 256 x 256 and 16 frames of
1000 x 1002 (W x H), 4:2:0, quality 75 and 95, synthetic smooth content with a little noise:

  * each of the two launches, device events, with the bytes it moves and TB/s,
  * the download of the coefficients into the pinned buffer, device events, GB/s,
  * the host entropy coder of the batch (``vunet_jpeg_entropy_encode`` from the pinned coefficients) on 1, 4 and 8 threads, wall clock,
  * ``encode_batch`` as a whole (8 threads, wall clock to its end -- it ends synchronised: the bytes are on the host),
  * the same frames through a download of the pixels plus Pillow's ``Image.save`` on ONE host thread -- what a user of the package
    pays without it,
  * the device entropy coder (``entropy="device"``): each of its entry points, device events -- vunet_jpeg_huff_count (zero +
    histogram), vunet_jpeg_huff_lengths (zero + lengths + prefix sum), vunet_jpeg_huff_pack (zero + pack), vunet_jpeg_huff_stuff
    (count + prefix sum + write) -- and the bytes its final download carries against the coefficients' download,
  * ``encode_batch`` as a whole on the four routes host / device x plain / ``optimize=True``, wall clock, alternating call by call in
    one process; the optimised bytes are checked against Pillow's ``optimize=True`` first,
  * the batch's stream bytes, plain against optimised.

Device events around windows of many calls after a warm-up; the routes of a group alternate in the same process, ``--rounds``
windows each, and the median and the spread (min .. max) are printed.  The encoded bytes are checked against Pillow's before anything
is timed.  No bound is set here: the numbers are what they are.  Needs the GPU and PIL; there is no fallback.

    python tools/time_jpeg_encode.py --out profiles/jpeg_encode_time.txt
"""
import argparse
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

SHAPES = [(50, 256, 256), (16, 1002, 1000)]      # N, H, W


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
    fn()
    times = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times), min(times), max(times)


def wall_alternating(named, rounds):
    """``wall`` for several routes whose calls alternate: {name: (median, min, max)} in ms."""
    for _, fn in named:
        fn()
    times = {n: [] for n, _ in named}
    for _ in range(rounds):
        for n, fn in named:
            torch.cuda.synchronize()
            t = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[n].append((time.perf_counter() - t) * 1e3)
    return {n: (statistics.median(v), min(v), max(v)) for n, v in times.items()}


def frames(n, h, w, seed):
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    out = []
    for _ in range(n):
        a, b, c = g.uniform(20, 90, 3)
        img = np.stack([np.sin(xx / a + k) * 70 + np.cos(yy / b - k) * 50 + np.sin((xx + yy) / c) * 20 + 128 for k in range(3)], axis=2)
        out.append(np.clip(img + g.normal(0, 2.0, img.shape), 0, 255).astype(np.uint8))
    return np.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_jpeg_encode needs an MI355X")
    try:
        from PIL import Image
    except ImportError:
        raise SystemExit("time_jpeg_encode needs PIL for the comparison")
    from behavior_driven_video_synthesis_amd import _lib, jpeg_encode as J
    from behavior_driven_video_synthesis_amd.ops import _call, _p, _stream
    lines = [f"# tools/time_jpeg_encode.py: 4:2:0; {a.calls} calls per window, {a.rounds} windows per route, alternating; median "
             f"(min .. max); {torch.cuda.get_device_name(0)}; Pillow {__import__('PIL').__version__}"]

    def row(title, name, res, unit, extra=""):
        med, lo, hi = res
        lines.append(f"{title:<30} {name:<62} {med:10.3f} {unit}  ({lo:.3f} .. {hi:.3f}){extra}")
        print(lines[-1], flush=True)

    def pillow_bytes(f, q, optimize=False):
        buf = io.BytesIO()
        Image.fromarray(f, "RGB").save(buf, "JPEG", quality=q, subsampling=2, optimize=optimize)
        return buf.getvalue()

    for n, h, w in SHAPES:
        raw = frames(n, h, w, 0)
        dev = torch.from_numpy(raw).cuda()
        lines.append(f"# ---- {n} frames of {w} x {h}")
        print(lines[-1], flush=True)
        for q in (75, 95):
            # ---- the bytes first
            J.clear_buffers()
            streams = J.encode_batch(dev, quality=q, subsampling="4:2:0")
            assert streams == [pillow_bytes(f, q) for f in raw], f"quality {q}: the encoder's bytes differ from Pillow's"
            kb = sum(len(s) for s in streams) / n / 1024
            lines.append(f"# quality {q}: {kb:.0f} KiB per stream; encode_batch == Pillow's Image.save, byte for byte, on this batch")
            (bufs,) = J._buffers.values()
            info = J.JpegInfoC()
            _call("vunet_jpeg_encode_info", h, w, 3, 2, 2, ctypes.byref(info))
            count, q_off = n * info.ncoef, n * ctypes.sizeof(J.JpegImg)
            base, host = bufs.dev.data_ptr(), ctypes.c_void_p(bufs.stage.data_ptr())
            imgs, qtab = ctypes.c_void_p(base), ctypes.c_void_p(base + q_off)
            res = compare([("rgb", lambda: _call("vunet_jpeg_from_rgb", _p(dev), n, h, w, 3, imgs, host, n, _p(bufs.planes), count, _stream())),
                           ("fdct", lambda: _call("vunet_jpeg_fdct", _p(bufs.planes), count, qtab, 192, imgs, host, n, _p(bufs.coef), count, _stream())),
                           ("down", lambda: bufs.coef_host[:count].copy_(bufs.coef[:count], non_blocking=True))], a.calls, a.rounds)
            moved = {"rgb": 3 * n * h * w + count, "fdct": 3 * count, "down": 2 * count}
            names = {"rgb": f"quality {q}: vunet_jpeg_from_rgb (pixels in, planes out)", "fdct": f"quality {q}: vunet_jpeg_fdct (planes in, int16 out)",
                     "down": f"quality {q}: coefficients to the pinned buffer"}
            for k, r in res.items():
                row("download" if k == "down" else "launch", names[k], r, "us", f"  {moved[k] / 1e6:.1f} MB, {moved[k] / r[0] / 1e6:.3f} TB/s")
            torch.cuda.synchronize()
            # ---- the host entropy coder alone, from the pinned coefficients
            fn, tables = _lib.lib().vunet_jpeg_entropy_encode, J.quant_tables(q)[[0, 1, 1]].copy()
            cap = 1024 + 2 * info.ncoef
            out = np.empty(n * cap, dtype=np.uint8)
            cbase = bufs.coef_host.data_ptr()

            def one(i):
                length = ctypes.c_int64(0)
                rc = fn(ctypes.c_void_p(cbase + 2 * i * info.ncoef), ctypes.byref(info), tables.ctypes.data, out.ctypes.data + i * cap, cap,
                        ctypes.byref(length))
                return rc, length.value
            assert [v for _, v in map(one, range(n))] == [len(s) for s in streams]
            for t in (1, 4, 8):
                with ThreadPoolExecutor(max_workers=t) as ex:
                    row("host entropy coder", f"quality {q}, {t} thread{'s' if t > 1 else ''}, batch of {n}",
                        wall(lambda: list(ex.map(one, range(n))), a.rounds), "ms")
            row("encode_batch, 8 threads", f"quality {q}: upload + 2 launches + download + entropy coder", wall(
                lambda: J.encode_batch(dev, quality=q, subsampling="4:2:0"), a.rounds), "ms")

            def pillow():
                return [pillow_bytes(f, q) for f in dev.cpu().numpy()]
            row("host, one thread", f"quality {q}: download of the pixels + Pillow Image.save", wall(pillow, a.rounds), "ms")
            # ---- the device entropy coder: the bytes first, then its entry points on what the last call left in the buffers
            optimised = [pillow_bytes(f, q, True) for f in raw]
            for entropy in ("host", "device"):
                assert J.encode_batch(dev, quality=q, subsampling="4:2:0", entropy=entropy, optimize=True) == optimised, \
                    f"quality {q}, {entropy}: the optimised bytes differ from Pillow's"
            assert J.encode_batch(dev, quality=q, subsampling="4:2:0", entropy="device") == streams
            plain_bytes, opt_bytes = sum(len(s) for s in streams), sum(len(s) for s in optimised)
            lines.append(f"# quality {q}: the batch's streams: {plain_bytes} bytes plain, {opt_bytes} bytes with optimize=True "
                         f"({100 * (1 - opt_bytes / plain_bytes):.1f} % smaller); both routes == Pillow's optimize=True, byte for byte")
            print(lines[-1], flush=True)
            ent, blocks = bufs.entropy, n * info.nblocks
            (spans_off, codes_off, _), (_, start_at, _) = ent.layout                # the plain call above left one row of codes
            hb, db = ent.up.data_ptr(), ent.up_dev.data_ptr()
            spans = ent.up.numpy()[spans_off:spans_off + 16 * n].view(np.int64).reshape(n, 2)
            unstuffed = int(((spans[:, 1] + 7) // 8).sum())
            raw_bytes, out_cap = int(spans[-1, 0] + ((spans[-1, 1] + 7) // 8 + J.CHUNK - 1) // J.CHUNK * J.CHUNK), 2 * unstuffed
            coef = (_p(bufs.coef), count, imgs, host, n)
            tabs = (ctypes.c_void_p(db + codes_off), 1, ctypes.c_void_p(db), ctypes.c_void_p(hb))
            sp = (ctypes.c_void_p(db + spans_off), ctypes.c_void_p(hb + spans_off))
            res = compare([("count", lambda: _call("vunet_jpeg_huff_count", *coef, _p(ent.hist), 1024 * n, _stream())),
                           ("lengths", lambda: _call("vunet_jpeg_huff_lengths", *coef, *tabs, _p(ent.bits), blocks, _p(ent.small), start_at, _stream())),
                           ("pack", lambda: _call("vunet_jpeg_huff_pack", *coef, *tabs, _p(ent.bits), blocks, *sp, _p(ent.raw), raw_bytes, _stream())),
                           ("stuff", lambda: _call("vunet_jpeg_huff_stuff", _p(ent.raw), raw_bytes, host, *sp, n, _p(ent.chunks), raw_bytes // J.CHUNK,
                                                   _p(ent.out), out_cap, ctypes.c_void_p(ent.small.data_ptr() + 4 * start_at), _stream()))],
                          a.calls, a.rounds)
            names = {"count": "vunet_jpeg_huff_count (zero, histogram)", "lengths": "vunet_jpeg_huff_lengths (zero, lengths, prefix sum)",
                     "pack": "vunet_jpeg_huff_pack (zero, pack)", "stuff": "vunet_jpeg_huff_stuff (count, prefix sum, write)"}
            for k, r in res.items():
                row("launches", f"quality {q}: {names[k]}", r, "us")
            torch.cuda.synchronize()
            assert J.encode_batch(dev, quality=q, subsampling="4:2:0", entropy="device") == streams       # (the buffers are as a call leaves them)
            down = min(out_cap, unstuffed + unstuffed // 16 + 4096) + 4 * (n + 1)
            lines.append(f"# quality {q}: the device route's final download: {down} bytes ({down / 1e6:.2f} MB; the scans are "
                         f"{sum(len(t) - t.index(bytes([0xFF, 0xDA])) - 16 for t in streams)} of them) against {2 * count} bytes of coefficients ({2 * count / 1e6:.1f} MB) on the host route")
            print(lines[-1], flush=True)
            routes = [(f"{entropy}{', optimize' if opt else ''}", (lambda e=entropy, o=opt: J.encode_batch(dev, quality=q, subsampling="4:2:0",
                                                                                                        entropy=e, optimize=o)))
                      for entropy in ("host", "device") for opt in (False, True)]
            for k, r in wall_alternating(routes, a.rounds).items():
                row("encode_batch, alternating", f"quality {q}: entropy={k} (8 threads on the host route)", r, "ms")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
