"""Baseline JPEG encode of device frames: the uint8 stacks every video call of ``render`` ends in -> JFIF byte streams.  What the
reference does per frame on the host -- ``cv2.imwrite`` / the frames of ``cv2.VideoWriter`` (lib/logging.py, lib/figures.py,
data/*.py) -- is split here where the work changes character, the mirror image of ``jpeg_decode`` (csrc/jpeg_enc.hip,
csrc/jpeg_huff_enc.h, include/vunet_jpeg_enc.h):

* colour conversion, chroma down-sampling, the forward DCT and the quantiser are two HIP launches for the whole batch, whatever the
  images' sizes, after ONE small upload (descriptors and tables), and ONE download of the quantised coefficients into a reused
  pinned buffer;
* the entropy coder, a serial bit walk, runs on the host by default: the library's C++ on the codec's small thread pool
  (``jpeg_host.per_image``; ctypes releases the GIL);
* ``entropy="device"`` keeps it on the GPU (csrc/jpeg_huff.hip): per block its bit count, a prefix sum per image, every block's
  bits packed at its offset, the bytes stuffed -- one launch per stage, two host waits -- and ONLY the scans' bytes are downloaded;
  the host writes the header and ``FF D9`` around them.  Same bytes as the host route;
* ``optimize=True`` is Pillow's: Huffman tables built from the image's own symbol counts (libjpeg's ``jpeg_gen_optimal_table``),
  a second pass over the coefficients on the host route, a histogram launch and one more round trip (histograms down, tables up)
  on the device route.  The streams carry their tables: every decoder reads them.

The bytes are Pillow's ``Image.save(.., "JPEG", quality=q, subsampling=s)`` (libjpeg-turbo's defaults: the "islow" integer forward
DCT, the Annex K tables), pinned against Pillow 12.2.0 by tests/golden/g24_jpeg_encode.npz, and with ``optimize=True`` Pillow's
``optimize=True`` bytes (tests/golden/g25_jpeg_optimize.npz).  ASSUMED, NOT PINNED: ``cv2.imwrite``
writes with other defaults (quality 95, 4:2:0) -- ``quality=95`` mimics it -- and OpenCV is no dependency of this package.

* ``encode_batch``  frames -> ``list[bytes]``;
* ``save_images``   a thin loop over it: one ``.jpg`` per frame;
* ``JpegEncodeError``  carries the C error code.

Not done: progressive mode, restart markers.  There is no CPU path."""
from __future__ import annotations

import ctypes
import functools
from collections import namedtuple
from typing import Dict, List

import numpy as np
import torch

from . import _lib, jpeg_host
from .jpeg_host import MAX_SIDE, MAX_THREADS, Arena, JpegImg, JpegInfoC, fill_rows, frame_paths, layout, per_image
from .ops import _call, _p, _stream

SUBSAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}
ENTROPY = ("host", "device")
CHUNK = 1024                        # the device coder's unstuffed scans start at multiples of it (csrc/jpeg_huff_enc.h kStuffChunk)
BLOCK_BITS = 1664                   # no block codes to more: 26 bits per coefficient
ERR_CAPACITY = _lib.const("VUNET_JPEG_ERR_CAPACITY")
ERR_RANGE, ERR_ARG = _lib.const("VUNET_JPEG_ERR_RANGE"), _lib.const("VUNET_ERR_ARG")
REASONS = {ERR_CAPACITY: "the stream is longer than its output buffer",
           ERR_RANGE: "a coefficient outside baseline's range (DC difference > 11 bits or AC > 10 bits)",
           ERR_ARG: "an argument the library refuses"}


class JpegEncodeError(jpeg_host._CodecError):
    """``code``: the library's value; ``index``: the frame's place in the batch."""
    REASONS, WHAT = REASONS, "frame"


_device = functools.partial(jpeg_host.device, "encode_batch")     # (a module attribute: the CPU tests replace it)
# by (device, stream): the pinned descriptor / table block ``stage`` and its device mirror ``dev``, the component planes and the
# coefficients on the device, the pinned coefficients ``coef_host`` and the streams' bytes ``out`` on the host
_buffers: Dict[tuple, Arena] = {}
# The device coder's arena, ``buf.entropy``.  ``up`` / ``up_dev``: the pinned block of what goes up and its device mirror -- tab_row
# int32 [N] | spans int64 [N][2] | codes uint32 [rows][4][256].  ``small`` / ``small_host``: uint32 totals [r4(N)] | status [r4(2 N)] |
# img_start [N + 1].  ``bits``: one word per block.  ``hist``: [N][4][256] with ``optimize``.  ``raw``: the unstuffed scans,
# ``chunks`` one word per 1024 bytes of them, ``out`` / ``out_host`` the stuffed scans.
_ENTROPY = "up up_dev small small_host bits hist hist_host raw chunks out out_host"
# what one call hands its device steps.  ``steps``: the arguments of ``_transform`` and ``_launch`` behind the frames -- images,
# channels, the upload's bytes, where its tables lie and how many entries they have, the coefficients of the batch; for the device
# coder the infos, each image's host table pointer and ``optimize``
_Plan = namedtuple("_Plan", "steps infos qptrs optimize")


def _entropy_layout(n: int, rows: int):
    """-> (spans_off, codes_off, up_bytes) of ``up``, in bytes; (status_at, start_at, words) of ``small``, in words."""
    up, up_bytes = layout(("tab_row", 4 * n, 1), ("spans", 16 * n, 16), ("codes", 4096 * rows, 1))
    small, words = layout(("totals", n, 1), ("status", 2 * n, 4), ("img_start", n + 1, 4))
    return (up["spans"], up["codes"], up_bytes), (small["status"], small["img_start"], words)


def clear_buffers() -> None:
    """Drop the cached buffers."""
    _buffers.clear()


def quant_tables(quality: int) -> np.ndarray:
    """uint16 [2, 64], natural order: the Annex K tables at libjpeg's ``quality`` (1 .. 100), luma then chroma.  Host only."""
    q = np.empty((2, 64), dtype=np.uint16)
    _call("vunet_jpeg_quant_tables", int(quality), q.ctypes.data)
    return q


def _transform(buf: Arena, frames: torch.Tensor, m: int, channels: int, up_bytes: int, q_off: int, q_count: int, coef_count: int) -> None:
    """One upload of the descriptors and tables and the two launches, on the current stream, not waited for.  The host copy of the
    descriptors is what the library checks before it launches."""
    n, hmax, wmax = (int(v) for v in frames.shape[:3])
    buf.upload(up_bytes)
    base = buf.dev.data_ptr()
    imgs, qtab, host = ctypes.c_void_p(base), ctypes.c_void_p(base + q_off), ctypes.c_void_p(buf.stage.data_ptr())
    _call("vunet_jpeg_from_rgb", _p(frames), n, hmax, wmax, channels, imgs, host, m, _p(buf.planes), coef_count, _stream())
    _call("vunet_jpeg_fdct", _p(buf.planes), coef_count, qtab, q_count, imgs, host, m, _p(buf.coef), coef_count, _stream())


def _wait(buf: Arena) -> None:
    buf.record()
    buf.wait()


def _launch(buf: Arena, frames: torch.Tensor, m: int, channels: int, up_bytes: int, q_off: int, q_count: int, coef_count: int) -> None:
    """The host route's device step: ``_transform`` and the download of the coefficients into the pinned buffer, waited for."""
    _transform(buf, frames, m, channels, up_bytes, q_off, q_count, coef_count)
    buf.coef_host[:coef_count].copy_(buf.coef[:coef_count], non_blocking=True)
    _wait(buf)


def _optimal_tables(lib, hist: np.ndarray, ntab: int):
    """``hist`` uint32 [4, 256] -> (rc, counts uint8 [4, 16], symbols uint8 [4, 256]): the first ``ntab`` tables built, the rest empty."""
    counts, symbols, nsym = np.zeros((4, 16), dtype=np.uint8), np.zeros((4, 256), dtype=np.uint8), ctypes.c_int32(0)
    for t in range(ntab):
        rc = lib.vunet_jpeg_optimal_table(hist[t].ctypes.data, counts[t].ctypes.data, symbols[t].ctypes.data, ctypes.byref(nsym))
        if rc != 0:
            return rc, counts, symbols
    return 0, counts, symbols


def _encode_on_device(buf: Arena, frames: torch.Tensor, plan: _Plan) -> List[bytes]:
    """The device route behind ``_transform``: [histograms, a wait, tables up;] lengths and their prefix sums, a wait for the bit
    totals, the spans up, pack and stuff, one wait for the scans' lengths and bytes.  The host writes header and EOI around them."""
    (n, channels, _, _, _, coef_count), infos, qptrs, optimize = plan
    lib, stream = _lib.lib(), _stream()
    if any(i.nblocks * BLOCK_BITS >= 1 << 32 for i in infos):
        j = next(j for j, i in enumerate(infos) if i.nblocks * BLOCK_BITS >= 1 << 32)
        raise ValueError(f"frame {j}: {infos[j].nblocks} blocks may code to more bits than the device coder's 32-bit offsets count; "
                         f"use entropy=\"host\"")
    ent = buf.entropy
    if ent is None:
        ent = buf.entropy = Arena(buf.device, _ENTROPY)
    rows, blocks, ntab = (n if optimize else 1), sum(i.nblocks for i in infos), (4 if channels == 3 else 2)
    ent.layout = (spans_off, codes_off, tab_bytes), (status_at, start_at, small_words) = _entropy_layout(n, rows)
    ent.get("up", tab_bytes, torch.uint8, "pinned")
    ent.get("up_dev", tab_bytes, torch.uint8)
    ent.get("small", small_words, torch.int32)
    ent.get("small_host", small_words, torch.int32, "pinned")
    ent.get("bits", blocks, torch.int32)
    if optimize:
        ent.get("hist", 1024 * n, torch.int32)
        ent.get("hist_host", 1024 * n, torch.int32, "pinned")
    _transform(buf, frames, *plan.steps)
    up = ent.up.numpy()
    tab_row, spans = up[:4 * n].view(np.int32), up[spans_off:spans_off + 16 * n].view(np.int64).reshape(n, 2)
    hbase, dbase = ent.up.data_ptr(), ent.up_dev.data_ptr()
    imgs, imgs_host, coef = ctypes.c_void_p(buf.dev.data_ptr()), ctypes.c_void_p(buf.stage.data_ptr()), _p(buf.coef)
    counts = symbols = None
    if optimize:
        _call("vunet_jpeg_huff_count", coef, coef_count, imgs, imgs_host, n, _p(ent.hist), 1024 * n, stream)
        ent.hist_host[:1024 * n].copy_(ent.hist[:1024 * n], non_blocking=True)
        _wait(buf)
        hist = ent.hist_host.numpy()[:1024 * n].view(np.uint32).reshape(n, 4, 256)
        counts, symbols = np.empty((n, 4, 16), dtype=np.uint8), np.empty((n, 4, 256), dtype=np.uint8)
        failed = ctypes.c_int32(-1)
        rc = lib.vunet_jpeg_optimal_tables(hist.ctypes.data, n, ntab, counts.ctypes.data, symbols.ctypes.data, hbase + codes_off,
                                           ctypes.byref(failed))
        if rc != 0:
            raise JpegEncodeError(rc, failed.value)
        tab_row[:] = np.arange(n)
    else:
        _call("vunet_jpeg_code_words", None, None, hbase + codes_off)
        tab_row[:] = 0
    spans[:] = 0
    ent.up_dev[:tab_bytes].copy_(ent.up[:tab_bytes], non_blocking=True)
    codes, rows_dev, rows_host = ctypes.c_void_p(dbase + codes_off), ctypes.c_void_p(dbase), ctypes.c_void_p(hbase)
    _call("vunet_jpeg_huff_lengths", coef, coef_count, imgs, imgs_host, n, codes, rows, rows_dev, rows_host, _p(ent.bits), blocks,
          _p(ent.small), start_at, stream)
    ent.small_host[:start_at].copy_(ent.small[:start_at], non_blocking=True)
    _wait(buf)
    small = ent.small_host.numpy().view(np.uint32)
    status = small[status_at:status_at + 2 * n].reshape(n, 2)
    if status.any():                                        # the lowest failing index
        j = int(np.flatnonzero(status.any(axis=1))[0])
        raise JpegEncodeError(ERR_RANGE if status[j, 0] else ERR_ARG, j)
    nbytes = (small[:n].astype(np.int64) + 7) // 8
    padded = (nbytes + CHUNK - 1) // CHUNK * CHUNK
    spans[:, 0], spans[:, 1] = np.cumsum(padded) - padded, small[:n]
    raw_bytes, out_cap, unstuffed = int(padded.sum()), int(2 * nbytes.sum()), int(nbytes.sum())
    if out_cap >= 1 << 32:
        raise ValueError(f"encode_batch: the batch's scans ({unstuffed} bytes before stuffing) pass the device coder's 32-bit offsets; "
                         f"use smaller batches or entropy=\"host\"")
    ent.get("raw", raw_bytes, torch.uint8)
    ent.get("chunks", raw_bytes // CHUNK, torch.int32)
    ent.get("out", out_cap, torch.uint8)
    ent.get("out_host", out_cap, torch.uint8, "pinned")
    ent.up_dev[spans_off:codes_off].copy_(ent.up[spans_off:codes_off], non_blocking=True)
    spans_dev, spans_host = ctypes.c_void_p(dbase + spans_off), ctypes.c_void_p(hbase + spans_off)
    _call("vunet_jpeg_huff_pack", coef, coef_count, imgs, imgs_host, n, codes, rows, rows_dev, rows_host, _p(ent.bits), blocks,
          spans_dev, spans_host, _p(ent.raw), raw_bytes, stream)
    _call("vunet_jpeg_huff_stuff", _p(ent.raw), raw_bytes, imgs_host, spans_dev, spans_host, n, _p(ent.chunks), raw_bytes // CHUNK,
          _p(ent.out), out_cap, ctypes.c_void_p(ent.small.data_ptr() + 4 * start_at), stream)
    # stuffing adds a byte per 0xFF, 1 in 256 of random bits: a sixteenth more than the unstuffed bytes comes down with the lengths,
    # and the rest of a batch that needs more (saturated coefficients) in a second copy
    first = min(out_cap, unstuffed + unstuffed // 16 + 4096)
    ent.small_host[start_at:small_words].copy_(ent.small[start_at:small_words], non_blocking=True)
    ent.out_host[:first].copy_(ent.out[:first], non_blocking=True)
    _wait(buf)
    starts = ent.small_host.numpy().view(np.uint32)[start_at:small_words].astype(np.int64)
    if starts[n] > first:
        ent.out_host[first:int(starts[n])].copy_(ent.out[first:int(starts[n])], non_blocking=True)
        _wait(buf)
    scans, header, length, res = ent.out_host.numpy(), np.empty(1024, dtype=np.uint8), ctypes.c_int64(0), []
    for j in range(n):
        c, s = (counts[j].ctypes.data, symbols[j].ctypes.data) if optimize else (None, None)
        rc = lib.vunet_jpeg_write_header(ctypes.byref(infos[j]), ctypes.c_void_p(qptrs[j]), c, s, header.ctypes.data, header.size,
                                         ctypes.byref(length))
        if rc != 0:
            raise JpegEncodeError(rc, j)
        res.append(header[:length.value].tobytes() + scans[starts[j]:starts[j + 1]].tobytes() + b"\xff\xd9")
    return res


def _code_with_retry(code, dst: int, cap: int):
    """``code(dst, cap, length)`` codes one stream into the ``cap`` bytes at the host address ``dst``; one that is longer (the
    capacity code) is coded again into a buffer of the length the first call asked for.  -> (code, the stream's bytes)"""
    length = ctypes.c_int64(0)
    rc = code(ctypes.c_void_p(dst), cap, ctypes.byref(length))
    if rc == ERR_CAPACITY:
        own = np.empty(length.value, dtype=np.uint8)
        rc = code(ctypes.c_void_p(own.ctypes.data), own.size, ctypes.byref(length))
        return rc, own.tobytes()
    return rc, ctypes.string_at(dst, length.value)


def _sizes(sizes, n: int, h: int, w: int) -> List[tuple]:
    if sizes is None:
        return [(h, w)] * n
    sizes = [(int(a), int(b)) for a, b in (sizes.tolist() if hasattr(sizes, "tolist") else sizes)]
    if len(sizes) != n or any(not (1 <= a <= h and 1 <= b <= w) for a, b in sizes):
        raise ValueError(f"sizes: {n} pairs (h, w) with 1 <= h <= {h} and 1 <= w <= {w} expected, got {sizes}")
    return sizes


def _per_image(value, n: int, what: str) -> list:
    values = list(value) if isinstance(value, (list, tuple)) else [value] * n
    if len(values) != n:
        raise ValueError(f"{what}: one value or one per image ({n}) expected, got {len(values)}")
    return values


def encode_batch(frames: torch.Tensor, quality=75, subsampling="4:2:0", sizes=None, threads: int = 8, entropy: str = "host",
                 optimize: bool = False) -> List[bytes]:
    """``frames`` uint8 [N, H, W, 3] (RGB interleaved) or [N, H, W] (gray) on the current GPU -> N baseline JPEG streams, image n
    byte for byte ``Image.fromarray(frames[n, :h, :w]).save(.., "JPEG", quality=quality, subsampling=subsampling)``.

    ``quality``: libjpeg's 1 .. 100.  ``subsampling``: "4:4:4", "4:2:2" or "4:2:0" (ignored for gray).  Either may be a list with one
    value per image: the two launches take mixed samplings and tables as they take mixed sizes.  ``sizes``: per-image
    ``(h, w)`` inside the padded stack, as ``decode_batch`` returns them (default: every image fills it).  ``threads``: host threads
    of the entropy coder, at most 16.  ``entropy``: "host" or "device", where the Huffman coder runs; the bytes are the same, and
    with "device" ``threads`` has no effect and only the scans' bytes are downloaded (two host waits; an image of more blocks than
    32-bit bit offsets cover, about 2.5 million, is refused with a ``ValueError``).  ``optimize``: Pillow's ``optimize=True`` --
    per-image Huffman tables from the image's own symbol counts, written into the stream's DHT segments; smaller streams for a second
    pass over the coefficients (host) or a histogram launch and one more round trip (device).

    One small upload, two launches, one download of the coefficients into a reused pinned buffer on the current stream, a wait for
    it, then the entropy coder on the host.  After the first call at a shape nothing is allocated on the device.  Not recordable
    into a hipGraph as a whole (the host half would not be replayed); the two launches are."""
    if not torch.is_tensor(frames) or frames.dtype != torch.uint8 or not (frames.dim() == 3 or (frames.dim() == 4 and frames.shape[3] == 3)):
        raise ValueError(f"frames: uint8 [N, H, W, 3] or [N, H, W] expected, got {getattr(frames, 'dtype', type(frames))} "
                         f"{tuple(getattr(frames, 'shape', ()))}")
    n, h, w = (int(v) for v in frames.shape[:3])
    quality, subsampling = _per_image(quality, n, "quality"), _per_image(subsampling, n, "subsampling")
    if any(s not in SUBSAMPLING for s in subsampling):
        raise ValueError(f"subsampling: one of {sorted(SUBSAMPLING)} expected, got {sorted(set(subsampling))}")
    if any(not isinstance(q, (int, np.integer)) or not 1 <= q <= 100 for q in quality):
        raise ValueError(f"quality: integers 1 .. 100 expected, got {sorted(set(quality), key=str)}")
    if entropy not in ENTROPY:
        raise ValueError(f"entropy: one of {ENTROPY} expected, got {entropy!r}")
    threads, optimize = int(threads), bool(optimize)
    if not 1 <= threads <= MAX_THREADS:
        raise ValueError(f"encode_batch: 1 <= threads <= {MAX_THREADS} expected, got {threads}")
    if not (1 <= n <= MAX_SIDE and 1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f"encode_batch: 1 <= N, H, W <= {MAX_SIDE} expected, got {n}, {h}, {w}")
    device = _device()
    if frames.device != device:
        raise ValueError(f"frames: a tensor on {device} expected, got {frames.device}")
    frames = frames if frames.is_contiguous() else frames.contiguous()
    channels = 3 if frames.dim() == 4 else 1
    sizes = _sizes(sizes, n, h, w)
    lib = _lib.lib()
    infos = []
    for (a, b), s in zip(sizes, subsampling):
        info = JpegInfoC()
        _call("vunet_jpeg_encode_info", a, b, channels, *(SUBSAMPLING[s] if channels == 3 else (1, 1)), ctypes.byref(info))
        infos.append(info)
    key = (str(device), _stream().value if device.type == "cuda" else 0)
    buf = _buffers.get(key)
    if buf is None:
        buf = _buffers[key] = Arena(device, "planes coef coef_host out")
    q_off = n * ctypes.sizeof(JpegImg)
    levels = sorted(set(int(q) for q in quality))     # one [3][64] table block per distinct quality
    tables = np.concatenate([quant_tables(q)[[0, 1, 1]] for q in levels])
    table_of = [192 * levels.index(int(q)) for q in quality]
    up_bytes = q_off + tables.nbytes
    caps = [1024 + 2 * i.ncoef for i in infos]        # two bytes per coefficient (0/255 noise at quality 100 takes 1.6); a longer one: below
    coef_count = sum(i.ncoef for i in infos)
    buf.staging(up_bytes)
    buf.get("planes", coef_count, torch.uint8)
    buf.get("coef", coef_count, torch.int16)
    buf.get("coef_host", coef_count, torch.int16, "pinned")
    buf.get("out", sum(caps), torch.uint8, "host")
    base = buf.stage.data_ptr()
    rows = (JpegImg * n).from_address(base)
    qbase = tables.ctypes.data
    ctypes.memmove(base + q_off, qbase, tables.nbytes)
    fill_rows(rows, infos, table_of, range(n))
    qptrs = [qbase + 2 * t for t in table_of]
    steps = (n, channels, up_bytes, q_off, tables.size, coef_count)
    if entropy == "device":
        return _encode_on_device(buf, frames, _Plan(steps, infos, qptrs, optimize))
    _launch(buf, frames, *steps)
    cbase, obase, ntab = buf.coef_host.data_ptr(), buf.out.data_ptr(), (4 if channels == 3 else 2)
    coffs, offs = [2 * r.coef_off for r in rows], np.concatenate([[0], np.cumsum(caps)]).tolist()

    def one(j):
        cptr, info, qptr = ctypes.c_void_p(cbase + coffs[j]), ctypes.byref(infos[j]), ctypes.c_void_p(qptrs[j])
        if not optimize:
            return _code_with_retry(lambda *dst: lib.vunet_jpeg_entropy_encode(cptr, info, qptr, *dst), obase + offs[j], caps[j])
        hist = np.empty((4, 256), dtype=np.uint32)        # two passes over the pinned coefficients: count, then code
        rc = lib.vunet_jpeg_symbol_histogram(cptr, info, hist.ctypes.data)
        if rc == 0:
            rc, counts, symbols = _optimal_tables(lib, hist, ntab)
        if rc != 0:
            return rc, b""
        return _code_with_retry(lambda *dst: lib.vunet_jpeg_entropy_encode_tables(cptr, info, qptr, counts.ctypes.data, symbols.ctypes.data, *dst),
                                obase + offs[j], caps[j])
    res = per_image(one, range(n), threads)
    for j, (rc, _) in enumerate(res):
        if rc != 0:
            raise JpegEncodeError(rc, j)
    return [data for _, data in res]


def save_images(pattern: str, frames: torch.Tensor, quality: int = 75, subsampling: str = "4:2:0", sizes=None, start: int = 0,
                threads: int = 8, entropy: str = "host", optimize: bool = False) -> List[str]:
    """``encode_batch`` and one file per frame: ``pattern % index`` (``"img_%06d.jpg"``, the reference's frame names) or
    ``pattern.format(index)``, indices from ``start``.  -> the paths written."""
    streams = encode_batch(frames, quality, subsampling, sizes, threads, entropy, optimize)
    paths = frame_paths(pattern, len(streams), start)
    for path, data in zip(paths, streams):
        with open(path, "wb") as f:
            f.write(data)
    return paths
