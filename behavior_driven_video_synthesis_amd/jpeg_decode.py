"""Baseline JPEG decode for the raw-frame input route: encoded byte streams in, the uint8 RGB stack ``[N, Hmax, Wmax, 3]`` of
``image_input.frames_to_images`` out, on the GPU.  What the reference does per frame on the host -- ``cv2.imread`` of every
``img_%06d.jpg`` (data/base_dataset.py) -- is split here where the work changes character (csrc/jpeg_entropy.h, csrc/jpeg.hip,
include/vunet_jpeg.h):

* the entropy decode, a serial bit walk, runs on the host by default: the library's C++ on a small thread pool (ctypes releases
  the GIL), straight into one reused pinned buffer.  ``entropy="device"`` runs it on the GPU as well, by self-synchronising walks
  over subsequences of ``VUNET_JPEG_SUBSEQ_BYTES`` (csrc/jpeg_sync.h, csrc/jpeg_huff_dec.hip, include/vunet_jpeg_huffdec.h); the stream bytes go up instead;
* everything after it -- dequantisation, the inverse DCT, chroma up-sampling, YCbCr -> RGB -- is two HIP launches for the whole
  batch, whatever the images' sizes and samplings, after ONE upload (descriptors, tables and coefficients in one piece).

The bytes are Pillow's (libjpeg-turbo's defaults: the "islow" integer inverse DCT, "fancy" up-sampling), pinned against Pillow
12.2.0 by tests/golden/g23_jpeg.npz.  ASSUMED, NOT PINNED: that ``cv2.imread`` decodes with the same libjpeg-turbo defaults
(OpenCV is no dependency of this package and is absent where the fixtures are written).  EXIF orientation is ignored, as Pillow's
``Image.open`` ignores it and as ffmpeg-written frames need.  A grayscale stream gives R = G = B = Y, ``cv2.imread``'s default.

* ``parse``         the header of one stream -> ``JpegInfo`` (host only, no GPU);
* ``decode_batch``  streams -> ``(frames uint8 [N, Hmax, Wmax, 3] on the device, hw int32 [N, 2] on the host)``;
* ``JpegUnsupported`` / ``JpegCorrupt``  carry the C error code and its reason.

What this module shares with ``jpeg_encode`` -- the descriptor table, the reused memory, the upload layouts, the thread pool -- is
``jpeg_host``.

Supported: baseline sequential, 8-bit, 1 or 3 components, 4:4:4 / 4:2:2 / 4:2:0, one interleaved scan, restart intervals.
Progressive, arithmetic-coded, 12-bit and CMYK streams are refused (``fallback=True`` hands them to Pillow on the host where PIL
imports).  There is no CPU path for the supported ones."""
from __future__ import annotations

import ctypes
import functools
import io
from collections import namedtuple
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib, jpeg_host
from .jpeg_host import MAX_SIDE, MAX_THREADS, Arena, JpegImg, JpegInfoC, fill_rows, layout, per_image
from .ops import _call, _p, _stream

REASONS = {_lib.const("VUNET_JPEG_ERR_TRUNCATED"): "the stream ends inside a segment, a table or the scan, or before EOI",
           _lib.const("VUNET_JPEG_ERR_MARKER"): "no SOI, a marker out of place, a malformed segment or a missing table",
           _lib.const("VUNET_JPEG_ERR_HUFFMAN"): "a Huffman code that is in no table, or a coefficient index past 63",
           _lib.const("VUNET_JPEG_ERR_RESTART"): "a restart marker is missing or out of sequence",
           _lib.const("VUNET_JPEG_ERR_SOF"): "progressive, extended, lossless or arithmetic-coded frame (only SOF0 is decoded)",
           _lib.const("VUNET_JPEG_ERR_PRECISION"): "16-bit quantisation tables or samples that are not 8-bit",
           _lib.const("VUNET_JPEG_ERR_COMPONENTS"): "4 components (CMYK / YCCK), an Adobe transform other than YCbCr, or RGB components",
           _lib.const("VUNET_JPEG_ERR_SAMPLING"): "sampling other than 4:4:4, 4:2:2 or 4:2:0",
           _lib.const("VUNET_JPEG_ERR_SCANS"): "more than one scan"}
_UNSUPPORTED = range(-119, -109)         # VUNET_JPEG_ERR_*: -110 .. -119 unsupported, -100 .. -109 corrupt

JpegInfo = namedtuple("JpegInfo", "height width ncomp hsamp vsamp mcu_cols mcu_rows restart bw0 bh0 bw1 bh1 nblocks ncoef")


class JpegError(jpeg_host._CodecError):
    """``code``: the library's VUNET_JPEG_ERR_* value; ``reason``: what it says; ``index``: the stream's place in the batch."""
    REASONS, WHAT = REASONS, "stream"


class JpegUnsupported(JpegError):
    """A well-formed stream outside the supported subset."""


class JpegCorrupt(JpegError):
    """A truncated or malformed stream."""


def _error(code: int, index: Optional[int] = None) -> JpegError:
    return (JpegUnsupported if code in _UNSUPPORTED else JpegCorrupt)(code, index)


def _bytes(data, index: Optional[int] = None) -> bytes:
    if isinstance(data, (bytearray, memoryview)):
        data = bytes(data)
    if not isinstance(data, bytes):
        where = "" if index is None else f"stream {index}: "
        raise TypeError(f"{where}bytes expected, got {type(data).__name__}")
    return data


def _parse_c(data: bytes, index: Optional[int] = None):
    info = JpegInfoC()
    rc = _lib.lib().vunet_jpeg_parse(data, len(data), ctypes.byref(info))
    if rc != 0:
        raise _error(rc, index)
    return info


def parse(data) -> JpegInfo:
    """The header of one stream (host only): sizes, component count, the first component's sampling, the MCU grid, the block grids
    and the coefficient count.  Raises ``JpegUnsupported`` / ``JpegCorrupt``."""
    info = _parse_c(_bytes(data))
    return JpegInfo(*(getattr(info, f) for f in JpegInfo._fields))


_device = functools.partial(jpeg_host.device, "decode_batch")     # (a module attribute: the CPU tests replace it)
_buffers: Dict[tuple, Arena] = {}        # by (device, stream, tag): ``stage`` / ``dev`` / ``planes``, the default output stacks ``outs``


def clear_buffers() -> None:
    """Drop the cached buffers (not while frames returned without ``out=`` are still in use)."""
    _buffers.clear()


def _pillow_rgb(data: bytes, index: int, err: JpegError) -> np.ndarray:
    try:
        from PIL import Image
    except ImportError:
        raise err from None
    return np.array(Image.open(io.BytesIO(data)).convert("RGB"))   # (a writable copy)


def _finish(buf: Arena, coef, coef_count: int, q_off: int, m: int, plane_bytes: int, out: torch.Tensor) -> None:
    """What every route ends in, two launches on the current stream: the coefficients at the device pointer ``coef`` -> the planes
    -> ``out``, by the descriptors and tables of the uploaded block.  The host copy of the descriptors is what the library checks
    before it launches."""
    n, hmax, wmax = (int(v) for v in out.shape[:3])
    base, host, stream = buf.dev.data_ptr(), ctypes.c_void_p(buf.stage.data_ptr()), _stream()
    imgs, qtab = ctypes.c_void_p(base), ctypes.c_void_p(base + q_off)
    _call("vunet_jpeg_idct", coef, coef_count, qtab, m * 192, imgs, host, m, _p(buf.planes), plane_bytes, stream)
    _call("vunet_jpeg_to_rgb", _p(buf.planes), plane_bytes, imgs, host, m, n, hmax, wmax, _p(out), stream)


_HostPlan = namedtuple("_HostPlan", "m nbytes q_off c_off coef_count plane_bytes")     # (the arguments of ``_launch`` behind ``buf``)


def _host_plan(m: int, coef_count: int) -> _HostPlan:
    """The host route's upload: descriptors | quantisation tables | coefficients, these on a 128-byte line."""
    offs, nbytes = layout(("imgs", m * ctypes.sizeof(JpegImg), 1), ("qtab", 384 * m, 1), ("coef", 2 * coef_count, 128))
    return _HostPlan(m, nbytes, offs["qtab"], offs["coef"], coef_count, max(coef_count, 16))


def _launch(buf: Arena, m: int, nbytes: int, q_off: int, c_off: int, coef_count: int, plane_bytes: int, out: torch.Tensor) -> None:
    """The host route's device step: one upload of the staging buffer's first ``nbytes`` (descriptors | tables | coefficients) and
    the two launches."""
    buf.upload(nbytes)
    _finish(buf, ctypes.c_void_p(buf.dev.data_ptr() + c_off), coef_count, q_off, m, plane_bytes, out)


def _decode_host(buf: Arena, data, infos, native, threads: int, out: torch.Tensor) -> None:
    """The host route of ``decode_batch`` for the streams ``native``: the entropy decode of every stream on the thread pool, straight
    into the pinned staging buffer, then ``_launch``."""
    own = [infos[i] for i in native]
    plan = buf.layout = _host_plan(len(native), sum(inf.ncoef for inf in own))
    buf.staging(plan.nbytes)
    buf.get("planes", plan.plane_bytes, torch.uint8)
    base = buf.stage.data_ptr()
    rows = (JpegImg * plan.m).from_address(base)
    fill_rows(rows, own, range(0, 192 * plan.m, 192), native)
    fn, coef_offs = _lib.lib().vunet_jpeg_entropy_decode, [r.coef_off for r in rows]

    def one(j):
        d = data[native[j]]
        return fn(d, len(d), ctypes.byref(own[j]), ctypes.c_void_p(base + plan.c_off + 2 * coef_offs[j]), ctypes.c_void_p(base + plan.q_off + 384 * j))
    for i, rc in zip(native, per_image(one, range(plan.m), threads)):
        if rc != 0:
            raise _error(rc, i)
    _launch(buf, *plan, out)


Subseq = _lib.struct("vunet_jpeg_subseq")
SUBSEQ_BYTES, GROUP = _lib.const("VUNET_JPEG_SUBSEQ_BYTES"), _lib.const("VUNET_JPEG_HUFFDEC_GROUP")
TAB_BYTES, STATE_WORDS = _lib.const("VUNET_JPEG_HUFFDEC_TAB_BYTES"), _lib.const("VUNET_JPEG_HUFFDEC_STATE_WORDS")
MAX_SCAN_BYTES, IRREGULAR = _lib.const("VUNET_JPEG_HUFFDEC_MAX_BYTES"), _lib.const("VUNET_JPEG_HUFFDEC_IRREGULAR")
SYNC_BATCH = 4                           # sync launches per readback of the convergence counters
_stats = dict(rounds=0, launches=0, subsequences=0, host_fallbacks=0)


def last_stats() -> dict:
    """What the last ``decode_batch(.., entropy="device")`` did: ``rounds`` (sync launches up to and including the first in which no
    state changed), ``launches`` (sync launches issued: a multiple of ``SYNC_BATCH`` or the bound), ``subsequences`` (threads of the
    walk, padding excluded) and ``host_fallbacks`` (streams decoded by the host walk instead: irregular marker layout, or flagged
    by the device -- zero for clean streams)."""
    return dict(_stats)


def _scan(lib, d: bytes, inf):
    """The marker scan of one stream -> (code, segments int64 [nseg, 3], qtab + table row as one uint8 array)."""
    mcus = inf.mcu_cols * inf.mcu_rows
    expected = -(-mcus // inf.restart) if inf.restart > 0 else 1
    segs, nseg, tabs = np.empty((expected, 3), dtype=np.int64), ctypes.c_int64(0), np.empty(384 + TAB_BYTES, dtype=np.uint8)
    rc = lib.vunet_jpeg_scan_segments(d, len(d), ctypes.byref(inf), segs.ctypes.data, expected, ctypes.byref(nseg), tabs.ctypes.data,
                                      tabs.ctypes.data + 384)
    return rc, segs[:nseg.value], tabs


def _device_layout(m: int, nsub: int, nscan: int):
    """The device route's upload -> (offsets by name, bytes): descriptors | quantisation tables | table rows | spans | subsequence
    rows | scan bytes, and 16 bytes past their rounded end for the walk's last loads."""
    return layout(("imgs", m * ctypes.sizeof(JpegImg), 1), ("qtab", 384 * m, 1), ("tabs", m * TAB_BYTES, 16), ("spans", 8 * m, 1),
                  ("rows", nsub * ctypes.sizeof(Subseq), 16), ("bytes", nscan, 1), ("tail", 16, 16))


def _decode_device(buf: Arena, data, infos, native, threads: int, out: torch.Tensor) -> None:
    """The device route of ``decode_batch`` for the streams ``native`` (indices with a parsed header): marker scan on the host (no bit
    walk), ONE upload of descriptors | quantisation tables | table rows | spans | subsequence rows | scan bytes, the sync launches
    with a readback of their counters every ``SYNC_BATCH`` (the first wait), block ordinals, write and DC sums, a readback of the
    per-image flags (the second wait), the host walk for what was irregular or flagged, then ``_finish``."""
    lib, m = _lib.lib(), len(native)
    scans = per_image(lambda i: _scan(lib, data[i], infos[i]), native, threads)
    for i, (rc, _, _) in zip(native, scans):
        if rc < 0:
            raise _error(rc, i)
    # the layout of the upload; an irregular stream brings no rows and no bytes
    counts, offs, nsub, nscan, nthreads = [], [], 0, 0, 0
    for rc, segs, _ in scans:
        rows = 0 if rc else int(((segs[:, 1] - segs[:, 0] + SUBSEQ_BYTES - 1) // SUBSEQ_BYTES).sum())
        counts.append(jpeg_host.round_up(rows, GROUP))
        nthreads += rows
        offs.append(nscan - (int(segs[0, 0]) if rows else 0))
        nsub, nscan = nsub + counts[-1], nscan + (jpeg_host.round_up(int(segs[-1, 1] - segs[0, 0]), 16) if rows else 0)
    if nscan > MAX_SCAN_BYTES:
        raise ValueError(f'decode_batch: {nscan} bytes of scans in one call; entropy="device" takes at most {MAX_SCAN_BYTES} '
                         '(entropy="host" has no such limit)')
    buf.layout = offs_up, nbytes = _device_layout(m, nsub, nscan)
    q_off, t_off, s_off, r_off, b_off = (offs_up[k] for k in ("qtab", "tabs", "spans", "rows", "bytes"))
    own = [infos[i] for i in native]
    coef_count = sum(inf.ncoef for inf in own)
    plane_bytes = max(coef_count, 16)
    buf.staging(nbytes)
    buf.get("planes", plane_bytes, torch.uint8)
    if buf.entropy is None:               # coefficients, the walk's state, counters | flags and their pinned mirror; ``scratch``:
        buf.entropy = Arena(buf.device, "coef state small small_host scratch")   # pinned, for what the host walk decodes instead
    ent = buf.entropy
    bound = max(counts) // GROUP + 1
    ncounters = jpeg_host.round_up(bound, SYNC_BATCH)
    ent.get("coef", coef_count, torch.int16)
    ent.get("state", max(nsub * STATE_WORDS, 4), torch.int32)
    ent.get("small", ncounters + m, torch.int32)
    ent.get("small_host", ncounters + m, torch.int32, "pinned")
    ent.upload_bytes = nbytes                                          # (what tools/time_jpeg.py reports)
    base = buf.stage.data_ptr()
    stage = buf.stage.numpy()
    rows, spans = (JpegImg * m).from_address(base), stage[s_off:s_off + 8 * m].view(np.int32).reshape(m, 2)
    fill_rows(rows, own, range(0, 192 * m, 192), native)
    row_at = 0
    for j, i in enumerate(native):
        inf, (rc, segs, tabs) = own[j], scans[j]
        stage[q_off + 384 * j:q_off + 384 * (j + 1)] = tabs[:384]
        stage[t_off + TAB_BYTES * j:t_off + TAB_BYTES * (j + 1)] = tabs[384:]
        spans[j] = (row_at, counts[j])
        if counts[j]:
            made = ctypes.c_int64(0)
            rc = lib.vunet_jpeg_huffdec_rows(segs.ctypes.data, len(segs), ctypes.byref(inf), j, offs[j], row_at,
                                             base + r_off + row_at * ctypes.sizeof(Subseq), counts[j], ctypes.byref(made))
            if rc != 0 or made.value != counts[j]:
                raise RuntimeError(f"vunet_jpeg_huffdec_rows failed on stream {i} (code {rc})")
            lo, hi = int(segs[0, 0]), int(segs[-1, 1])
            stage[b_off + offs[j] + lo:b_off + offs[j] + hi] = np.frombuffer(data[i], dtype=np.uint8, count=hi - lo, offset=lo)
        row_at += counts[j]
    buf.upload(nbytes)
    dev, host, stream = buf.dev.data_ptr(), ctypes.c_void_p(base), _stream()
    at = lambda off: ctypes.c_void_p(dev + off)                       # noqa: E731
    at_host = lambda off: ctypes.c_void_p(base + off)                 # noqa: E731
    small = ent.small.data_ptr()
    flags, flags_host = ctypes.c_void_p(small + 4 * ncounters), ent.small_host[ncounters:ncounters + m]
    suspects = [j for j in range(m) if not counts[j]]
    rounds = done = 0
    if nsub:
        current = torch.cuda.current_stream()
        while not rounds:
            k = min(SYNC_BATCH, bound - done)
            if k < 1:
                raise RuntimeError(f"the device entropy decoder did not settle within its bound of {bound} launches")
            _call("vunet_jpeg_huffdec_sync", at(b_off), nscan, at(r_off), at_host(r_off), nsub, at(t_off), at_host(t_off), host, m,
                  _p(ent.state), ent.state.numel(), _p(ent.small), ncounters, done, k, stream)
            done += k
            ent.small_host[:done].copy_(ent.small[:done], non_blocking=True)
            current.synchronize()                                      # the first wait: the convergence counters
            quiet = np.flatnonzero(ent.small_host[:done].numpy() == 0)
            rounds = int(quiet[0]) + 1 if quiet.size else 0
        _call("vunet_jpeg_huffdec_blocks", at(r_off), at_host(r_off), nsub, at(s_off), at_host(s_off), host, m, _p(ent.state),
              ent.state.numel(), flags, m, stream)
        _call("vunet_jpeg_huffdec_write", at(b_off), nscan, at(r_off), at_host(r_off), nsub, at(t_off), at_host(t_off), at(0), host, m,
              _p(ent.state), ent.state.numel(), done, _p(ent.coef), coef_count, flags, m, stream)
        _call("vunet_jpeg_huffdec_dc", at(0), host, at(t_off), at_host(t_off), m, _p(ent.coef), coef_count, stream)
        flags_host.copy_(ent.small[ncounters:ncounters + m], non_blocking=True)
        current.synchronize()                                          # the second wait: the per-image flags
        suspects = sorted(set(suspects) | set(np.flatnonzero(flags_host.numpy()).tolist()))
    _stats.update(rounds=rounds, launches=done, subsequences=nthreads, host_fallbacks=len(suspects))
    if suspects:
        # the host walk decides: its error is raised (the lowest index first), what it accepts goes into the image's slot
        scratch = ent.get("scratch", sum(own[j].ncoef for j in suspects), torch.int16, "pinned")
        qtab, put = np.empty(192, dtype=np.uint16), 0
        for j in suspects:
            i = native[j]
            rc = lib.vunet_jpeg_entropy_decode(data[i], len(data[i]), ctypes.byref(infos[i]), ctypes.c_void_p(scratch.data_ptr() + 2 * put),
                                               qtab.ctypes.data)
            if rc != 0:
                raise _error(rc, i)
            ent.coef[rows[j].coef_off:rows[j].coef_off + infos[i].ncoef].copy_(scratch[put:put + infos[i].ncoef], non_blocking=True)
            put += infos[i].ncoef
        torch.cuda.current_stream().synchronize()                      # (the scratch is free again when the next call writes it)
    _finish(buf, _p(ent.coef), coef_count, q_off, m, plane_bytes, out)


def decode_batch(streams: Sequence, hmax: Optional[int] = None, wmax: Optional[int] = None, out: Optional[torch.Tensor] = None,
                 threads: Optional[int] = None, fallback: bool = False, tag=None, entropy: str = "host"):
    """Encoded baseline JPEG streams (a sequence of ``bytes``) -> ``(frames, hw)``: frames uint8 [N, Hmax, Wmax, 3] on the current
    GPU, RGB interleaved, image n in ``frames[n, :h, :w]`` -- bit for bit ``np.asarray(Image.open(..).convert("RGB"))`` --, and hw
    int32 [N, 2] (h, w) on the HOST (the headers are parsed there; no synchronisation is needed to know it).

    ``hmax`` / ``wmax``: a larger stack than the largest image.  ``out``: the stack to write into (uint8 [N, Hmax, Wmax, 3] on the
    current GPU, contiguous); bytes outside an image's h x w are left as they are.  Without ``out`` the stack is a cached buffer
    (zeros outside any image it ever held), valid until the next call with the same shape and ``tag`` -- two inputs of one step that
    are decoded separately take different tags.  ``threads``: host threads of the entropy decode, default ``min(N, 8)``, at most 16.

    The entropy decode writes into a reused pinned buffer; one upload, then two launches on the current stream, no
    synchronisation but the wait for the previous call's upload to have left that buffer.  Nothing is allocated after the first
    call at a shape.  Not recordable into a hipGraph (the host decode would not be replayed): issue it ahead of the replay.

    ``JpegUnsupported`` for a stream outside the supported subset -- or, with ``fallback=True``, Pillow decodes it on the host and
    its frame is uploaded (``JpegUnsupported`` still where PIL does not import).  ``JpegCorrupt`` always raises.

    ``entropy="device"``: the Huffman walk runs on the GPU too (csrc/jpeg_huff_dec.hip; ``_decode_device``).  Same frames, same
    ``hw``, same exceptions for every input; the stream bytes go up instead of the coefficients.  It waits for the device twice (the
    convergence counter, the per-image flags), so it is no more recordable into a hipGraph than the host route.  A stream whose
    marker layout is not the plain one, or that the device flags, is decoded by the host walk (``last_stats()["host_fallbacks"]``)."""
    if entropy not in ("host", "device"):
        raise ValueError(f'decode_batch: entropy is "host" or "device", got {entropy!r}')
    if isinstance(streams, (bytes, bytearray, memoryview)) or not hasattr(streams, "__len__"):
        raise TypeError("decode_batch: a sequence of bytes objects expected (one stream per image)")
    data = [_bytes(s, i) for i, s in enumerate(streams)]
    n = len(data)
    if not 1 <= n <= MAX_SIDE:
        raise ValueError(f"decode_batch: 1 <= N <= {MAX_SIDE} streams expected, got {n}")
    threads = min(n, 8) if threads is None else int(threads)
    if not 1 <= threads <= MAX_THREADS:
        raise ValueError(f"decode_batch: 1 <= threads <= {MAX_THREADS} expected, got {threads}")
    infos, foreign = [], {}
    for i, d in enumerate(data):
        try:
            infos.append(_parse_c(d, i))
        except JpegUnsupported as e:
            if not fallback:
                raise
            foreign[i] = _pillow_rgb(d, i, e)
            infos.append(None)
    sizes = [(inf.height, inf.width) if inf is not None else foreign[i].shape[:2] for i, inf in enumerate(infos)]
    hm, wm = max(max(h for h, _ in sizes), int(hmax or 0)), max(max(w for _, w in sizes), int(wmax or 0))
    if (hmax is not None and int(hmax) < hm) or (wmax is not None and int(wmax) < wm) or hm > MAX_SIDE or wm > MAX_SIDE:
        raise ValueError(f"decode_batch: the largest image is {max(h for h, _ in sizes)} x {max(w for _, w in sizes)}; hmax, wmax = "
                         f"{hmax}, {wmax} must hold it and be <= {MAX_SIDE}")
    device = _device()
    if out is not None:
        if not torch.is_tensor(out) or out.dtype != torch.uint8 or tuple(out.shape) != (n, hm, wm, 3) or not out.is_contiguous() or \
                out.device != device:
            raise ValueError(f"out: contiguous uint8 [{n}, {hm}, {wm}, 3] on {device} expected, got "
                             f"{getattr(out, 'dtype', type(out))} {tuple(getattr(out, 'shape', ()))} on {getattr(out, 'device', None)}")
    key = (str(device), _stream().value if device.type == "cuda" else 0, tag)
    buf = _buffers.get(key)
    if buf is None:
        buf = _buffers[key] = Arena(device, "planes")
        buf.outs = {}
    if out is None and (n, hm, wm) not in buf.outs:
        buf.outs[n, hm, wm] = torch.zeros(n, hm, wm, 3, dtype=torch.uint8, device=device)
    frames = buf.outs[n, hm, wm] if out is None else out
    native = [i for i in range(n) if infos[i] is not None]
    if native:
        (_decode_device if entropy == "device" else _decode_host)(buf, data, infos, native, threads, frames)
    for i, f in foreign.items():
        frames[i, :f.shape[0], :f.shape[1]].copy_(torch.from_numpy(f))
    return frames, torch.tensor(sizes, dtype=torch.int32).reshape(n, 2)
