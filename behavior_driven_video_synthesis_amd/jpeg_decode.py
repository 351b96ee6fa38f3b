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

Supported: baseline sequential, 8-bit, 1 or 3 components, 4:4:4 / 4:2:2 / 4:2:0, one interleaved scan, restart intervals.
Progressive, arithmetic-coded, 12-bit and CMYK streams are refused (``fallback=True`` hands them to Pillow on the host where PIL
imports).  There is no CPU path for the supported ones."""
from __future__ import annotations

import ctypes
import io
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .ops import _call, _p, _stream

JpegInfoC = _lib.struct("vunet_jpeg_info")
JpegImg = _lib.struct("vunet_jpeg_img")
MAX_SIDE = 65535                         # N, Hmax, Wmax of one call (grid dimensions)
MAX_THREADS = 16

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


class JpegError(ValueError):
    """``code``: the library's VUNET_JPEG_ERR_* value; ``reason``: what it says; ``index``: the stream's place in the batch."""

    def __init__(self, code: int, index: Optional[int] = None):
        self.code, self.reason, self.index = int(code), REASONS.get(int(code), "unknown error"), index
        where = "" if index is None else f"stream {index}: "
        super().__init__(f"{where}{self.reason} (code {self.code})")


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


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("decode_batch needs the GPU (hand-written gfx950 kernels; no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


class _Buffers:
    """The reused memory of one (device, stream, tag): the pinned staging buffer, its device mirror, the component planes, the
    default output stacks.  Grow-only: a second call at a shape allocates nothing."""

    def __init__(self, device: torch.device):
        self.device, self.stage, self.dev, self.planes, self.event, self.outs = device, None, None, None, None, {}
        self.entropy = None               # the device entropy route's own buffers (``_Entropy``), made on its first call

    def reserve(self, nbytes: int, plane_bytes: int):
        if self.event is not None:
            self.event.synchronize()      # the last upload has left the pinned buffer before the host writes it again
        if self.stage is None or self.stage.numel() < nbytes:
            pin = self.device.type == "cuda"
            self.stage = torch.empty(nbytes, dtype=torch.uint8, pin_memory=pin)
            self.dev = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        if self.planes is None or self.planes.numel() < plane_bytes:
            self.planes = torch.empty(plane_bytes, dtype=torch.uint8, device=self.device)

    def out(self, n: int, hmax: int, wmax: int) -> torch.Tensor:
        key = (n, hmax, wmax)
        if key not in self.outs:
            self.outs[key] = torch.zeros(n, hmax, wmax, 3, dtype=torch.uint8, device=self.device)
        return self.outs[key]


_buffers: Dict[tuple, _Buffers] = {}
_pools: Dict[int, ThreadPoolExecutor] = {}


def clear_buffers() -> None:
    """Drop the cached buffers (not while frames returned without ``out=`` are still in use)."""
    _buffers.clear()


def _pool(threads: int) -> ThreadPoolExecutor:
    if threads not in _pools:
        _pools[threads] = ThreadPoolExecutor(max_workers=threads, thread_name_prefix="vunet-jpeg")
    return _pools[threads]


def _round(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def _pillow_rgb(data: bytes, index: int, err: JpegError) -> np.ndarray:
    try:
        from PIL import Image
    except ImportError:
        raise err from None
    return np.array(Image.open(io.BytesIO(data)).convert("RGB"))   # (a writable copy)


def _launch(buf: _Buffers, m: int, nbytes: int, q_off: int, c_off: int, coef_count: int, plane_bytes: int, out: torch.Tensor) -> None:
    """One upload of the staging buffer's first ``nbytes`` (descriptors | tables | coefficients) and the two launches, on the current
    stream.  The host copy of the descriptors is what the library checks before it launches."""
    n, hmax, wmax = (int(v) for v in out.shape[:3])
    buf.dev[:nbytes].copy_(buf.stage[:nbytes], non_blocking=True)
    if buf.event is None:
        buf.event = torch.cuda.Event()
    buf.event.record()
    base = buf.dev.data_ptr()
    coef, qtab, imgs = ctypes.c_void_p(base + c_off), ctypes.c_void_p(base + q_off), ctypes.c_void_p(base)
    host = ctypes.c_void_p(buf.stage.data_ptr())
    _call("vunet_jpeg_idct", coef, coef_count, qtab, m * 192, imgs, host, m, _p(buf.planes), plane_bytes, _stream())
    _call("vunet_jpeg_to_rgb", _p(buf.planes), plane_bytes, imgs, host, m, n, hmax, wmax, _p(out), _stream())


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


class _Entropy:
    """The device route's own reused memory (grow-only, as ``_Buffers``): the coefficients, the walk's state, the counters and flags
    with their pinned mirror, and a pinned scratch for coefficients the host walk decodes instead."""

    def __init__(self, device: torch.device):
        self.device, self.coef, self.state, self.small, self.small_host, self.scratch = device, None, None, None, None, None
        self.upload_bytes = 0

    def reserve(self, coef_count: int, state_words: int, small_words: int):
        if self.coef is None or self.coef.numel() < coef_count:
            self.coef = torch.empty(coef_count, dtype=torch.int16, device=self.device)
        if self.state is None or self.state.numel() < state_words:
            self.state = torch.empty(state_words, dtype=torch.int32, device=self.device)
        if self.small is None or self.small.numel() < small_words:
            self.small = torch.empty(small_words, dtype=torch.int32, device=self.device)
            self.small_host = torch.empty(small_words, dtype=torch.int32, pin_memory=self.device.type == "cuda")

    def host_coef(self, count: int) -> torch.Tensor:
        if self.scratch is None or self.scratch.numel() < count:
            self.scratch = torch.empty(count, dtype=torch.int16, pin_memory=self.device.type == "cuda")
        return self.scratch


def _scan(lib, d: bytes, inf):
    """The marker scan of one stream -> (code, segments int64 [nseg, 3], qtab + table row as one uint8 array)."""
    mcus = inf.mcu_cols * inf.mcu_rows
    expected = -(-mcus // inf.restart) if inf.restart > 0 else 1
    segs, nseg, tabs = np.empty((expected, 3), dtype=np.int64), ctypes.c_int64(0), np.empty(384 + TAB_BYTES, dtype=np.uint8)
    rc = lib.vunet_jpeg_scan_segments(d, len(d), ctypes.byref(inf), segs.ctypes.data, expected, ctypes.byref(nseg), tabs.ctypes.data,
                                      tabs.ctypes.data + 384)
    return rc, segs[:nseg.value], tabs


def _decode_device(buf: _Buffers, data, infos, native, threads: int, out: torch.Tensor) -> None:
    """The device route of ``decode_batch`` for the streams ``native`` (indices with a parsed header): marker scan on the host (no bit
    walk), ONE upload of descriptors | quantisation tables | table rows | spans | subsequence rows | scan bytes, the sync launches
    with a readback of their counters every ``SYNC_BATCH`` (the first wait), block ordinals, write and DC sums, a readback of the
    per-image flags (the second wait), the host walk for what was irregular or flagged, then the two launches of the host route."""
    lib, m = _lib.lib(), len(native)
    scans = [_scan(lib, data[i], infos[i]) for i in native] if threads == 1 or m == 1 else \
        list(_pool(threads).map(lambda i: _scan(lib, data[i], infos[i]), native))
    for i, (rc, _, _) in zip(native, scans):
        if rc < 0:
            raise _error(rc, i)
    # the layout of the upload; an irregular stream brings no rows and no bytes
    counts, offs, nsub, nscan, nthreads = [], [], 0, 0, 0
    for rc, segs, _ in scans:
        rows = 0 if rc else int(((segs[:, 1] - segs[:, 0] + SUBSEQ_BYTES - 1) // SUBSEQ_BYTES).sum())
        counts.append(_round(rows, GROUP))
        nthreads += rows
        offs.append(nscan - (int(segs[0, 0]) if rows else 0))
        nsub, nscan = nsub + counts[-1], nscan + (_round(int(segs[-1, 1] - segs[0, 0]), 16) if rows else 0)
    if nscan > MAX_SCAN_BYTES:
        raise ValueError(f'decode_batch: {nscan} bytes of scans in one call; entropy="device" takes at most {MAX_SCAN_BYTES} '
                         '(entropy="host" has no such limit)')
    q_off = m * ctypes.sizeof(JpegImg)
    t_off = _round(q_off + m * 384, 16)
    s_off = t_off + m * TAB_BYTES
    r_off = _round(s_off + 8 * m, 16)
    b_off = r_off + nsub * ctypes.sizeof(Subseq)
    nbytes = _round(b_off + nscan, 16) + 16
    coef_count = sum(infos[i].ncoef for i in native)
    plane_bytes = max(coef_count, 16)
    buf.reserve(nbytes, plane_bytes)
    if buf.entropy is None:
        buf.entropy = _Entropy(buf.device)
    ent = buf.entropy
    bound = max(counts) // GROUP + 1
    ncounters = _round(bound, SYNC_BATCH)
    ent.reserve(coef_count, max(nsub * STATE_WORDS, 4), ncounters + m)
    ent.upload_bytes = nbytes                                          # (what tools/time_jpeg.py reports)
    base = buf.stage.data_ptr()
    stage = buf.stage.numpy()
    rows, spans = (JpegImg * m).from_address(base), stage[s_off:s_off + 8 * m].view(np.int32).reshape(m, 2)
    coef_at, block_at, row_at = 0, 0, 0
    for j, i in enumerate(native):
        inf, r, (rc, segs, tabs) = infos[i], rows[j], scans[j]
        r.coef_off, r.plane_off, r.q_off, r.block0, r.slot = coef_at, coef_at, 192 * j, block_at, i
        r.height, r.width, r.ncomp, r.hsamp, r.vsamp = inf.height, inf.width, inf.ncomp, inf.hsamp, inf.vsamp
        r.bw0, r.bh0, r.bw1, r.bh1 = inf.bw0, inf.bh0, inf.bw1, inf.bh1
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
        coef_at, block_at, row_at = coef_at + inf.ncoef, block_at + inf.nblocks, row_at + counts[j]
    buf.dev[:nbytes].copy_(buf.stage[:nbytes], non_blocking=True)
    if buf.event is None:
        buf.event = torch.cuda.Event()
    buf.event.record()
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
        scratch = ent.host_coef(sum(infos[native[j]].ncoef for j in suspects))
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
    n, hmax, wmax = (int(v) for v in out.shape[:3])
    _call("vunet_jpeg_idct", _p(ent.coef), coef_count, at(q_off), m * 192, at(0), host, m, _p(buf.planes), plane_bytes, stream)
    _call("vunet_jpeg_to_rgb", _p(buf.planes), plane_bytes, at(0), host, m, n, hmax, wmax, _p(out), stream)


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
        buf = _buffers[key] = _Buffers(device)
    native = [i for i in range(n) if infos[i] is not None]
    m = len(native)
    q_off = m * ctypes.sizeof(JpegImg)
    c_off = _round(q_off + m * 384, 128)
    coef_count = sum(infos[i].ncoef for i in native)
    nbytes, plane_bytes = c_off + 2 * coef_count, max(coef_count, 16)
    if not (m and entropy == "device"):      # (the device route sizes its own, smaller, upload)
        buf.reserve(max(nbytes, 16), plane_bytes)
    frames = buf.out(n, hm, wm) if out is None else out
    if m and entropy == "device":
        _decode_device(buf, data, infos, native, threads, frames)
    elif m:
        base = buf.stage.data_ptr()
        rows = (JpegImg * m).from_address(base)
        jobs, coef_at, block_at = [], 0, 0
        for j, i in enumerate(native):
            inf, r = infos[i], rows[j]
            r.coef_off, r.plane_off, r.q_off, r.block0, r.slot = coef_at, coef_at, 192 * j, block_at, i
            r.height, r.width, r.ncomp, r.hsamp, r.vsamp = inf.height, inf.width, inf.ncomp, inf.hsamp, inf.vsamp
            r.bw0, r.bh0, r.bw1, r.bh1 = inf.bw0, inf.bh0, inf.bw1, inf.bh1
            jobs.append((i, inf, base + c_off + 2 * coef_at, base + q_off + 384 * j))
            coef_at, block_at = coef_at + inf.ncoef, block_at + inf.nblocks
        fn = _lib.lib().vunet_jpeg_entropy_decode

        def one(job):
            i, inf, cptr, qptr = job
            return fn(data[i], len(data[i]), ctypes.byref(inf), ctypes.c_void_p(cptr), ctypes.c_void_p(qptr))
        codes = [one(j) for j in jobs] if threads == 1 or m == 1 else list(_pool(threads).map(one, jobs))
        for (i, *_), rc in zip(jobs, codes):
            if rc != 0:
                raise _error(rc, i)
        _launch(buf, m, nbytes, q_off, c_off, coef_count, plane_bytes, frames)
    for i, f in foreign.items():
        frames[i, :f.shape[0], :f.shape[1]].copy_(torch.from_numpy(f))
    return frames, torch.tensor(sizes, dtype=torch.int32).reshape(n, 2)
