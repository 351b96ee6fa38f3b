"""Baseline JPEG encode of device frames: the uint8 stacks every video call of ``render`` ends in -> JFIF byte streams.  What the
reference does per frame on the host -- ``cv2.imwrite`` / the frames of ``cv2.VideoWriter`` (lib/logging.py, lib/figures.py,
data/*.py) -- is split here where the work changes character, the mirror image of ``jpeg_decode`` (csrc/jpeg_enc.hip,
csrc/jpeg_huff_enc.h, include/vunet_jpeg_enc.h):

* colour conversion, chroma down-sampling, the forward DCT and the quantiser are two HIP launches for the whole batch, whatever the
  images' sizes, after ONE small upload (descriptors and tables), and ONE download of the quantised coefficients into a reused
  pinned buffer;
* the entropy coder, a serial bit walk, stays on the host: the library's C++ on ``jpeg_decode``'s small thread pool (ctypes
  releases the GIL).

The bytes are Pillow's ``Image.save(.., "JPEG", quality=q, subsampling=s)`` (libjpeg-turbo's defaults: the "islow" integer forward
DCT, the Annex K tables), pinned against Pillow 12.2.0 by tests/golden/g24_jpeg_encode.npz.  ASSUMED, NOT PINNED: ``cv2.imwrite``
writes with other defaults (quality 95, 4:2:0) -- ``quality=95`` mimics it -- and OpenCV is no dependency of this package.

* ``encode_batch``  frames -> ``list[bytes]``;
* ``save_images``   a thin loop over it: one ``.jpg`` per frame;
* ``JpegEncodeError``  carries the C error code.

Not done: optimised Huffman tables, progressive mode, restart markers.  There is no CPU path."""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib
from .jpeg_decode import MAX_SIDE, MAX_THREADS, JpegImg, JpegInfoC, _pool
from .ops import _call, _p, _stream

SUBSAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}
ERR_CAPACITY = _lib.const("VUNET_JPEG_ERR_CAPACITY")
REASONS = {ERR_CAPACITY: "the stream is longer than its output buffer",
           _lib.const("VUNET_JPEG_ERR_RANGE"): "a coefficient outside baseline's range (DC difference > 11 bits or AC > 10 bits)",
           _lib.const("VUNET_ERR_ARG"): "an argument the library refuses"}


class JpegEncodeError(ValueError):
    """``code``: the library's value; ``index``: the frame's place in the batch."""

    def __init__(self, code: int, index: Optional[int] = None):
        self.code, self.reason, self.index = int(code), REASONS.get(int(code), "unknown error"), index
        where = "" if index is None else f"frame {index}: "
        super().__init__(f"{where}{self.reason} (code {self.code})")


def _device() -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError("encode_batch needs the GPU (hand-written gfx950 kernels; no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


class _Buffers:
    """The reused memory of one (device, stream): the pinned descriptor / table block and its device mirror, the component planes
    and the coefficients on the device, the pinned coefficients and the streams' bytes on the host.  Grow-only: a second call at a
    shape allocates nothing."""

    def __init__(self, device: torch.device):
        self.device, self.stage, self.dev, self.planes, self.coef, self.coef_host, self.event, self.out = \
            device, None, None, None, None, None, None, None

    def reserve(self, up_bytes: int, coef_count: int, out_bytes: int):
        pin = self.device.type == "cuda"
        if self.stage is None or self.stage.numel() < up_bytes:
            self.stage = torch.empty(up_bytes, dtype=torch.uint8, pin_memory=pin)
            self.dev = torch.empty(up_bytes, dtype=torch.uint8, device=self.device)
        if self.coef is None or self.coef.numel() < coef_count:
            self.planes = torch.empty(coef_count, dtype=torch.uint8, device=self.device)
            self.coef = torch.empty(coef_count, dtype=torch.int16, device=self.device)
            self.coef_host = torch.empty(coef_count, dtype=torch.int16, pin_memory=pin)
        if self.out is None or self.out.size < out_bytes:
            self.out = np.empty(out_bytes, dtype=np.uint8)


_buffers: Dict[tuple, _Buffers] = {}


def clear_buffers() -> None:
    """Drop the cached buffers."""
    _buffers.clear()


def quant_tables(quality: int) -> np.ndarray:
    """uint16 [2, 64], natural order: the Annex K tables at libjpeg's ``quality`` (1 .. 100), luma then chroma.  Host only."""
    q = np.empty((2, 64), dtype=np.uint16)
    _call("vunet_jpeg_quant_tables", int(quality), q.ctypes.data)
    return q


def _launch(buf: _Buffers, frames: torch.Tensor, m: int, channels: int, up_bytes: int, q_off: int, q_count: int, coef_count: int) -> None:
    """One upload of the descriptors and tables, the two launches and the download of the coefficients into the pinned buffer, on the
    current stream, waited for.  The host copy of the descriptors is what the library checks before it launches."""
    n, hmax, wmax = (int(v) for v in frames.shape[:3])
    buf.dev[:up_bytes].copy_(buf.stage[:up_bytes], non_blocking=True)
    base = buf.dev.data_ptr()
    imgs, qtab, host = ctypes.c_void_p(base), ctypes.c_void_p(base + q_off), ctypes.c_void_p(buf.stage.data_ptr())
    _call("vunet_jpeg_from_rgb", _p(frames), n, hmax, wmax, channels, imgs, host, m, _p(buf.planes), coef_count, _stream())
    _call("vunet_jpeg_fdct", _p(buf.planes), coef_count, qtab, q_count, imgs, host, m, _p(buf.coef), coef_count, _stream())
    buf.coef_host[:coef_count].copy_(buf.coef[:coef_count], non_blocking=True)
    if buf.event is None:
        buf.event = torch.cuda.Event()
    buf.event.record()
    buf.event.synchronize()


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


def encode_batch(frames: torch.Tensor, quality=75, subsampling="4:2:0", sizes=None, threads: int = 8) -> List[bytes]:
    """``frames`` uint8 [N, H, W, 3] (RGB interleaved) or [N, H, W] (gray) on the current GPU -> N baseline JPEG streams, image n
    byte for byte ``Image.fromarray(frames[n, :h, :w]).save(.., "JPEG", quality=quality, subsampling=subsampling)``.

    ``quality``: libjpeg's 1 .. 100.  ``subsampling``: "4:4:4", "4:2:2" or "4:2:0" (ignored for gray).  Either may be a list with one
    value per image: the two launches take mixed samplings and tables as they take mixed sizes.  ``sizes``: per-image
    ``(h, w)`` inside the padded stack, as ``decode_batch`` returns them (default: every image fills it).  ``threads``: host threads
    of the entropy coder, at most 16.

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
    threads = int(threads)
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
        buf = _buffers[key] = _Buffers(device)
    q_off = n * ctypes.sizeof(JpegImg)
    levels = sorted(set(int(q) for q in quality))     # one [3][64] table block per distinct quality
    tables = np.concatenate([quant_tables(q)[[0, 1, 1]] for q in levels])
    table_of = {q: 192 * i for i, q in enumerate(levels)}
    up_bytes = q_off + tables.nbytes
    coef_count = sum(i.ncoef for i in infos)
    caps = [1024 + 2 * i.ncoef for i in infos]        # two bytes per coefficient (0/255 noise at quality 100 takes 1.6); a longer one: below
    buf.reserve(up_bytes, coef_count, sum(caps))
    base = buf.stage.data_ptr()
    rows = (JpegImg * n).from_address(base)
    ctypes.memmove(base + q_off, tables.ctypes.data, tables.nbytes)
    coef_at, block_at = 0, 0
    for j, inf in enumerate(infos):
        r = rows[j]
        r.coef_off, r.plane_off, r.q_off, r.block0, r.slot = coef_at, coef_at, table_of[int(quality[j])], block_at, j
        r.height, r.width, r.ncomp, r.hsamp, r.vsamp = inf.height, inf.width, inf.ncomp, inf.hsamp, inf.vsamp
        r.bw0, r.bh0, r.bw1, r.bh1 = inf.bw0, inf.bh0, inf.bw1, inf.bh1
        coef_at, block_at = coef_at + inf.ncoef, block_at + inf.nblocks
    _launch(buf, frames, n, channels, up_bytes, q_off, tables.size, coef_count)
    fn, cbase, obase, qbase = lib.vunet_jpeg_entropy_encode, buf.coef_host.data_ptr(), buf.out.ctypes.data, tables.ctypes.data
    offs = np.concatenate([[0], np.cumsum(caps)]).tolist()
    coffs = np.concatenate([[0], np.cumsum([i.ncoef for i in infos])]).tolist()

    def one(j):
        length, qptr = ctypes.c_int64(0), qbase + 2 * table_of[int(quality[j])]
        rc = fn(ctypes.c_void_p(cbase + 2 * coffs[j]), ctypes.byref(infos[j]), ctypes.c_void_p(qptr), ctypes.c_void_p(obase + offs[j]),
                caps[j], ctypes.byref(length))
        if rc == ERR_CAPACITY:                            # the stream is coded again into a buffer of the length it asked for
            own = np.empty(length.value, dtype=np.uint8)
            rc = fn(ctypes.c_void_p(cbase + 2 * coffs[j]), ctypes.byref(infos[j]), ctypes.c_void_p(qptr), own.ctypes.data,
                    own.size, ctypes.byref(length))
            return rc, own.tobytes()
        return rc, buf.out[offs[j]:offs[j] + length.value].tobytes()
    res = [one(j) for j in range(n)] if threads == 1 or n == 1 else list(_pool(threads).map(one, range(n)))
    for j, (rc, _) in enumerate(res):
        if rc != 0:
            raise JpegEncodeError(rc, j)
    return [data for _, data in res]


def _paths(pattern: str, count: int, start: int = 0) -> List[str]:
    """``pattern`` with one ``%d``-style or one ``{}``-style field -> ``count`` file names from index ``start``."""
    if "%" in pattern:
        names = [pattern % (start + i) for i in range(count)]
    else:
        names = [pattern.format(start + i) for i in range(count)]
    if len(set(names)) != count:
        raise ValueError(f"pattern {pattern!r} names {count} files alike: it needs an index field such as %06d or {{:06d}}")
    return names


def save_images(pattern: str, frames: torch.Tensor, quality: int = 75, subsampling: str = "4:2:0", sizes=None, start: int = 0,
                threads: int = 8) -> List[str]:
    """``encode_batch`` and one file per frame: ``pattern % index`` (``"img_%06d.jpg"``, the reference's frame names) or
    ``pattern.format(index)``, indices from ``start``.  -> the paths written."""
    streams = encode_batch(frames, quality, subsampling, sizes, threads)
    paths = _paths(pattern, len(streams), start)
    for path, data in zip(paths, streams):
        with open(path, "wb") as f:
            f.write(data)
    return paths
