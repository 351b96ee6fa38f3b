"""The host layer that ``jpeg_decode`` and ``jpeg_encode`` share: the ctypes handles and limits of include/vunet_jpeg.h, the one writer
of the ``vunet_jpeg_img`` descriptor table, the grow-only memory of a (device, stream), the byte layout of an upload, the thread
pool of the per-image host work, the error base and the frame file names.  No launch is issued here: every library call that
launches goes through the ``_call`` attribute of the codec module that makes it."""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor
from typing import Dict, List, Optional

import torch

from . import _lib

JpegInfoC = _lib.struct("vunet_jpeg_info")
JpegImg = _lib.struct("vunet_jpeg_img")
MAX_SIDE = 65535                         # N, Hmax, Wmax of one call (grid dimensions)
MAX_THREADS = 16


class _CodecError(ValueError):
    """``code``: the library's value; ``reason``: what the subclass's ``REASONS`` says of it; ``index``: the place in the batch of
    what the subclass's ``WHAT`` names (a stream, a frame)."""
    REASONS: Dict[int, str] = {}
    WHAT = ""

    def __init__(self, code: int, index: Optional[int] = None):
        self.code, self.reason, self.index = int(code), self.REASONS.get(int(code), "unknown error"), index
        where = "" if index is None else f"{self.WHAT} {index}: "
        super().__init__(f"{where}{self.reason} (code {self.code})")


def device(what: str) -> torch.device:
    if not torch.cuda.is_available():
        raise RuntimeError(f"{what} needs the GPU (hand-written gfx950 kernels; no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def round_up(v: int, m: int) -> int:
    return (v + m - 1) // m * m


def layout(*pieces):
    """Pieces ``(name, size, alignment)`` one after another, each at the next multiple of its alignment -> ``({name: offset},
    total)``, in the unit of the sizes (bytes of an upload, words of a counter block)."""
    offs, at = {}, 0
    for name, size, align in pieces:
        offs[name] = at = round_up(at, align)
        at += size
    return offs, at


def fill_rows(rows, infos, q_offs, slots):
    """The descriptor table: ``rows[j]`` (``vunet_jpeg_img``) from ``infos[j]``, its table offset and its slot in the frame stack.
    Coefficients, planes and blocks lie image after image.  -> (coefficients, blocks) of the batch."""
    coef_at, block_at = 0, 0
    for r, inf, q_off, slot in zip(rows, infos, q_offs, slots):
        r.coef_off, r.plane_off, r.q_off, r.block0, r.slot = coef_at, coef_at, q_off, block_at, slot
        r.height, r.width, r.ncomp, r.hsamp, r.vsamp = inf.height, inf.width, inf.ncomp, inf.hsamp, inf.vsamp
        r.bw0, r.bh0, r.bw1, r.bh1 = inf.bw0, inf.bh0, inf.bw1, inf.bh1
        coef_at, block_at = coef_at + inf.ncoef, block_at + inf.nblocks
    return coef_at, block_at


class Arena:
    """The reused memory of one (device, stream[, tag]): buffers by name, ``None`` until first asked for and replaced only when too
    small, so that a second call at a shape allocates nothing.  ``stage`` / ``dev`` are the pinned staging buffer and its device
    mirror, with the one event that says when an upload has left the former.  ``layout``: whatever the last call laid out in its
    buffers (for tools).  ``entropy``: the device route's own arena, made on that route's first call."""

    def __init__(self, device: torch.device, names: str):
        self.device, self.event, self.layout, self.entropy, self.upload_bytes = device, None, None, None, 0
        for name in ("stage", "dev", *names.split()):
            setattr(self, name, None)

    def get(self, name: str, count: int, dtype, place: str = "device") -> torch.Tensor:
        """``place``: "device", "pinned" (host memory, pinned where the device is a GPU) or "host"."""
        cur = getattr(self, name)
        if cur is None or cur.numel() < count:
            kw = dict(device=self.device) if place == "device" else dict(pin_memory=place == "pinned" and self.device.type == "cuda")
            cur = torch.empty(count, dtype=dtype, **kw)
            setattr(self, name, cur)
        return cur

    def staging(self, nbytes: int) -> None:
        self.wait()                       # the last upload has left the pinned buffer before the host writes it again
        self.get("stage", nbytes, torch.uint8, "pinned")
        self.get("dev", nbytes, torch.uint8)

    def upload(self, nbytes: int) -> None:
        self.dev[:nbytes].copy_(self.stage[:nbytes], non_blocking=True)
        self.record()

    def record(self) -> None:
        if self.event is None:
            self.event = torch.cuda.Event()
        self.event.record()

    def wait(self) -> None:
        if self.event is not None:
            self.event.synchronize()


_pools: Dict[int, ThreadPoolExecutor] = {}


def per_image(fn, items, threads: int) -> list:
    """``[fn(item) for item in items]``, on the shared pool of ``threads`` where that can help (ctypes releases the GIL)."""
    if threads == 1 or len(items) == 1:
        return [fn(item) for item in items]
    if threads not in _pools:
        _pools[threads] = ThreadPoolExecutor(max_workers=threads, thread_name_prefix="vunet-jpeg")
    return list(_pools[threads].map(fn, items))


def frame_paths(pattern: str, count: int, start: int = 0) -> List[str]:
    """``pattern`` with one ``%d``-style or one ``{}``-style field -> ``count`` file names from index ``start``."""
    if "%" in pattern:
        names = [pattern % (start + i) for i in range(count)]
    else:
        names = [pattern.format(start + i) for i in range(count)]
    if len(set(names)) != count:
        raise ValueError(f"pattern {pattern!r} names {count} files alike: it needs an index field such as %06d or {{:06d}}")
    return names
