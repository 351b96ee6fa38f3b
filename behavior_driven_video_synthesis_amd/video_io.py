"""Motion-JPEG videos of device frames: what the reference writes with ``cv2.VideoWriter(.., "MP4V", 12, ..)`` at the end of every
video call (lib/logging.py, lib/figures.py) becomes an AVI file whose frames are the baseline JPEG streams of ``jpeg_encode`` -- the
one container a player opens that needs no inter-frame codec.

* ``write_mjpeg``          frames uint8 [T, H, W, 3] on the GPU -> one ``.avi``;
* ``save_videos``          frames [B, T, H, W, 3] -> one file per row, all B * T frames encoded in one batch;
* ``write_mjpeg_streams``  ready JPEG streams -> the file (host only);
* ``read_mjpeg``           the file -> ``(fps, list[bytes])``; ``jpeg_decode.decode_batch(read_mjpeg(p)[1])`` gives a written video back
  on the device.

The file: ``RIFF <size> 'AVI '``; ``LIST 'hdrl'`` with ``avih`` (56 bytes) and one ``LIST 'strl'`` of ``strh`` (56 bytes: ``vids`` /
``MJPG``, dwRate / dwScale = fps) and ``strf`` (a 40-byte BITMAPINFOHEADER: 24 bit, biCompression ``MJPG``); ``LIST 'movi'`` with one
``00dc`` chunk per frame, padded to even length; ``idx1`` with one 16-byte entry per frame -- key-frame flag, offset of the chunk
header from the ``movi`` tag, chunk size.  Every number is little-endian.

ASSUMED, NOT PINNED: that an external player opens the file (none is at hand where the tests run: they check the structure and the
round trip).  Not done: MP4 or any inter-frame codec, audio, files past 4 GiB (OpenDML)."""
from __future__ import annotations

import struct
from fractions import Fraction
from typing import List, Sequence, Tuple

import torch

AVIF_HASINDEX, AVIIF_KEYFRAME = 0x10, 0x10
MAX_RIFF = 0xFFFFFFFF


def _chunk(tag: bytes, body: bytes) -> bytes:
    return tag + struct.pack("<I", len(body)) + body + (b"\0" if len(body) & 1 else b"")


def _list(kind: bytes, body: bytes) -> bytes:
    return b"LIST" + struct.pack("<I", 4 + len(body)) + kind + body


def write_mjpeg_streams(path: str, streams: Sequence[bytes], width: int, height: int, fps=12) -> str:
    """JPEG streams (all ``width`` x ``height``) -> the AVI file ``path``.  Host only.  ``fps``: frames per second, an int, a float or
    a ``Fraction`` (stored as dwRate / dwScale with a denominator of at most 1000)."""
    streams = [bytes(s) for s in streams]
    if not streams or any(s[:2] != b"\xff\xd8" for s in streams):
        raise ValueError("write_mjpeg_streams: at least one frame, each a JPEG stream (SOI first), expected")
    rate = Fraction(fps).limit_denominator(1000)
    if rate <= 0 or not (1 <= int(width) <= 65535 and 1 <= int(height) <= 65535):
        raise ValueError(f"write_mjpeg_streams: fps > 0 and 1 <= width, height <= 65535 expected, got {fps}, {width}, {height}")
    n, largest = len(streams), max(len(s) for s in streams)
    movi, index, at = [], [], 4                               # offsets count from the 'movi' tag
    for s in streams:
        c = _chunk(b"00dc", s)
        index.append(struct.pack("<4sIII", b"00dc", AVIIF_KEYFRAME, at, len(s)))
        movi.append(c)
        at += len(c)
    movi = b"".join(movi)
    avih = struct.pack("<14I", round(1e6 / rate), int(largest * rate) + 1, 0, AVIF_HASINDEX, n, 0, 1, largest, width, height, 0, 0, 0, 0)
    strh = struct.pack("<4s4sIHHIIIIIIIIHHHH", b"vids", b"MJPG", 0, 0, 0, 0, rate.denominator, rate.numerator, 0, n, largest,
                       0xFFFFFFFF, 0, 0, 0, width, height)
    strf = struct.pack("<IiiHH4sIiiII", 40, width, height, 1, 24, b"MJPG", width * height * 3, 0, 0, 0, 0)
    body = b"AVI " + _list(b"hdrl", _chunk(b"avih", avih) + _list(b"strl", _chunk(b"strh", strh) + _chunk(b"strf", strf))) + \
        _list(b"movi", movi) + _chunk(b"idx1", b"".join(index))
    if len(body) > MAX_RIFF:
        raise ValueError(f"write_mjpeg_streams: {len(body)} bytes do not fit one RIFF file (4 GiB)")
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)
    return path


def write_mjpeg(path: str, frames: torch.Tensor, fps=12, quality: int = 75, subsampling: str = "4:2:0", threads: int = 8,
                entropy: str = "host", optimize: bool = False) -> str:
    """``frames`` uint8 [T, H, W, 3] on the GPU -> the Motion-JPEG AVI ``path``: ``jpeg_encode.encode_batch`` once for the whole clip,
    then ``write_mjpeg_streams``.  The default of 12 frames per second is the reference's.  ``entropy`` and ``optimize`` are
    ``encode_batch``'s: every frame carries its own Huffman tables, so a file of optimised frames needs nothing else."""
    from . import jpeg_encode
    if not torch.is_tensor(frames) or frames.dim() != 4 or frames.shape[3] != 3:
        raise ValueError(f"write_mjpeg: frames uint8 [T, H, W, 3] expected, got {tuple(getattr(frames, 'shape', ()))}")
    streams = jpeg_encode.encode_batch(frames, quality, subsampling, threads=threads, entropy=entropy, optimize=optimize)
    return write_mjpeg_streams(path, streams, int(frames.shape[2]), int(frames.shape[1]), fps)


def save_videos(pattern: str, frames: torch.Tensor, fps=12, quality: int = 75, subsampling: str = "4:2:0", start: int = 0,
                threads: int = 8, entropy: str = "host", optimize: bool = False) -> List[str]:
    """``frames`` uint8 [B, T, H, W, 3] on the GPU (what ``render.*_video`` return) -> one file per row, ``pattern % index`` or
    ``pattern.format(index)`` from ``start``; all B * T frames are encoded in ONE batch.  -> the paths written."""
    from . import jpeg_encode
    if not torch.is_tensor(frames) or frames.dim() != 5 or frames.shape[4] != 3:
        raise ValueError(f"save_videos: frames uint8 [B, T, H, W, 3] expected, got {tuple(getattr(frames, 'shape', ()))}")
    b, t, h, w = (int(v) for v in frames.shape[:4])
    paths = jpeg_encode.frame_paths(pattern, b, start)
    streams = jpeg_encode.encode_batch(frames.reshape(b * t, h, w, 3), quality, subsampling, threads=threads, entropy=entropy,
                                       optimize=optimize)
    for i, path in enumerate(paths):
        write_mjpeg_streams(path, streams[i * t:(i + 1) * t], w, h, fps)
    return paths


def _chunks(data: bytes, at: int, end: int, what: str):
    """The (tag, body offset, size) of the chunks of ``data[at:end]``; raises where one runs past ``end``."""
    while at < end:
        if at + 8 > end:
            raise ValueError(f"read_mjpeg: a chunk header of {what} is cut short at byte {at}")
        tag, size = data[at:at + 4], struct.unpack_from("<I", data, at + 4)[0]
        if at + 8 + size > end:
            raise ValueError(f"read_mjpeg: chunk {tag!r} of {what} at byte {at} runs past its parent")
        yield tag, at + 8, size
        at += 8 + size + (size & 1)


def read_mjpeg(path: str) -> Tuple[float, List[bytes]]:
    """A Motion-JPEG AVI -> ``(fps, frames)``: dwRate / dwScale of the video stream and the bytes of every ``00dc`` / ``00db`` chunk of
    ``movi`` in file order.  Raises ``ValueError`` for a file that is no RIFF AVI, has no MJPG video stream, or whose chunk sizes or
    index do not agree with its contents."""
    with open(path, "rb") as f:
        data = f.read()
    if len(data) < 12 or data[:4] != b"RIFF" or data[8:12] != b"AVI ":
        raise ValueError("read_mjpeg: not a RIFF AVI file")
    end = 8 + struct.unpack_from("<I", data, 4)[0]
    if end > len(data):
        raise ValueError(f"read_mjpeg: the RIFF size says {end} bytes, the file has {len(data)}")
    fps, frames, offsets, index = None, None, [], None
    for tag, at, size in _chunks(data, 12, end, "RIFF"):
        kind = data[at:at + 4] if tag == b"LIST" and size >= 4 else None
        if kind == b"hdrl":
            for t2, a2, s2 in _chunks(data, at + 4, at + size, "hdrl"):
                if t2 == b"LIST" and data[a2:a2 + 4] == b"strl":
                    for t3, a3, s3 in _chunks(data, a2 + 4, a2 + s2, "strl"):
                        if t3 == b"strh" and s3 >= 48 and data[a3:a3 + 4] == b"vids" and fps is None:
                            if data[a3 + 4:a3 + 8].upper() != b"MJPG":
                                raise ValueError(f"read_mjpeg: the video stream is {data[a3 + 4:a3 + 8]!r}, not MJPG")
                            scale, rate = struct.unpack_from("<II", data, a3 + 20)
                            if scale == 0 or rate == 0:
                                raise ValueError("read_mjpeg: dwRate / dwScale is zero")
                            fps = rate / scale
        elif kind == b"movi":
            frames = []
            for t2, a2, s2 in _chunks(data, at + 4, at + size, "movi"):
                if t2 in (b"00dc", b"00db"):
                    frames.append(data[a2:a2 + s2])
                    offsets.append((a2 - 8 - at, s2))
        elif tag == b"idx1":
            index = [struct.unpack_from("<4sIII", data, at + 16 * i) for i in range(size // 16)]
    if fps is None or frames is None:
        raise ValueError("read_mjpeg: no MJPG video stream or no movi list")
    if index is not None:
        video = [(off, size) for ckid, _, off, size in index if ckid in (b"00dc", b"00db")]
        if video != offsets:
            raise ValueError("read_mjpeg: idx1 does not agree with the chunks of movi")
    return fps, frames
