"""The raw-frame input route: decoded uint8 RGB frames in, the fp32 ``[N, 3, S, S]`` images of the trainers (``pose_img``,
``app_img``) out, on the GPU.  What the reference does per image on the host -- the crop around the keypoints with the border
reflected (data/base_dataset.py:281-315, :461-489) and ``ToPILImage -> Resize([S, S], BICUBIC) -> ToTensor -> x * 2 - 1``
(data/__init__.py:15-43) -- runs here as three HIP launches (csrc/image_input.hip, include/vunet_image_input.h): the resampling
tables, the horizontal pass, the vertical pass.  The bytes are Pillow's: its 8-bit resampler is integer arithmetic on 22-bit
fixed-point coefficients, and the kernels restate it exactly (pinned against Pillow 12.2.0, tests/golden/g19_image_input.npz).

* ``frames_to_images``  uint8 stack [N, Hmax, Wmax, 3] (+ one geometry row per image) -> images and a per-image status;
* ``stack_frames``      frames of mixed sizes -> one padded stack and their sizes;
* ``bounding_box``      keypoints -> the geometry row of the reference's square crop (``get_bounding_box``);
* ``batch_images``      the trainers' hook: makes ``pose_img`` / ``app_img`` where a batch brings ``pose_img_u8`` / ``app_img_u8``
                        -- or ``pose_img_jpeg`` / ``app_img_jpeg``, encoded streams that jpeg_decode.py decodes into such a stack.

The dataset plumbing stays on the host, and of the JPEG decode only the entropy walk (jpeg_decode.py).  There is no CPU path."""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from .ops import _call, _p, _stream

KEYS = ("pose_img", "app_img")           # batch[K + "_u8"] (+ batch[K + "_geom"]) makes batch[K]
MAX_SIDE = 65535                         # N, Hmax, Wmax, S of one call (grid dimensions)

_scratch: Dict[tuple, Tuple[torch.Tensor, ...]] = {}
_whole: Dict[tuple, torch.Tensor] = {}


def ksize_max(hmax: int, wmax: int, size: int) -> int:
    """The row length of the coefficient tables of a stack: Pillow's ``ksize`` for the larger side, ``ceil(2 max(1, in / S)) 2 + 1``
    with ``in / S`` as Pillow forms it (the size through float32).  It bounds the ksize of every window the contract admits."""
    scale = float(np.float32(max(hmax, wmax))) / size
    return int(math.ceil(2.0 * max(scale, 1.0))) * 2 + 1


def clear_scratch() -> None:
    """Drop the cached scratch (not while a recorded step that used it is still replayed: its launches hold the addresses)."""
    _scratch.clear()
    _whole.clear()


def _whole_frames(n: int, hmax: int, wmax: int, device: torch.device) -> torch.Tensor:
    """The geometry of ``geom=None`` -- every image its whole stack slot -- on the device, uploaded once per shape."""
    key = (n, hmax, wmax, str(device))
    if key not in _whole:
        _whole[key] = torch.tensor([[hmax, wmax, 0, 0, wmax, hmax]] * n, dtype=torch.int32).reshape(n, 6).to(device)
    return _whole[key]


def _scratch_for(n: int, hmax: int, wmax: int, size: int, device: torch.device):
    """(coef [2, N, S, kmax] int32, bounds [2, N, S, 2] int32, intermediate [N, Hmax, S, 3] uint8) of one stack shape, allocated
    once per shape, device and stream (two streams never share an intermediate)."""
    key = (n, hmax, wmax, size, str(device), _stream().value)
    if key not in _scratch:
        kmax = ksize_max(hmax, wmax, size)
        _scratch[key] = (torch.empty(2, n, size, kmax, device=device, dtype=torch.int32),
                         torch.empty(2, n, size, 2, device=device, dtype=torch.int32),
                         torch.empty(n, hmax, size, 3, device=device, dtype=torch.uint8))
    return _scratch[key]


def check_geom(geom, n: int, hmax: int, wmax: int) -> torch.Tensor:
    """Host geometry (NumPy array, list or CPU tensor) -> a CPU int32 [N, 6] tensor; ValueError where it is not N rows of
    (h, w, x0, y0, cw, ch) inside the contract ``1 <= h, ch <= Hmax``, ``1 <= w, cw <= Wmax``."""
    g = np.asarray(geom.numpy() if torch.is_tensor(geom) else geom)
    if g.shape != (n, 6) or not np.issubdtype(g.dtype, np.integer):
        raise ValueError(f"geom: integer rows [{n}, 6] of (h, w, x0, y0, cw, ch) expected, got {g.dtype} {g.shape}")
    g = g.astype(np.int64)
    if np.abs(g).max(initial=0) > 0x7FFFFFFF:
        raise ValueError("geom: values must fit int32")
    bad = (g[:, 0] < 1) | (g[:, 0] > hmax) | (g[:, 5] < 1) | (g[:, 5] > hmax) | (g[:, 1] < 1) | (g[:, 1] > wmax) | (g[:, 4] < 1) | \
          (g[:, 4] > wmax)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise ValueError(f"geom row {i} = {g[i].tolist()} breaks the contract 1 <= h, ch <= {hmax} and 1 <= w, cw <= {wmax} (a window "
                         f"larger than its frame needs a larger stack: stack_frames(..., hmax, wmax))")
    return torch.from_numpy(g.astype(np.int32))


def _frames_device(frames, device) -> torch.Tensor:
    f = torch.from_numpy(frames) if isinstance(frames, np.ndarray) else frames
    if not torch.is_tensor(f) or f.dtype != torch.uint8 or f.dim() != 4 or f.shape[3] != 3:
        raise ValueError(f"frames: uint8 [N, Hmax, Wmax, 3] expected, got {getattr(f, 'dtype', type(f))} {tuple(getattr(f, 'shape', ()))}")
    if not f.is_cuda:
        if device is None and not torch.cuda.is_available():
            raise RuntimeError("frames_to_images needs the GPU (hand-written gfx950 kernels; no CPU fallback)")
        f = f.to(device if device is not None else "cuda", non_blocking=True)
    return f.contiguous()


def frames_to_images(frames, geom=None, size: int = 256, out_u8: bool = False):
    """uint8 frames [N, Hmax, Wmax, 3] (RGB interleaved; a device tensor, or a CPU tensor / NumPy array that is uploaded to the
    current GPU) -> ``(images, status)``: images fp32 [N, 3, size, size] in [-1, 1], bit-identical to
    ``ToPILImage -> Resize([size, size], BICUBIC) -> ToTensor -> x * 2 - 1`` of each crop window, or with ``out_u8`` the resized
    bytes [N, size, size, 3]; status int32 [N], 1 for an image whose geometry row breaks the contract (its image is -1.0 / 0).

    ``geom`` [N, 6] int32 rows (h, w, x0, y0, cw, ch): the valid frame inside the stack and the crop window in frame coordinates,
    which may hang over the frame -- the border is reflected (cv2.BORDER_REFLECT).  None: whole frames.  Host geometry is checked
    here (ValueError) and uploaded; a device tensor is taken as it is and checked by the kernels (status).  Three launches on the
    current stream, no synchronisation; tables and the intermediate come from a cache per stack shape."""
    f = _frames_device(frames, None)
    n, hmax, wmax = (int(v) for v in f.shape[:3])
    size = int(size)
    if not (1 <= size <= MAX_SIDE and n <= MAX_SIDE and 1 <= hmax <= MAX_SIDE and 1 <= wmax <= MAX_SIDE):
        raise ValueError(f"1 <= size, Hmax, Wmax <= {MAX_SIDE} and N <= {MAX_SIDE} expected, got size {size}, stack {tuple(f.shape)}")
    if geom is None:
        g = _whole_frames(n, hmax, wmax, f.device)
    elif torch.is_tensor(geom) and geom.is_cuda:
        if tuple(geom.shape) != (n, 6) or geom.dtype != torch.int32:
            raise ValueError(f"geom: int32 [{n}, 6] expected on the device, got {geom.dtype} {tuple(geom.shape)}")
        g = geom.to(f.device).contiguous()
    else:
        g = check_geom(geom, n, hmax, wmax).to(f.device, non_blocking=True)
    out = torch.empty((n, size, size, 3) if out_u8 else (n, 3, size, size), device=f.device, dtype=torch.uint8 if out_u8 else torch.float32)
    status = torch.empty(n, device=f.device, dtype=torch.int32)
    if n:
        with torch.cuda.device(f.device):
            coef, bounds, inter = _scratch_for(n, hmax, wmax, size, f.device)
            kmax = int(coef.shape[3])
            _call("vunet_image_input_tables", _p(g), n, hmax, wmax, size, kmax, _p(coef), _p(bounds), _p(status), _stream())
            _call("vunet_image_input_resample", _p(f), _p(g), n, hmax, wmax, size, kmax, _p(coef), _p(bounds), _p(status), _p(inter),
                  None if out_u8 else _p(out), _p(out) if out_u8 else None, _stream())
    return out, status


def resample_tables(geom, n_hw: Tuple[int, int], size: int):
    """The tables alone, for inspection: geometry [N, 6] and the stack's (Hmax, Wmax) -> ``(coef [2, N, S, kmax], bounds
    [2, N, S, 2], status [N])`` int32, axis 0 horizontal (in = cw), axis 1 vertical (in = ch); ``bounds`` = (first source index, tap
    count), coefficients in 22-bit fixed point, zeros past the count.  A skipped axis (in == S) holds the identity tap."""
    hmax, wmax = int(n_hw[0]), int(n_hw[1])
    g = geom if torch.is_tensor(geom) and geom.is_cuda else \
        check_geom(geom, len(geom), hmax, wmax).to("cuda")
    n, kmax = int(g.shape[0]), ksize_max(hmax, wmax, int(size))
    coef = torch.empty(2, n, int(size), kmax, device=g.device, dtype=torch.int32)
    bounds = torch.empty(2, n, int(size), 2, device=g.device, dtype=torch.int32)
    status = torch.empty(n, device=g.device, dtype=torch.int32)
    with torch.cuda.device(g.device):
        _call("vunet_image_input_tables", _p(g.contiguous()), n, hmax, wmax, int(size), kmax, _p(coef), _p(bounds), _p(status), _stream())
    return coef, bounds, status


def stack_frames(frames: Sequence, hmax: Optional[int] = None, wmax: Optional[int] = None):
    """Frames [h_i, w_i, 3] uint8 (NumPy arrays or CPU tensors) of mixed sizes -> ``(stack, hw)``: one zero-padded CPU tensor
    [N, Hmax, Wmax, 3] and int32 [N, 2] (h, w).  ``hmax`` / ``wmax`` ask for a larger stack than the largest frame -- needed
    where a crop window is larger than its frame (the surplus is never read)."""
    arrs = [np.asarray(f.numpy() if torch.is_tensor(f) else f) for f in frames]
    if not arrs:
        raise ValueError("stack_frames: at least one frame expected")
    for i, a in enumerate(arrs):
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
            raise ValueError(f"frame {i}: uint8 [h, w, 3] expected, got {a.dtype} {a.shape}")
    hm, wm = max(a.shape[0] for a in arrs), max(a.shape[1] for a in arrs)
    hm, wm = max(hm, int(hmax or 0)), max(wm, int(wmax or 0))
    stack = np.zeros((len(arrs), hm, wm, 3), dtype=np.uint8)
    for i, a in enumerate(arrs):
        stack[i, :a.shape[0], :a.shape[1]] = a
    return torch.from_numpy(stack), torch.tensor([a.shape[:2] for a in arrs], dtype=torch.int32)


def bounding_box(kps, frame_hw, relax: float = 0.1) -> np.ndarray:
    """Keypoints [N, J, >= 2] (x, y in frame pixels; or [J, 2] for one image) and the frame sizes [N, 2] (h, w) (or one pair for
    all) -> geometry rows int32 [N, 6] (h, w, x0, y0, cw, ch): the reference's square crop around a pose.

    Restated from ``get_bounding_box`` (lib/utils.py:616-655).  With ``x, y, w, h = cv2.boundingRect(pts)`` and ``int`` truncating
    toward zero: for ``w >= h``: ``x_tl = int(x - relax w)``, ``x_br = int(x + (1 + relax) w)``, ``D = x_br - x_tl``,
    ``y_tl = int((2 y + h - D) / 2)``, ``y_br = int((2 y + h + D) / 2)``; for ``w < h`` the same with the axes exchanged.

    ``cv2.boundingRect`` on float points is ASSUMED to be ``x = floor(min x)``, ``w = floor(max x) - x + 1`` (and alike for y).
    OpenCV is no dependency of this package and the rule is not pinned against it.

    Why the row is ``x0 = x_tl, y0 = y_tl, cw = x_br - x_tl, ch = y_br - y_tl``.  ``_get_pose_img`` (data/base_dataset.py:294-306)
    pads the frame by ``pad_left = max(0, -x_tl)``, ``pad_right = max(0, x_br - W)``, ``pad_top = max(0, -y_tl)``,
    ``pad_bottom = max(0, y_br - H)`` with the border reflected, and slices rows ``y_tl + pad_top : y_br + pad_top + pad_bottom``,
    columns ``x_tl + pad_left : x_br + pad_left + pad_right`` of the padded frame ``P``.  With each pad on its own side,
    ``P[r, c] = frame[reflect(r - pad_top, H), reflect(c - pad_left, W)]`` and ``P`` has ``H + pad_top + pad_bottom`` rows.  The slice
    starts at ``r = y_tl + pad_top``, i.e. frame row ``y_tl``; its end exceeds the rows of ``P`` exactly when ``pad_bottom > 0``
    (then ``H + pad_bottom = y_br``) and NumPy clips it to ``y_br + pad_top``: in both cases ``y_br - y_tl`` rows.  So window pixel
    ``(i, j)`` is ``frame[reflect(y_tl + i, H), reflect(x_tl + j, W)]`` -- the source fetch of the kernels.

    One deviation, deliberate: the reference hands the four pads to ``cv2.copyMakeBorder`` in the order (left, right, top,
    bottom) where OpenCV takes (top, bottom, left, right).  For a box that hangs over the frame by different amounts on
    different sides its own crop is therefore shifted and can come out non-square; the derivation above (each pad on its own
    side, evidently the intent) is what this function and the kernels implement.  Boxes inside the frame are unaffected."""
    k = np.asarray(kps.detach().cpu().numpy() if torch.is_tensor(kps) else kps, dtype=np.float64)
    if k.ndim == 2:
        k = k[None]
    if k.ndim != 3 or k.shape[2] < 2 or k.shape[1] < 1:
        raise ValueError(f"keypoints [N, J, >= 2] expected, got {k.shape}")
    hw = np.asarray(frame_hw.cpu().numpy() if torch.is_tensor(frame_hw) else frame_hw, dtype=np.int64).reshape(-1, 2)
    hw = np.broadcast_to(hw, (k.shape[0], 2)) if hw.shape[0] == 1 else hw
    if hw.shape[0] != k.shape[0]:
        raise ValueError(f"one (h, w) per image expected, got {hw.shape[0]} for {k.shape[0]} images")
    rows = []
    for pts, (fh, fw) in zip(k, hw):
        x, y = int(math.floor(pts[:, 0].min())), int(math.floor(pts[:, 1].min()))
        w, h = int(math.floor(pts[:, 0].max())) - x + 1, int(math.floor(pts[:, 1].max())) - y + 1
        if w >= h:
            x_tl, x_br = int(x - relax * w), int(x + (1.0 + relax) * w)
            y_tl, y_br = int((2 * y + h - (x_br - x_tl)) / 2), int((2 * y + h + (x_br - x_tl)) / 2)
        else:
            y_tl, y_br = int(y - relax * h), int(y + (1.0 + relax) * h)
            x_tl, x_br = int((2 * x + w - (y_br - y_tl)) / 2), int((2 * x + w + (y_br - y_tl)) / 2)
        rows.append((int(fh), int(fw), x_tl, y_tl, x_br - x_tl, y_br - y_tl))
    return np.asarray(rows, dtype=np.int32)


def decode_jpeg(batch: dict, device=None, entropy: str = "host") -> dict:
    """``batch`` with its encoded inputs decoded: for K in ``pose_img``, ``app_img``, where ``batch[K + "_jpeg"]`` (a sequence of
    ``bytes``, baseline JPEG streams) is present and neither ``batch[K]`` nor ``batch[K + "_u8"]`` is, ``K + "_jpeg"`` is replaced by
    ``K + "_u8"`` -- the stack of ``jpeg_decode.decode_batch`` on ``device`` (None: the current GPU), valid until the next batch is
    decoded -- and, where the batch brings no ``K + "_geom"``, by whole-frame geometry rows from the decoded sizes.  (With
    ``pose_img_aug``, whose route takes no geometry, the sizes go to ``pose_img_hw`` instead.)  The batch itself where it brings
    no such key.  ``entropy``: ``decode_batch``'s keyword (``"device"``: the Huffman walk runs on the GPU too)."""
    out = None
    for key in KEYS:
        streams = batch.get(key + "_jpeg")
        if streams is None or key in batch or key + "_u8" in batch:
            continue
        from . import jpeg_decode
        out = dict(batch) if out is None else out
        if device is None or torch.device(device).type != "cuda":
            frames, hw = jpeg_decode.decode_batch(streams, tag=key, entropy=entropy)
        else:
            with torch.cuda.device(device):
                frames, hw = jpeg_decode.decode_batch(streams, tag=key, entropy=entropy)
        del out[key + "_jpeg"]
        out[key + "_u8"] = frames
        if key == "pose_img" and "pose_img_aug" in batch:
            out.setdefault("pose_img_hw", hw)
        elif key + "_geom" not in batch:
            h, w = hw[:, 0:1], hw[:, 1:2]
            out[key + "_geom"] = torch.cat([h, w, torch.zeros_like(h), torch.zeros_like(h), w, h], dim=1)
    return batch if out is None else out


def to_device(batch: dict, device, entropy: str = "host") -> dict:
    """``batch`` with its raw-frame inputs (``K_u8``, ``K_geom`` for K in ``pose_img``, ``app_img``) as device tensors, host
    geometry checked first -- what a step that is recorded into a hipGraph needs (its inputs are static device buffers).  The
    batch itself where it brings none of them or they are on the device already.  ``pose_img_aug`` / ``pose_img_hw`` (the
    matrices and frame sizes of appearance_aug.batch_appearance) are staged alike.  Encoded inputs (``K_jpeg``) are decoded first
    (``decode_jpeg``, which takes ``entropy``): a recorded step is replayed on the stack the decode has just filled."""
    batch = decode_jpeg(batch, device, entropy)
    out = None
    for key in KEYS:
        u8 = batch.get(key + "_u8")
        if u8 is None or key in batch:
            continue
        geom = batch.get(key + "_geom")
        host_u8 = not (torch.is_tensor(u8) and u8.is_cuda)
        host_geom = geom is not None and not (torch.is_tensor(geom) and geom.is_cuda)
        if not (host_u8 or host_geom):
            continue
        out = dict(batch) if out is None else out
        if host_u8:
            out[key + "_u8"] = _frames_device(u8, device)
        if host_geom:
            n, hmax, wmax = (int(v) for v in out[key + "_u8"].shape[:3])
            out[key + "_geom"] = check_geom(geom, n, hmax, wmax).to(device, non_blocking=True)
    batch = batch if out is None else out
    if "pose_img_aug" in batch:   # the appearance augmentation's matrices and frame sizes (appearance_aug.batch_appearance)
        from . import appearance_aug
        batch = appearance_aug.to_device(batch, device)
    return batch


def batch_images(batch: dict, size: int, entropy: str = "host") -> Dict[str, torch.Tensor]:
    """The images a batch leaves to the package: for K in ``pose_img``, ``app_img``, where ``batch[K + "_u8"]`` is present and
    ``batch[K]`` is not, ``K -> frames_to_images(batch[K + "_u8"], batch.get(K + "_geom"), size)[0]`` (and ``K + "_status"``).
    A batch that brings ``K + "_jpeg"`` instead has it decoded first (``decode_jpeg``, which takes ``entropy``).  An empty dict -- no launch, nothing
    touched -- for a batch of ready fp32 images."""
    batch = decode_jpeg(batch, entropy=entropy)
    made = {}
    for key in KEYS:
        if key + "_u8" in batch and key not in batch:
            made[key], made[key + "_status"] = frames_to_images(batch[key + "_u8"], batch.get(key + "_geom"), size)
    return made
