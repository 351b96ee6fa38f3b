"""The random appearance augmentation (the reference's ``data: inplane_normalize: False``, the value its
``config/shape_and_pose_net.yaml`` ships): ``pose_img_inplane`` as a randomly transformed copy of the pose image, drawn afresh for
every sample.  What the reference does per image on the host with torchvision and Pillow --

* DeepFashion (data/deepfashion.py:92-108, :170-181): ``ToPILImage -> RandomAffine(degrees 30, translate (0.3, 0), scale (0.7, 1),
  BILINEAR, fill white) -> Resize(S, BICUBIC) -> ToTensor -> x * 2 - 1``;
* Market (data/market.py:52-64, :118-126): ``ToPILImage -> Pad(S // 2, reflect) -> RandomRotation(90, BILINEAR) ->
  CenterCrop(128) -> Resize(S, BICUBIC) -> ToTensor -> x * 2 - 1``

-- runs here as one HIP launch (csrc/appearance_aug.hip, include/vunet_appearance_aug.h) on the uint8 stack of the raw-frame route
(image_input.py), followed by that route's bicubic launches where the window is not the output size.  The bytes are Pillow's:
its bilinear ``Image.transform(AFFINE)`` is plain double arithmetic with a truncating store, and the kernel restates it exactly
(pinned against Pillow 12.2.0, tests/golden/g22_appearance_aug.npz).  The reflect pad is virtual and only the cropped window is
computed.

* ``affine_images``      uint8 stack [N, Hmax, Wmax, 3] + one output-to-input affine per image -> images and a per-image status;
* ``rotation_matrix``    Pillow's own ``Image.rotate`` matrix (pinned: the fixture calls ``Image.rotate``);
* ``inverse_affine``     torchvision 0.4.x's ``_get_inverse_affine_matrix`` with shear 0 (ASSUMED, see below);
* ``AppearanceAug``      the two datasets' random draws on the host (ASSUMED, see below) and their launch arguments;
* ``batch_appearance``   the trainers' hook: makes ``pose_img_inplane`` where a batch brings ``pose_img_u8`` + ``pose_img_aug``.

ASSUMED, NOT PINNED: torchvision is no dependency of this package and is absent where the fixtures are written.  The order in which
``RandomAffine.get_params`` / ``RandomRotation.get_params`` consume ``random.uniform``, ``_get_inverse_affine_matrix`` and
``CenterCrop``'s origin ``int(round((H - crop) / 2.))`` are restated from torchvision 0.4.x's source as published; nothing checks
them against torchvision itself.  What IS pinned is everything from the matrix on: the transform, the reflect pad, the crop window,
``Image.rotate``'s matrix and the resize.

The random parameters are drawn on the host; the JPEG decode and the dataset plumbing stay there too.  There is no CPU path."""
from __future__ import annotations

import math
import random
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import image_input
from .ops import _call, _p, _stream

KINDS = ("deepfashion", "market")
MAX_SIDE = image_input.MAX_SIDE          # N, Hmax, Wmax, oh, ow of one call (grid dimensions)
MAX_PAD = 1 << 20
MAX_ORIGIN = 1 << 24

_whole_hw: Dict[tuple, torch.Tensor] = {}


def rotation_matrix(w: int, h: int, angle: float) -> list:
    """The output-to-input matrix of Pillow's ``Image.rotate(angle)`` (no ``expand``, no ``center``, no ``translate``) on a
    ``w x h`` image: the angle mod 360, the centre ``(w / 2, h / 2)``, ``cos`` / ``sin`` of ``-radians(angle)`` rounded to 15
    decimals, the translation composed as Pillow composes it.  (Pillow short-cuts 0, 180 and, on square images, +-90 degrees to a
    copy / transpose; this matrix gives the same bytes.)"""
    angle = float(angle) % 360.0
    cx, cy = w / 2.0, h / 2.0
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    x, y = -cx, -cy
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += cx
    m[5] += cy
    return m


def inverse_affine(center: Tuple[float, float], angle: float, translate: Tuple[float, float], scale: float) -> list:
    """torchvision 0.4.x's ``_get_inverse_affine_matrix(center, angle, translate, scale, shear=0)`` (ASSUMED, module docstring):
    with ``a = radians(angle)`` and ``s = 1 / scale``, ``M = s / (cos^2 a + sin^2 a) * [cos a, sin a, 0, -sin a, cos a, 0]``, then
    ``M2 += M0 (-cx - tx) + M1 (-cy - ty)``, ``M2 += cx`` and ``M5`` alike, in that order."""
    a = math.radians(angle)
    s = 1.0 / scale
    d = math.cos(a) * math.cos(a) + math.sin(a) * math.sin(a)
    m = [math.cos(a), math.sin(a), 0, -math.sin(a), math.cos(a), 0]
    m = [s / d * v for v in m]
    m[2] += m[0] * (-center[0] - translate[0]) + m[1] * (-center[1] - translate[1])
    m[5] += m[3] * (-center[0] - translate[0]) + m[4] * (-center[1] - translate[1])
    m[2] += center[0]
    m[5] += center[1]
    return [float(v) for v in m]


def _hw_rows(hw) -> np.ndarray:
    a = np.asarray(hw.cpu().numpy() if torch.is_tensor(hw) else hw)
    if a.ndim != 2 or a.shape[1] != 2 or not np.issubdtype(a.dtype, np.integer) or (a.size and a.min() < 1):
        raise ValueError(f"hw: integer rows [N, 2] of (h, w) >= 1 expected, got {a.dtype} {a.shape}")
    return a.astype(np.int64)


class AppearanceAug:
    """The random draws of one dataset's augmentation, on the host, from one ``random.Random(seed)`` (ASSUMED draw order, module
    docstring), per image and in this order:

    * ``"deepfashion"``: ``angle = U(-30, 30)``, ``tx = round(U(-0.3 w, 0.3 w))``, ``ty = round(U(-0, 0))`` (drawn although it is
      0), ``scale = U(0.7, 1)``; the matrix is ``inverse_affine((w 0.5 + 0.5, h 0.5 + 0.5), angle, (tx, ty), scale)``.  Fill white,
      no pad, the window is the frame.
    * ``"market"``: ``angle = U(-90, 90)``; the matrix is ``rotation_matrix(w + 2 p, h + 2 p, angle)`` with the reflect pad
      ``p = size // 2`` (``size``: the trainers' ``spatial_size``).  Fill black, the window is the centre ``crop x crop`` of the
      padded image, origin ``int(round((H - crop) / 2.))`` (torchvision's ``CenterCrop``).  The frames of a batch are one size."""

    def __init__(self, kind: str, seed: Optional[int] = None, crop: int = 128, size: Optional[int] = None):
        kind = str(kind).lower()
        if kind not in KINDS:
            raise ValueError(f"appearance_aug: one of {KINDS} expected, got {kind!r}")
        self.kind, self.crop, self.size = kind, int(crop), None if size is None else int(size)
        self.rng = random.Random(seed)

    def __repr__(self):
        return f"AppearanceAug({self.kind!r}, crop={self.crop}, size={self.size})"

    def pad(self, size: Optional[int] = None) -> int:
        if self.kind != "market":
            return 0
        size = self.size if size is None else int(size)
        if size is None:
            raise ValueError("AppearanceAug('market'): the reflect pad is size // 2 -- pass size")
        return size // 2

    def draw(self, hw, size: Optional[int] = None) -> np.ndarray:
        """One matrix per row (h, w) of ``hw`` -> float64 [N, 6], output-to-input, for ``affine_images``."""
        rows, p, u = [], self.pad(size), self.rng.uniform
        for h, w in _hw_rows(hw).tolist():
            if self.kind == "deepfashion":
                angle = u(-30.0, 30.0)
                tx = round(u(-0.3 * w, 0.3 * w))
                ty = round(u(-0.0 * h, 0.0 * h))
                scale = u(0.7, 1.0)
                rows.append(inverse_affine((w * 0.5 + 0.5, h * 0.5 + 0.5), angle, (tx, ty), scale))
            else:
                rows.append(rotation_matrix(w + 2 * p, h + 2 * p, u(-90.0, 90.0)))
        return np.asarray(rows, dtype=np.float64).reshape(-1, 6)

    def launch_args(self, size: Optional[int] = None, frame_hw: Optional[Tuple[int, int]] = None) -> dict:
        """The uniform arguments of ``affine_images``: ``dict(pad, origin, out_hw, fill)``.  ``frame_hw`` = (h, w) of the frames
        (Market needs it for the crop origin; DeepFashion's window is the frame -- None: the whole stack slot)."""
        if self.kind == "deepfashion":
            return dict(pad=0, origin=(0, 0), out_hw=None if frame_hw is None else (int(frame_hw[0]), int(frame_hw[1])),
                        fill=(255, 255, 255))
        if frame_hw is None:
            raise ValueError("AppearanceAug('market').launch_args: frame_hw = (h, w) of the frames is needed for the crop origin")
        p = self.pad(size)
        H, W = int(frame_hw[0]) + 2 * p, int(frame_hw[1]) + 2 * p
        origin = (int(round((W - self.crop) / 2.)), int(round((H - self.crop) / 2.)))   # (x, y)
        return dict(pad=p, origin=origin, out_hw=(self.crop, self.crop), fill=(0, 0, 0))


def check_mats(mats, n: int) -> torch.Tensor:
    """Host matrices (NumPy array, list or CPU tensor) -> a CPU float64 [N, 6] tensor; ValueError where they are not N rows of six
    finite floating-point coefficients."""
    m = np.asarray(mats.numpy() if torch.is_tensor(mats) else mats)
    if m.shape != (n, 6) or not np.issubdtype(m.dtype, np.floating):
        raise ValueError(f"mats: floating-point rows [{n}, 6] (output-to-input affines) expected, got {m.dtype} {m.shape}")
    m = m.astype(np.float64)
    if not np.isfinite(m).all():
        i = int(np.flatnonzero(~np.isfinite(m).all(axis=1))[0])
        raise ValueError(f"mats row {i} = {m[i].tolist()} is not finite")
    return torch.from_numpy(np.ascontiguousarray(m))


def check_hw(hw, n: int, hmax: int, wmax: int) -> torch.Tensor:
    """Host frame sizes -> a CPU int32 [N, 2] tensor; ValueError where they are not N rows (h, w) with ``1 <= h <= Hmax``,
    ``1 <= w <= Wmax``."""
    a = np.asarray(hw.numpy() if torch.is_tensor(hw) else hw)
    if a.shape != (n, 2) or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"hw: integer rows [{n}, 2] of (h, w) expected, got {a.dtype} {a.shape}")
    a = a.astype(np.int64)
    bad = (a[:, 0] < 1) | (a[:, 0] > hmax) | (a[:, 1] < 1) | (a[:, 1] > wmax)
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise ValueError(f"hw row {i} = {a[i].tolist()} breaks the contract 1 <= h <= {hmax} and 1 <= w <= {wmax}")
    return torch.from_numpy(a.astype(np.int32))


def _whole(n: int, hmax: int, wmax: int, device: torch.device) -> torch.Tensor:
    """``hw=None`` -- every frame its whole stack slot -- on the device, uploaded once per shape."""
    key = (n, hmax, wmax, str(device))
    if key not in _whole_hw:
        _whole_hw[key] = torch.tensor([[hmax, wmax]] * n, dtype=torch.int32).reshape(n, 2).to(device)
    return _whole_hw[key]


def affine_images(frames, mats, hw=None, out_hw: Optional[Tuple[int, int]] = None, origin: Tuple[int, int] = (0, 0), pad: int = 0,
                  fill: Sequence[int] = (0, 0, 0), size: Optional[int] = None, out_u8: bool = False):
    """uint8 frames [N, Hmax, Wmax, 3] (RGB interleaved; a device tensor, or a CPU tensor / NumPy array that is uploaded) and one
    output-to-input affine per image, ``mats`` [N, 6] float64 -> ``(images, status)``: per image, bit for bit,

        ``Image.fromarray(np.pad(frame, pad, "reflect")).transform((W, H), AFFINE, mat, BILINEAR, fillcolor=fill)``

    cut to the window of ``out_hw`` = (oh, ow) pixels at ``origin`` = (ox, oy) (default: the whole padded stack slot; the window may
    hang over the image -- fill), then -- where ``size`` is given and is not the window -- ``Resize([size, size], BICUBIC)`` through
    ``image_input.frames_to_images``, then ``ToTensor -> x * 2 - 1``: fp32 [N, 3, oh, ow] (or [N, 3, size, size]) in [-1, 1], or
    with ``out_u8`` the bytes [N, oh, ow, 3].  status int32 [N]: 1 for an image whose matrix is not finite or whose ``hw`` row breaks
    ``1 <= h <= Hmax``, ``1 <= w <= Wmax`` (its image is all fill).

    ``hw`` [N, 2] int32 rows (h, w): the valid frame inside each stack slot (None: the whole slot).  Host ``mats`` / ``hw`` are
    checked here (ValueError) and uploaded; device tensors are taken as they are and checked by the kernel (status).  One launch
    on the current stream (plus the three of the resize), no synchronisation."""
    f = image_input._frames_device(frames, None)
    n, hmax, wmax = (int(v) for v in f.shape[:3])
    pad, ox, oy = int(pad), int(origin[0]), int(origin[1])
    oh, ow = (hmax + 2 * pad, wmax + 2 * pad) if out_hw is None else (int(out_hw[0]), int(out_hw[1]))
    fill = tuple(int(c) for c in fill)
    if not (n <= MAX_SIDE and 1 <= hmax <= MAX_SIDE and 1 <= wmax <= MAX_SIDE and 1 <= oh <= MAX_SIDE and 1 <= ow <= MAX_SIDE):
        raise ValueError(f"1 <= Hmax, Wmax, oh, ow <= {MAX_SIDE} and N <= {MAX_SIDE} expected, got window {(oh, ow)}, stack {tuple(f.shape)}")
    if not (0 <= pad <= MAX_PAD and abs(ox) <= MAX_ORIGIN and abs(oy) <= MAX_ORIGIN):
        raise ValueError(f"0 <= pad <= {MAX_PAD} and |origin| <= {MAX_ORIGIN} expected, got pad {pad}, origin {(ox, oy)}")
    if len(fill) != 3 or not all(0 <= c <= 255 for c in fill):
        raise ValueError(f"fill: three bytes expected, got {fill}")
    if torch.is_tensor(mats) and mats.is_cuda:
        if tuple(mats.shape) != (n, 6) or mats.dtype != torch.float64:
            raise ValueError(f"mats: float64 [{n}, 6] expected on the device, got {mats.dtype} {tuple(mats.shape)}")
        m = mats.to(f.device).contiguous()
    else:
        m = check_mats(mats, n).to(f.device, non_blocking=True)
    if hw is None:
        s = _whole(n, hmax, wmax, f.device)
    elif torch.is_tensor(hw) and hw.is_cuda:
        if tuple(hw.shape) != (n, 2) or hw.dtype != torch.int32:
            raise ValueError(f"hw: int32 [{n}, 2] expected on the device, got {hw.dtype} {tuple(hw.shape)}")
        s = hw.to(f.device).contiguous()
    else:
        s = check_hw(hw, n, hmax, wmax).to(f.device, non_blocking=True)
    resize = size is not None and (int(size), int(size)) != (oh, ow)
    as_u8 = out_u8 or resize
    out = torch.empty((n, oh, ow, 3) if as_u8 else (n, 3, oh, ow), device=f.device, dtype=torch.uint8 if as_u8 else torch.float32)
    status = torch.empty(n, device=f.device, dtype=torch.int32)
    if n:
        with torch.cuda.device(f.device):
            _call("vunet_appearance_affine", _p(f), _p(s), _p(m), n, hmax, wmax, pad, ox, oy, oh, ow, fill[0], fill[1], fill[2],
                  None if as_u8 else _p(out), _p(out) if as_u8 else None, _p(status), _stream())
            if resize:   # Resize after the augmentation: the bilinear bytes through the existing bicubic route
                out, _ = image_input.frames_to_images(out, None, int(size), out_u8=out_u8)
    return out, status


def to_device(batch: dict, device) -> dict:
    """``batch`` with the augmentation's inputs (``pose_img_u8``, ``pose_img_aug``, ``pose_img_hw``) as device tensors, host
    values checked first -- what a step recorded into a hipGraph needs (the matrices are one more static device input).  The batch
    itself where it brings no ``pose_img_aug``, carries a ready ``pose_img_inplane``, or everything is on the device already."""
    if "pose_img_aug" not in batch or "pose_img_u8" not in batch or "pose_img_inplane" in batch:
        return batch
    on_dev = lambda v: torch.is_tensor(v) and v.is_cuda   # noqa: E731
    u8, mats, hw = batch["pose_img_u8"], batch["pose_img_aug"], batch.get("pose_img_hw")
    if on_dev(u8) and on_dev(mats) and (hw is None or on_dev(hw)):
        return batch
    out = dict(batch)
    if not on_dev(u8):
        out["pose_img_u8"] = u8 = image_input._frames_device(u8, device)
    n, hmax, wmax = (int(v) for v in u8.shape[:3])
    if not on_dev(mats):
        out["pose_img_aug"] = check_mats(mats, n).to(device, non_blocking=True)
    if hw is not None and not on_dev(hw):
        out["pose_img_hw"] = check_hw(hw, n, hmax, wmax).to(device, non_blocking=True)
    return out


def batch_appearance(batch: dict, size: int, aug_args) -> Dict[str, torch.Tensor]:
    """The appearance input a batch leaves to the package: where ``batch`` has ``pose_img_u8`` and ``pose_img_aug`` ([N, 6]
    float64, e.g. ``AppearanceAug.draw``; ``pose_img_hw`` optional) and no ``pose_img_inplane``, ``{"pose_img_inplane": images,
    "pose_img_inplane_status": status}`` of ``affine_images(..., size=size)``.  ``aug_args``: an ``AppearanceAug`` (its
    ``launch_args(size, stack slot)``) or the dict of uniform arguments itself.  An empty dict -- no launch, nothing touched --
    otherwise.  A batch with ``pose_img_geom`` as well raises ValueError: the reference's crop route (Human3.6m) has no augmentation."""
    if "pose_img_u8" not in batch or "pose_img_aug" not in batch or "pose_img_inplane" in batch:
        return {}
    if "pose_img_geom" in batch:
        raise ValueError("pose_img_aug with pose_img_geom: the crop route has no appearance augmentation in the reference")
    if aug_args is None:
        raise ValueError("the batch brings pose_img_aug but no augmentation is configured (data.appearance_aug: 'deepfashion' | 'market')")
    u8 = batch["pose_img_u8"]
    if isinstance(aug_args, AppearanceAug):
        aug_args = aug_args.launch_args(size, tuple(int(v) for v in u8.shape[1:3]))
    images, status = affine_images(u8, batch["pose_img_aug"], batch.get("pose_img_hw"), size=size, **aug_args)
    return {"pose_img_inplane": images, "pose_img_inplane_status": status}
