"""The person-box crop of the reference's ``run_inference`` (experiments/shape_and_pose_net.py:888-891, lib/utils.py:530-585): every
reconstructed and every transferred image is cut to the bounding rectangle of its valid keypoints and resized back to
``spatial_size`` before the Inception score ("IS on masks").  The reference takes ``cv2.boundingRect`` per image on the host (a
``kp.cpu().numpy()`` round trip each) and then ``kornia.crop_and_resize``; here both are HIP launches (csrc/person_crop.hip,
include/vunet_person_crop.h) and nothing leaves the device:

* ``keypoint_boxes``         keypoints [N, J, 2 or 3] in pixels -> boxes [N, 4] int32 (x, y, w, h) and ``valid`` [N] int32;
* ``crop_and_resize``        images + boxes -> [N, Ch, size, size], bilinear with zero padding;
* ``inception_input_boxes``  images + boxes -> the [N, 3, 299, 299] Inception input of those crops in ONE launch, bit-identical to
                             ``models.inception.inception_input(crop_and_resize(...), mode)``.

Two points are ASSUMED, not pinned, because OpenCV and kornia are no dependencies of this package:
``cv2.boundingRect`` on float points is taken to be ``x = floor(min x)``, ``w = floor(max x) - x + 1`` (the rule
``image_input.bounding_box`` assumes too); and ``sampling="reference"`` restates kornia 0.2.0 (pixel coordinates normalised with
``2 / (W - 1)``) over torch 1.3.1's ``F.grid_sample`` default ``align_corners=False``, which samples pixel
``u W / (W - 1) - 0.5`` where the box geometry intends ``u``.  ``sampling="exact"`` samples ``u`` itself.  There is no CPU path.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from .ops import _call, _p, _stream

SAMPLING = {"reference": _lib.const("VUNET_CROP_REFERENCE"), "exact": _lib.const("VUNET_CROP_EXACT")}
INPUT_MODES = {"none": 0, "transform": 1, "fid": 2}
INCEPTION_SIZE = _lib.const("VUNET_INCEPTION_SIZE")


def _sampling(sampling: str) -> int:
    if sampling not in SAMPLING:
        raise ValueError(f"sampling: 'reference' or 'exact' expected, got {sampling!r}")
    return SAMPLING[sampling]


def keypoint_boxes(kps: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """keypoints [N, J, C] (C = 2 or 3; x, y first) in pixels -> (``boxes`` [N, 4] int32 (x, y, w, h), ``valid`` [N] int32).
    A keypoint counts only if all of its C coordinates are > 0 (lib/utils.py:562); an image without one gets ``valid = 0`` and the
    box (0, 0, 0, 0).  One launch, no host synchronisation."""
    if not kps.is_cuda:
        raise RuntimeError("keypoints must be on the GPU (hand-written gfx950 kernels; no CPU fallback)")
    if kps.dim() != 3 or kps.shape[2] not in (2, 3) or kps.shape[1] < 1:
        raise ValueError(f"keypoints [N, J >= 1, 2 or 3] expected, got {tuple(kps.shape)}")
    k = kps.detach().to(torch.float32).contiguous()
    n = int(k.shape[0])
    boxes = torch.empty(n, 4, device=k.device, dtype=torch.int32)
    valid = torch.empty(n, device=k.device, dtype=torch.int32)
    if n:
        with torch.cuda.device(k.device):
            _call("vunet_kp_boxes", _p(k), n, int(k.shape[1]), int(k.shape[2]), _p(boxes), _p(valid), _stream())
    return boxes, valid


def _boxes_device(img: torch.Tensor, boxes: torch.Tensor, valid: Optional[torch.Tensor]):
    n = int(img.shape[0])
    if not (img.is_cuda and boxes.is_cuda and (valid is None or valid.is_cuda)):
        raise RuntimeError("the person crop needs device tensors (hand-written gfx950 kernels; no CPU fallback)")
    if tuple(boxes.shape) != (n, 4) or boxes.dtype != torch.int32:
        raise ValueError(f"boxes: int32 [{n}, 4] rows (x, y, w, h) expected, got {boxes.dtype} {tuple(boxes.shape)}")
    if valid is None:
        valid = torch.ones(n, device=img.device, dtype=torch.int32)
    elif tuple(valid.shape) != (n,) or valid.dtype != torch.int32:
        raise ValueError(f"valid: int32 [{n}] expected, got {valid.dtype} {tuple(valid.shape)}")
    return boxes.contiguous(), valid.contiguous()


def crop_and_resize(img: torch.Tensor, boxes: torch.Tensor, size: int, valid: Optional[torch.Tensor] = None,
                    sampling: str = "reference") -> torch.Tensor:
    """``kornia.crop_and_resize(img, corners of the boxes, (size, size))``: img [N, Ch, Hs, Ws] fp32 and boxes [N, 4] int32
    (x, y, w, h) -> [N, Ch, size, size], bilinear, a tap outside the image contributing 0; ``valid`` [N] int32 (None: every box
    counts), 0 fills the crop with zeros.  ``sampling``: see the module header.  One launch on the current stream."""
    if img.dim() != 4:
        raise ValueError(f"img [N, Ch, Hs, Ws] expected, got {tuple(img.shape)}")
    mode = _sampling(sampling)
    if int(size) < 2:
        raise ValueError(f"size >= 2 expected, got {size}")
    boxes, valid = _boxes_device(img, boxes, valid)
    x = img.detach().to(torch.float32).contiguous()
    n, ch = int(x.shape[0]), int(x.shape[1])
    out = torch.empty(n, ch, int(size), int(size), device=x.device, dtype=torch.float32)
    if n:
        with torch.cuda.device(x.device):
            _call("vunet_box_crop", _p(x), n, ch, int(x.shape[2]), int(x.shape[3]), _p(boxes), _p(valid), int(size), mode, _p(out),
                  _stream())
    return out


def inception_input_boxes(img: torch.Tensor, boxes: torch.Tensor, crop_size: int, valid: Optional[torch.Tensor] = None,
                          mode: str = "none", sampling: str = "reference") -> torch.Tensor:
    """img [N, 3, Hs, Ws] + boxes -> [N, 3, 299, 299]: the crop to ``crop_size`` and the bilinear resize of
    ``models.inception.inception_input`` (with its ``mode`` affine) in one launch; the crop is never stored."""
    if img.dim() != 4 or img.shape[1] != 3:
        raise ValueError(f"img [N, 3, Hs, Ws] expected, got {tuple(img.shape)}")
    smp = _sampling(sampling)
    if int(crop_size) < 2:
        raise ValueError(f"crop_size >= 2 expected, got {crop_size}")
    boxes, valid = _boxes_device(img, boxes, valid)
    x = img.detach().to(torch.float32).contiguous()
    n = int(x.shape[0])
    y = torch.empty(n, 3, INCEPTION_SIZE, INCEPTION_SIZE, device=x.device, dtype=torch.float32)
    if n:
        with torch.cuda.device(x.device):
            _call("vunet_inception_input_boxes", _p(x), n, int(x.shape[2]), int(x.shape[3]), _p(boxes), _p(valid), int(crop_size), smp,
                  INPUT_MODES[mode], _p(y), _stream())
    return y
