"""The part-normalised appearance input (the reference's ``data: inplane_normalize: True``, its DeepFashion and Market runs): the
appearance encoder sees one square crop per body part, each warped out of the image by a perspective transform built from the
keypoints, stacked on the channel axis -- the reference's ``pose_img_inplane``.  What the reference does per image on the host
with OpenCV (data/base_dataset.py:685-725, lib/utils.py:70-232) runs here as two HIP launches (csrc/inplane.hip,
include/vunet_inplane.h):

* ``part_transforms``  keypoints -> one homography per (image, part), destination -> source, float64, and a ``valid`` flag;
* ``part_crops``       image + keypoints -> [N, 3 P, s_out, s_out]: the transforms, then every part warped bilinearly with the
                       border replicated; an absent part is ``-1.0`` (the reference's black uint8 crop after ``ToTensor``, ``* 2 - 1``).

Three deviations from the reference, all deliberate: the four source points stay float64 (the reference
rounds them to float32 before ``cv2.getPerspectiveTransform``); a degenerate quad makes the part absent (OpenCV returns
whatever its decomposition yields); the float image is warped (OpenCV warps the uint8 image with source coordinates quantised to
1/32 px and rounds the result to uint8).  OpenCV is not a dependency and parity with it is not pinned.  There is no CPU path.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple, Union

import torch

from . import _lib
from .ops import _call, _p, _stream

T2P, T3P, T4P, T5P = (_lib.const("VUNET_INPLANE_" + k) for k in ("T2P", "T3P", "T4P", "T5P"))   # the kind is the number of joints it reads
MAX_IDS, MAX_PARTS = _lib.const("VUNET_INPLANE_MAX_IDS"), _lib.const("VUNET_INPLANE_MAX_PARTS")
BATCH_KEY = "inplane_keypoints"          # [N, J, 2] (x, y) pixel coordinates of batch["pose_img"]


class PartModel:
    """A name and a list of parts ``(kind, joint ids)`` -- the reference's ``JointModel.norm_T`` with the joints each builder
    reads spelled out:

    * ``T4P``: the four body joints in the order of ``JointModel.body`` (lib/utils.py:136-147);
    * ``T5P``: right hip, right shoulder, neck, left shoulder, left hip (:70-133);
    * ``T3P``: right shoulder, left shoulder, head (``rshoulder``, ``lshoulder``, ``headup``, :150-192);
    * ``T2P``: the limb's two joints (the ``ids`` of ``partial(t2p, ids=...)``, :195-232).

    The tables the kernels read are uploaded once per device (``tables``)."""

    def __init__(self, name: str, parts: Sequence[Tuple[int, Sequence[int]]]):
        parts = [(int(k), tuple(int(j) for j in ids)) for k, ids in parts]
        if not 1 <= len(parts) <= MAX_PARTS:
            raise ValueError(f"1..{MAX_PARTS} parts expected, got {len(parts)}")
        for k, ids in parts:
            if k not in (T2P, T3P, T4P, T5P):
                raise ValueError(f"part kind must be T2P, T3P, T4P or T5P, got {k}")
            if len(ids) != k or min(ids) < 0:
                raise ValueError(f"a part of kind T{k}P reads {k} joints with ids >= 0, got {ids}")
        self.name, self.parts = str(name), tuple(parts)
        self.n_parts, self.min_joints = len(parts), 1 + max(max(ids) for _, ids in parts)
        self._tables: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}

    def tables(self, device) -> Tuple[torch.Tensor, torch.Tensor]:
        """(kinds [P] int32, ids [P, MAX_IDS] int32, unused slots -1) on ``device``, uploaded on first use."""
        key = str(torch.device(device))
        if key not in self._tables:
            kinds = torch.tensor([k for k, _ in self.parts], dtype=torch.int32)
            ids = torch.tensor([list(i) + [-1] * (MAX_IDS - len(i)) for _, i in self.parts], dtype=torch.int32)
            self._tables[key] = (kinds.to(device), ids.to(device))
        return self._tables[key]

    def __repr__(self):
        return f"PartModel({self.name!r}, {self.n_parts} parts)"


# data/market.py:45 (norm_T) with body / rshoulder / lshoulder / headup of :25-32 -- beside lib.utils.MARKET_JOINT_MODEL
MARKET_PARTS = PartModel("Market", [(T4P, (8, 9, 3, 2)), (T3P, (8, 9, 13)), (T2P, (0, 1)), (T2P, (1, 2)), (T2P, (6, 7)), (T2P, (7, 8)),
                                    (T2P, (3, 4)), (T2P, (4, 5)), (T2P, (9, 10)), (T2P, (10, 11))])
# data/deepfashion.py:61-72 (norm_T) with body / rshoulder / lshoulder / headup of :26-33 -- beside lib.utils.DEEPFASHION_JOINT_MODEL
DEEPFASHION_PARTS = PartModel("DeepFashion", [(T4P, (8, 2, 5, 11)), (T3P, (2, 5, 0)), (T2P, (2, 3)), (T2P, (3, 4)), (T2P, (5, 6)),
                                              (T2P, (6, 7)), (T2P, (8, 9)), (T2P, (9, 10)), (T2P, (11, 12)), (T2P, (12, 13))])
_BY_DATASET = {"market": MARKET_PARTS, "deepfashion": DEEPFASHION_PARTS}


def part_model(parts: Union[PartModel, str, Sequence]) -> PartModel:
    """A ``PartModel`` as it is, a dataset name ("Market", "DeepFashion") or a user list of ``(kind, joint ids)``."""
    if isinstance(parts, PartModel):
        return parts
    if isinstance(parts, str):
        if parts.lower() not in _BY_DATASET:
            raise ValueError(f"no shipped part model for dataset {parts!r} (Market, DeepFashion): pass a PartModel or a part list")
        return _BY_DATASET[parts.lower()]
    return PartModel("user", parts)


def _kps_device(kps: torch.Tensor, parts: PartModel) -> torch.Tensor:
    if not kps.is_cuda:
        raise RuntimeError("keypoints must be on the GPU (hand-written gfx950 kernels; no CPU fallback)")
    if kps.dim() != 3 or kps.shape[2] != 2 or kps.shape[1] < parts.min_joints:
        raise ValueError(f"keypoints [N, J >= {parts.min_joints}, 2] expected for {parts!r}, got {tuple(kps.shape)}")
    return kps.detach().to(torch.float32).contiguous()


def part_transforms(kps: torch.Tensor, parts, s_out: int, oh: float):
    """keypoints [N, J, 2] (x, y) in pixels -> (``Minv`` [N, P, 9] float64: row-major 3x3, crop pixel -> image pixel;
    ``src_points`` [N, P, 4, 2] float64: the quad's corners in the builder's order; ``valid`` [N, P] int32: 0 for an absent part,
    whose ``Minv`` is zeros).  ``oh`` is the image height the T2P leg fallback draws down to (the reference passes
    ``spatial_size``).  One launch, no host synchronisation."""
    parts = part_model(parts)
    k = _kps_device(kps, parts)
    n, p = int(k.shape[0]), parts.n_parts
    if int(s_out) < 1:
        raise ValueError(f"s_out >= 1 expected, got {s_out}")
    minv = torch.empty(n, p, 9, device=k.device, dtype=torch.float64)
    src = torch.empty(n, p, 4, 2, device=k.device, dtype=torch.float64)
    valid = torch.empty(n, p, device=k.device, dtype=torch.int32)
    if n:
        kinds, ids = parts.tables(k.device)
        _call("vunet_inplane_transforms", _p(k), n, int(k.shape[1]), _p(kinds), _p(ids), p, int(s_out), float(oh), _p(minv), _p(src),
              _p(valid), _stream())
    return minv, src, valid


def warp_parts(img: torch.Tensor, minv: torch.Tensor, valid: torch.Tensor, s_out: int, absent: float = -1.0) -> torch.Tensor:
    """The warp alone: img [N, 3, Hs, Ws] fp32, ``minv`` [N, P, 9] float64 and ``valid`` [N, P] int32 (from ``part_transforms`` or
    computed elsewhere) -> [N, 3 P, s_out, s_out] fp32."""
    if not (img.is_cuda and minv.is_cuda and valid.is_cuda):
        raise RuntimeError("warp_parts needs device tensors (hand-written gfx950 kernels; no CPU fallback)")
    if img.dim() != 4 or img.shape[1] != 3:
        raise ValueError(f"img [N, 3, Hs, Ws] expected, got {tuple(img.shape)}")
    n, p = int(img.shape[0]), int(minv.shape[1]) if minv.dim() == 3 else -1
    if tuple(minv.shape) != (n, p, 9) or tuple(valid.shape) != (n, p) or minv.dtype != torch.float64 or valid.dtype != torch.int32:
        raise ValueError(f"minv [{n}, P, 9] float64 and valid [{n}, P] int32 expected, got {tuple(minv.shape)} {minv.dtype} and "
                         f"{tuple(valid.shape)} {valid.dtype}")
    if not 1 <= p <= MAX_PARTS or int(s_out) < 1 or n > 65535:
        raise ValueError(f"1..{MAX_PARTS} parts, s_out >= 1 and at most 65535 images expected, got P = {p}, s_out = {s_out}, N = {n}")
    x = img.detach().to(torch.float32).contiguous()
    out = torch.empty(n, 3 * p, int(s_out), int(s_out), device=x.device, dtype=torch.float32)
    if n:
        _call("vunet_inplane_warp", _p(x), n, int(x.shape[2]), int(x.shape[3]), _p(minv.contiguous()), _p(valid.contiguous()), p,
              int(s_out), float(absent), _p(out), _stream())
    return out


def part_crops(img: torch.Tensor, kps: torch.Tensor, parts, s_out: int, oh: Optional[float] = None, absent: float = -1.0) -> torch.Tensor:
    """``pose_img_inplane`` of the reference: img [N, 3, Hs, Ws] (values as the step gets them, [-1, 1]) and its keypoints
    [N, J, 2] -> [N, 3 P, s_out, s_out], part p in channels 3p .. 3p+2, an absent part filled with ``absent``.  ``oh`` defaults to
    the image height.  Two launches on the current stream; nothing is differentiated (the input of the appearance encoder is data)."""
    if img.dim() != 4 or kps.dim() != 3 or img.shape[0] != kps.shape[0]:
        raise ValueError(f"img [N, 3, Hs, Ws] and keypoints [N, J, 2] expected, got {tuple(img.shape)} and {tuple(kps.shape)}")
    minv, _, valid = part_transforms(kps.to(img.device), parts, s_out, float(img.shape[2]) if oh is None else oh)
    return warp_parts(img, minv, valid, s_out, absent)


def configured_parts(data_cfg: dict) -> Optional[PartModel]:
    """The part model of a ``data`` config section: ``data["inplane_parts"]`` (a ``PartModel``, a dataset name or a part list) or
    the shipped one of ``data["dataset"]``; None where ``inplane_normalize`` is off or no model is known."""
    if not data_cfg.get("inplane_normalize", False):
        return None
    if data_cfg.get("inplane_parts") is not None:
        return part_model(data_cfg["inplane_parts"])
    return _BY_DATASET.get(str(data_cfg.get("dataset", "")).lower())


def batch_crops(batch: dict, parts: Optional[PartModel], s_out: int, oh: float) -> Optional[torch.Tensor]:
    """The crops of ``batch["pose_img"]`` where the caller left them to the package: ``parts`` known (``inplane_normalize`` set), no
    ``pose_img_inplane`` in the batch and ``batch["inplane_keypoints"]`` present.  None otherwise: the caller's path of before."""
    if parts is None or "pose_img_inplane" in batch or BATCH_KEY not in batch:
        return None
    return part_crops(batch["pose_img"], batch[BATCH_KEY], parts, s_out, oh)
