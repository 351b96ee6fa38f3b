"""Angle-space poses (the reference's ``keypoint_type: angle_world_expmap``, config/behavior_net.yaml): every pose is a root
translation plus one exponential-map rotation per joint, 99 numbers for H3.6M.  What the reference does with them on the host,
frame by frame and joint by joint, runs here as three HIP launches (csrc/pose_angles.hip, include/vunet_pose_angles.h):

* ``convert_to_3d``            angles -> joint positions through the kinematic chain (data/data_conversions_3d.py:1047-1066, ``fkl``
                               :608-668); with ``stats`` it takes the network's normalised output and un-normalises in the same launch;
* ``revert_coordinate_space``  the root's rotation and translation accumulated over a sequence (:671-703);
* ``euler_error``              ``mse_euler``'s per-sequence arithmetic (lib/metrics.py:321-357), ``EulerErrorTable`` its per-action lists.

The kernels compute in float64 and store fp32.  The skeleton is never part of this package: a ``KinematicTree`` is built from the
dict the reference's dataset holds.  There is no CPU path.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .ops import _call, _p, _stream

MAX_JOINTS = _lib.const("VUNET_POSE_MAX_JOINTS")
EULER_MAX_D, EULER_MAX_TD = _lib.const("VUNET_POSE_EULER_MAX_D"), _lib.const("VUNET_POSE_EULER_MAX_TD")   # one sequence's angles sit in LDS


class KinematicTree:
    """The kinematic tree as the reference's dataset holds it -- ``parent`` [J] (-1: the root), ``offset`` [J, 3] or [3 J] bone
    vectors, ``expmapInd`` J index triples into the pose vector, ``posInd["ids"]`` the root translation's three indices or None
    (``rotInd`` is for the Euler-angle format and is not read) -- checked and kept on the device.  The kernel walks the joints in
    index order, so every parent must come before its children: a tree that breaks this is rejected here."""

    def __init__(self, tree, device="cuda"):
        parent = np.asarray(tree["parent"]).astype(np.int64).reshape(-1)
        j = int(parent.size)
        if not 1 <= j <= MAX_JOINTS:
            raise ValueError(f"a tree of 1..{MAX_JOINTS} joints expected, got {j}")
        bad = [i for i, p in enumerate(parent.tolist()) if not (p == -1 or 0 <= p < i)]
        if bad:
            raise ValueError(f"parents must precede their children (parent[i] == -1 or 0 <= parent[i] < i): joints {bad} break this")
        offset = np.asarray(tree["offset"], dtype=np.float64)
        if offset.size != 3 * j:
            raise ValueError(f"offset: {j} x 3 bone vectors expected, got {offset.shape}")
        expmap = np.asarray([np.asarray(e) for e in tree["expmapInd"]]).astype(np.int64)
        if expmap.size != 3 * j:
            raise ValueError(f"expmapInd: {j} index triples expected, got {expmap.shape}")
        pos = tree.get("posInd")
        ids = pos.get("ids") if isinstance(pos, dict) else pos
        ids = None if ids is None else np.asarray(ids).astype(np.int64).reshape(-1)
        if ids is not None and ids.size != 3:
            raise ValueError(f"posInd: three indices expected, got {ids.tolist()}")
        idx = expmap.reshape(-1) if ids is None else np.concatenate([expmap.reshape(-1), ids])
        if idx.min() < 0:
            raise ValueError("negative index into the pose vector")
        self.n_joints, self.min_dim = j, int(idx.max()) + 1
        self.parent = torch.as_tensor(parent.astype(np.int32), device=device)
        self.offset = torch.as_tensor(offset.reshape(j, 3), device=device)
        self.expmap_ind = torch.as_tensor(expmap.reshape(j, 3).astype(np.int32), device=device)
        self.pos_ind = None if ids is None else torch.as_tensor(ids.astype(np.int32), device=device)

    @classmethod
    def of(cls, tree, device) -> "KinematicTree":
        return tree if isinstance(tree, cls) else cls(tree, device)


class AngleStats:
    """The dataset's normalisation statistics over the whole pose vector, on the device (``data_mean``, ``data_std``,
    ``dim_to_ignore``: what ``revert_output_format`` / ``unNormalizeData`` take, data/data_conversions_3d.py:178-211).  The
    statistics' dtype decides the precision of the un-normalisation, as it does in ``PoseCamera``: float32 arrays mean float32
    arithmetic, anything else float64.  Only the un-normalisation follows it; the kinematics and the Euler conversion after
    it are float64 either way."""

    def __init__(self, data_mean, data_std, dim_to_ignore=(), device="cuda"):
        mean, std = np.asarray(data_mean), np.asarray(data_std)
        if mean.shape != std.shape or mean.ndim != 1:
            raise ValueError(f"data_mean {mean.shape} and data_std {std.shape}: two vectors of the same length expected")
        self.f32_math = int(mean.dtype == np.float32 and std.dtype == np.float32)
        ignore = {int(d) for d in np.asarray(dim_to_ignore).reshape(-1)}
        use = [d for d in range(mean.size) if d not in ignore]
        if not use:
            raise ValueError("every dimension is ignored")
        pos = np.full(mean.size, -1, dtype=np.int32)
        pos[use] = np.arange(len(use), dtype=np.int32)
        self.dim, self.n_use = int(mean.size), len(use)
        self.pos_of_dim = torch.as_tensor(pos, device=device)
        self.mean = torch.as_tensor(mean.astype(np.float64), device=device)
        self.std = torch.as_tensor(std.astype(np.float64), device=device)

    @classmethod
    def from_dim_to_use(cls, data_mean, data_std, dim_to_use, device="cuda") -> "AngleStats":
        use = {int(d) for d in np.asarray(dim_to_use).reshape(-1)}
        return cls(data_mean, data_std, [d for d in range(int(np.asarray(data_mean).size)) if d not in use], device)


def _f32_device(name: str, t: torch.Tensor, like: torch.Tensor) -> torch.Tensor:
    if not t.is_cuda or t.device != like.device:
        raise RuntimeError(f"{name} must be on {like.device} (hand-written gfx950 kernels; no CPU fallback)")
    return t.to(torch.float32).contiguous()


def _f64_device(v, n: int, device) -> torch.Tensor:
    """``n`` doubles on ``device``: a device tensor stays there (no host round trip), anything else is copied up."""
    if isinstance(v, torch.Tensor) and v.is_cuda:
        return v.detach().to(device, torch.float64).reshape(n).contiguous()
    return torch.as_tensor(np.asarray(v.detach() if isinstance(v, torch.Tensor) else v, dtype=np.float64).reshape(n), device=device)


_horizon_tables: Dict[tuple, torch.Tensor] = {}


def _horizons_on(device, hz: Sequence[int]) -> torch.Tensor:
    """The horizon list as device int32, uploaded once per (device, list): a call after the first copies nothing."""
    key = (str(device), tuple(hz))
    if key not in _horizon_tables:
        if len(_horizon_tables) >= 64:
            _horizon_tables.clear()
        _horizon_tables[key] = torch.as_tensor(list(hz), dtype=torch.int32, device=device)
    return _horizon_tables[key]


def convert_to_3d(poses: torch.Tensor, tree, swap_yz: bool = False, stats: Optional[AngleStats] = None) -> torch.Tensor:
    """``convert_to_3d(poses_as_angles, kinematic_tree, swap_yz)`` of the reference: [..., D] un-normalised angle vectors ->
    [..., J, 3] fp32 joint positions; ``swap_yz`` stores (x, z, y).  With ``stats`` the poses are the network's NORMALISED
    [..., n_use] vectors and the un-normalisation happens in the same launch."""
    tree = KinematicTree.of(tree, poses.device)
    x = _f32_device("poses", poses, tree.parent)
    width = stats.n_use if stats is not None else x.shape[-1]
    dim = stats.dim if stats is not None else x.shape[-1]
    if x.dim() < 1 or x.shape[-1] != width or dim < tree.min_dim:
        raise ValueError(f"pose vectors of {width} numbers covering the tree's {tree.min_dim} dimensions expected, got {tuple(poses.shape)}")
    lead = tuple(x.shape[:-1])
    x = x.reshape(-1, width)
    t = x.shape[0]
    xyz = torch.empty(t, tree.n_joints, 3, device=x.device, dtype=torch.float32)
    if t:
        _call("vunet_pose_fk", _p(x), width, _p(stats.pos_of_dim) if stats is not None else None,
              _p(stats.mean) if stats is not None else None, _p(stats.std) if stats is not None else None,
              stats.f32_math if stats is not None else 0, dim, _p(tree.parent), _p(tree.offset), _p(tree.expmap_ind), _p(tree.pos_ind),
              tree.n_joints, int(bool(swap_yz)), _p(xyz), t, _stream())
    return xyz.reshape(lead + (tree.n_joints, 3))


def revert_coordinate_space(channels: torch.Tensor, R0, T0) -> torch.Tensor:
    """``revert_coordinate_space(channels, R0, T0)`` of the reference on [T, D] or [B, T, D] un-normalised poses: the root's
    rotation (dimensions 3..5) and translation (0..2) accumulated frame by frame from the start rotation ``R0`` [3, 3] and
    translation ``T0`` [3]; every sequence of a batch starts from the same (R0, T0).  fp32 out, the same shape."""
    if channels.dim() not in (2, 3) or channels.shape[-1] < 6:
        raise ValueError(f"channels: [T, D] or [B, T, D] with D >= 6 expected, got {tuple(channels.shape)}")
    if not channels.is_cuda:
        raise RuntimeError("channels must be on the GPU (hand-written gfx950 kernels; no CPU fallback)")
    ch = channels.to(torch.float32).contiguous()
    r0, t0 = _f64_device(R0, 9, ch.device), _f64_device(T0, 3, ch.device)
    out = torch.empty_like(ch)
    b, t, d = (1,) * (3 - ch.dim()) + tuple(ch.shape)
    if b and t:
        _call("vunet_pose_revert_root", _p(ch), _p(r0), _p(t0), _p(out), b, t, d, _stream())
    return out


def euler_error(rec: torch.Tensor, gt: torch.Tensor, stats: AngleStats, horizons: Sequence[int]) -> torch.Tensor:
    """``mse_euler``'s number for every sequence: rec, gt [B, T, n_use] normalised -> fp32 device tensor [B, n_horizons], no
    host sync.  Both are un-normalised, every exponential map (dimensions 3 on, three at a time) becomes Euler angles, and
    per horizon e the result is the mean over the first e frames of the Euclidean distance gt - rec.  Two things the reference
    does are kept as they are: the first six dimensions are zeroed in gt ONLY (the matching line for rec is commented out there),
    and the distance runs over the dimensions whose gt deviation over that sequence's frames exceeds 1e-4 -- the six zeroed
    ones never do, so rec's global translation and rotation do not count after all.  A horizon longer than the sequence
    averages the frames there are (the numpy slice)."""
    hz = [int(e) for e in horizons]
    if not hz or min(hz) < 1:
        raise ValueError(f"horizons: at least one, each >= 1, got {list(horizons)}")
    if rec.dim() != 3 or rec.shape != gt.shape or rec.shape[2] != stats.n_use:
        raise ValueError(f"rec and gt: [B, T, {stats.n_use}] expected, got {tuple(rec.shape)} and {tuple(gt.shape)}")
    if stats.dim % 3 or stats.dim < 6:
        raise ValueError(f"a pose of a translation plus exponential-map triples expected, got {stats.dim} dimensions")
    r, g = _f32_device("rec", rec, stats.mean), _f32_device("gt", gt, stats.mean)
    b, t = int(r.shape[0]), int(r.shape[1])
    out = torch.empty(b, len(hz), device=r.device, dtype=torch.float32)
    if b == 0:
        return out
    if t < 1:
        raise ValueError("sequences of at least one frame expected")
    if stats.dim > EULER_MAX_D or t * (stats.dim + 1) > EULER_MAX_TD:
        raise ValueError(f"T (D + 1) <= {EULER_MAX_TD} and D <= {EULER_MAX_D} expected (one sequence in LDS), got T = {t}, D = {stats.dim}")
    hd = _horizons_on(r.device, hz)
    _call("vunet_pose_euler_error", _p(r), _p(g), stats.n_use, _p(stats.pos_of_dim), _p(stats.mean), _p(stats.std), stats.f32_math,
          stats.dim, _p(hd), len(hz), _p(out), b, t, _stream())
    return out


class EulerErrorTable:
    """The reference's ``error_dict`` of ``mse_euler``: per action and horizon a list of per-sequence errors.  ``add`` keeps the
    device rows and decides on the host, from the action names alone, which sequences count -- the reference's cap: a sequence
    is skipped once its action's list ALREADY holds more than ``max_len`` entries, so a list ends with ``max_len + 1``.
    ``summary`` copies once and returns {action: {horizon: mean}} (NaN for an action without entries).  ``actions`` None: an
    action gets its lists when it is first seen (the reference's dict raises ``KeyError`` on a name it was not built with, and
    so does a table built with names)."""

    def __init__(self, actions: Optional[Sequence[str]], horizons: Sequence[int], max_len: int):
        self.open = actions is None
        self.actions, self.horizons, self.max_len = list(actions or ()), [int(e) for e in horizons], int(max_len)
        self.counts: Dict[str, int] = {a: 0 for a in self.actions}
        self._parts: List[torch.Tensor] = []
        self._rows: Dict[str, List[int]] = {a: [] for a in self.actions}
        self._n = 0

    def add(self, values: torch.Tensor, actions: Sequence[str]):
        if values.dim() != 2 or values.shape[1] != len(self.horizons) or values.shape[0] != len(actions):
            raise ValueError(f"values [{len(actions)}, {len(self.horizons)}] expected, got {tuple(values.shape)}")
        for i, a in enumerate(actions):
            if a not in self.counts:
                if not self.open:
                    raise KeyError(f"unknown action {a!r}")
                self.actions.append(a)
                self.counts[a], self._rows[a] = 0, []
            if self.counts[a] > self.max_len:
                continue
            self.counts[a] += 1
            self._rows[a].append(self._n + i)
        self._parts.append(values.detach())
        self._n += int(values.shape[0])

    def lists(self) -> Dict[str, np.ndarray]:
        """{action: float64 [entries, n_horizons]} (one device-to-host copy)."""
        flat = (torch.cat(self._parts).to(torch.float64).cpu().numpy() if self._parts else np.zeros((0, len(self.horizons))))
        return {a: flat[np.asarray(r, dtype=np.int64)] for a, r in self._rows.items()}

    def summary(self) -> Dict[str, Dict[int, float]]:
        return {a: {e: (float(np.mean(v[:, h])) if v.shape[0] else float("nan")) for h, e in enumerate(self.horizons)}
                for a, v in self.lists().items()}
