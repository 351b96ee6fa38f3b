"""Batched pose-sequence rendering (BASELINE config 5): 3-D poses -> camera projection -> stickman raster ->
``VunetAlter.transfer``, all on the GPU.

The reference renders a sequence frame by frame in Python (data/data_conversions_3d.py:1130-1185): per frame a
numpy projection (:588-605, :892-912), a CPU cv2 raster (lib/utils.py:325-512), an H2D copy, a batch-1
``synth_model.transfer`` and a D2H copy.  Here one raster launch draws every frame of the sequence and the
synthesis runs in batches; results are identical frame for frame (tests/test_hip_render.py).

``dtype="bf16"`` selects the precision BASELINE config 5 names for this loop; fp32 is the default.  The pose half of
``transfer`` (``du`` + ``dd``, the part that runs per frame) then executes on channel-blocked bf16 activations
(``render_blk.BlockedTransfer``, csrc/conv_blk.hip: bf16 operands and stored activations, fp32 accumulation);
``layout="nchw"`` keeps fp32 NCHW activations and only rounds the operands of the 3x3 convolutions
(``ops.inference_precision``, csrc/conv_bf16.hip) -- also what models outside ``BlockedTransfer.supported`` get.
``share_appearance=True`` encodes the appearance image once per sequence instead of once per frame (the
reference re-encodes the same image for every frame); with a fixed ``eps`` the frames are bit-identical either
way, without one the sequence shares a single posterior sample instead of drawing one per frame.
"""
from __future__ import annotations

from typing import Optional, Sequence

import torch

from . import ops
from .render_blk import engine_for
from .lib.utils import H36M_JOINT_MODEL, H36M_LIMBS, make_joint_img_batch, scale_img, skeleton_colors


def apply_affine_transform(x: torch.Tensor, m: torch.Tensor) -> torch.Tensor:
    """R x + t with M = [R, t] (3x4): data/data_conversions_3d.py:588-605.  x: [..., 3]."""
    ones = torch.ones_like(x[..., :1])
    return torch.cat([x, ones], dim=-1) @ m.transpose(-1, -2)


def camera_projection(poses: torch.Tensor, camera_parameters: Sequence[float]) -> torch.Tensor:
    """Pinhole projection with (f_x, x_0, f_y, y_0): data/data_conversions_3d.py:892-912.  poses: [..., J, 3]."""
    fx, x0, fy, y0 = [float(v) for v in camera_parameters]
    cam = torch.tensor([[fx, 0.0, x0], [0.0, fy, y0], [0.0, 0.0, 1.0]], dtype=poses.dtype, device=poses.device)
    p = poses / poses[..., -1:]
    return (p @ cam.T)[..., :-1]


def project_sequence(poses3d_world: torch.Tensor, extrinsics: torch.Tensor, intrinsics: Sequence[float],
                     image_size: Sequence[float], spatial_size: int) -> torch.Tensor:
    """[T, J, 3] world poses -> [T, J, 2] pixel keypoints at ``spatial_size`` (data/human36m.py:826-834)."""
    kps2d = camera_projection(apply_affine_transform(poses3d_world, extrinsics), intrinsics)
    scale = torch.tensor([float(spatial_size) / image_size[0], float(spatial_size) / image_size[1]],
                         dtype=kps2d.dtype, device=kps2d.device)
    return kps2d * scale


_side_streams = {}


def _side_stream(device):
    key = torch.device(device).index or 0
    if key not in _side_streams:
        _side_streams[key] = torch.cuda.Stream(device=device)
    return _side_streams[key]


@torch.no_grad()
def render_sequence(vunet, app_img: torch.Tensor, kps2d: torch.Tensor, spatial_size: Optional[int] = None,
                    joint_model=H36M_JOINT_MODEL, chunk: int = 16, as_uint8: bool = True, dtype: str = "f32",
                    share_appearance: bool = False, eps=None, layout: str = "auto"):
    """Render T frames: ``app_img`` [1, C, H, W] (appearance), ``kps2d`` [T, J, 2] pixel keypoints.

    Returns (frames, stickmen): frames uint8 [T, H, W, 3] as the reference builds them
    (``scale_img(rgb) * 255``, channels last, :1160-1167; values are clamped to [0, 255] before the cast) or
    the raw fp32 [T, 3, H, W] output when ``as_uint8`` is False; stickmen fp32 [T, 3, H, W] in [-1, 1].
    """
    size = spatial_size or vunet.spatial_size
    was_training = vunet.training
    vunet.eval()
    if layout not in ("auto", "nchw", "blk"):
        raise ValueError(f"unknown activation layout {layout!r}")
    engine = engine_for(vunet) if (dtype == "bf16" and layout != "nchw") else None
    if layout == "blk" and engine is None:
        raise ValueError("layout='blk' needs dtype='bf16' and a model BlockedTransfer.supported covers")
    outs = []
    if engine is not None and share_appearance and app_img.is_cuda:
        # One appearance encoding per sequence: ~100 batch-1 launches that leave most of the chip idle.  They run on a
        # side stream, next to the raster and the pose pyramid of the first chunk, which need nothing from them.
        main, side = torch.cuda.current_stream(), _side_stream(app_img.device)
        side.wait_stream(main)
        with torch.cuda.stream(side), ops.inference_precision(dtype), ops.prepacked(vunet):
            code = engine.encode_code(vunet.appearance_code(app_img, eps))
        stick = make_joint_img_batch((size, size), kps2d.to(app_img.device), joint_model, as_float=True)
        for s in range(0, stick.shape[0], chunk):
            feats = engine.pose_features(stick[s:s + chunk])
            if s == 0:
                main.wait_stream(side)
                for t in code:
                    t.record_stream(main)
            outs.append(engine.decode(feats, code))
    else:
        stick = make_joint_img_batch((size, size), kps2d.to(app_img.device), joint_model, as_float=True)
        # the weights do not change inside a sequence: fold / pack every layer once (two launches) instead of per call
        with ops.inference_precision(dtype), ops.prepacked(vunet):
            code = vunet.appearance_code(app_img, eps) if share_appearance else None
            if code is not None and engine is not None:
                code = engine.encode_code(code)
            for s in range(0, stick.shape[0], chunk):
                c = stick[s:s + chunk]
                if code is None:
                    e = None if eps is None else [t.expand(c.shape[0], -1, -1, -1).contiguous() for t in eps]
                    frame_code = vunet.appearance_code(app_img.expand(c.shape[0], -1, -1, -1).contiguous(), e)
                    if engine is not None:
                        frame_code = engine.encode_code(frame_code)
                else:
                    frame_code = code
                outs.append(engine.transfer_code(frame_code, c) if engine is not None
                            else vunet.transfer_code(frame_code, c))
    rgb = torch.cat(outs, dim=0)
    vunet.train(was_training)
    if as_uint8:
        rgb = (scale_img(rgb) * 255.0).clamp_(0.0, 255.0).permute(0, 2, 3, 1).to(torch.uint8)
    return rgb, stick


# ------------------------------------------------------------------------------------------------
# BASELINE config 5 end to end: flow sample -> pose_behavior_rnn decode -> per-frame VUnet render
# ------------------------------------------------------------------------------------------------
class PoseCamera:
    """What turns decoded pose vectors into pixel keypoints: the dataset's normalisation statistics
    (``data_mean`` / ``data_std`` / ``dim_to_use``, data/data_conversions_3d.py:361-385), a camera's extrinsics [3, 4] and
    intrinsics (f_x, x_0, f_y, y_0), the camera's image size (h, w) and the synthesis resolution.  Held on the device."""

    def __init__(self, data_mean, data_std, dim_to_use, extrinsics, intrinsics, image_size, spatial_size, device="cuda"):
        import numpy as np
        mean, std = np.asarray(data_mean), np.asarray(data_std)
        self.f32_math = int(mean.dtype == np.float32 and std.dtype == np.float32)
        self.mean = torch.as_tensor(mean.astype(np.float64), device=device)
        self.std = torch.as_tensor(std.astype(np.float64), device=device)
        use = np.asarray(sorted(int(d) for d in dim_to_use), dtype=np.int32)
        self.dims = torch.as_tensor(use, device=device)
        self.n_use, self.dim = int(use.size), int(mean.size)
        ext = np.asarray(extrinsics, dtype=np.float64).reshape(3, 4)
        fx, x0, fy, y0 = [float(v) for v in intrinsics]
        # (joint_scaling = size / image size, applied to (x, y) with image_size given as (s[0], s[1]): :1139-1140)
        scale = [float(spatial_size) / float(image_size[0]), float(spatial_size) / float(image_size[1])]
        self.cam = torch.as_tensor(np.concatenate([ext.reshape(-1), [fx, x0, fy, y0], scale]), device=device)
        self.cam_image = torch.as_tensor(np.concatenate([ext.reshape(-1), [fx, x0, fy, y0], [1.0, 1.0]]), device=device)
        self.spatial_size = int(spatial_size)
        self.image_size = (int(image_size[0]), int(image_size[1]))

    def project(self, poses: torch.Tensor) -> torch.Tensor:
        """[T, n_use] decoded (normalised) pose vectors -> [T, J, 2] pixel keypoints at the synthesis resolution."""
        return self._project(poses, self.cam)

    def project_image(self, poses: torch.Tensor) -> torch.Tensor:
        """[T, n_use] decoded (normalised) pose vectors -> [T, J, 2] keypoints in pixels of the camera's image (``image_size``):
        the projection launch of ``project`` with a scale of (1, 1) -- what ``skeleton_frames`` draws."""
        return self._project(poses, self.cam_image)

    def _project(self, poses: torch.Tensor, cam: torch.Tensor) -> torch.Tensor:
        ops._dev(poses)
        x = poses.reshape(-1, poses.shape[-1]).contiguous()
        if x.shape[1] != self.n_use:
            raise ValueError(f"pose vectors of {self.n_use} used dimensions expected, got {tuple(poses.shape)}")
        t, j = x.shape[0], self.dim // 3
        kps = torch.empty(t, j, 2, device=x.device, dtype=torch.float32)
        ops._call("vunet_seq_pose_project", ops._p(x), self.n_use, ops._p(self.dims), ops._p(self.mean), ops._p(self.std), self.dim,
                  self.f32_math, ops._p(cam), ops._p(kps), t, j, ops._stream())
        return kps


class AnglePoseCamera:
    """``PoseCamera`` for a model trained on ``keypoint_type: angle_world_expmap``: its pose vectors are a root translation and
    exponential-map joint rotations, not joint positions, so between the un-normalisation and the camera sits the forward
    kinematics over ``tree`` (a ``pose_angles.KinematicTree`` or the dict the reference's dataset holds), as the reference's
    ``convert_to_3d`` in front of its plots and videos (data/data_conversions_3d.py:1047-1066; ``swap_yz`` is its flag).  Two
    launches: un-normalise + kinematics (csrc/pose_angles.hip), then the projection kernel ``PoseCamera`` uses, on the 3-D joints."""

    def __init__(self, data_mean, data_std, dim_to_use, tree, extrinsics, intrinsics, image_size, spatial_size, swap_yz=False,
                 device="cuda"):
        import numpy as np
        from .pose_angles import AngleStats, KinematicTree
        self.stats = AngleStats.from_dim_to_use(data_mean, data_std, dim_to_use, device=device)
        self.tree = KinematicTree.of(tree, device)
        self.n_use, self.dim, self.swap_yz = self.stats.n_use, self.stats.dim, bool(swap_yz)
        j3 = 3 * self.tree.n_joints
        # the projection kernel un-normalises what it reads: identity statistics over the 3 J coordinates leave them as they are
        self._dims = torch.arange(j3, dtype=torch.int32, device=device)
        self._zero = torch.zeros(j3, dtype=torch.float64, device=device)
        self._one = torch.ones(j3, dtype=torch.float64, device=device)
        ext = np.asarray(extrinsics, dtype=np.float64).reshape(3, 4)
        fx, x0, fy, y0 = [float(v) for v in intrinsics]
        scale = [float(spatial_size) / float(image_size[0]), float(spatial_size) / float(image_size[1])]
        self.cam = torch.as_tensor(np.concatenate([ext.reshape(-1), [fx, x0, fy, y0], scale]), device=device)
        self.cam_image = torch.as_tensor(np.concatenate([ext.reshape(-1), [fx, x0, fy, y0], [1.0, 1.0]]), device=device)
        self.spatial_size = int(spatial_size)
        self.image_size = (int(image_size[0]), int(image_size[1]))

    def joints(self, poses: torch.Tensor) -> torch.Tensor:
        """[T, n_use] decoded (normalised) pose vectors -> [T, J, 3] world joint positions."""
        from .pose_angles import convert_to_3d
        ops._dev(poses)
        x = poses.reshape(-1, poses.shape[-1])
        if x.shape[1] != self.n_use:
            raise ValueError(f"pose vectors of {self.n_use} used dimensions expected, got {tuple(poses.shape)}")
        return convert_to_3d(x, self.tree, self.swap_yz, stats=self.stats)

    def project(self, poses: torch.Tensor) -> torch.Tensor:
        """[T, n_use] decoded (normalised) pose vectors -> [T, J, 2] pixel keypoints at the synthesis resolution."""
        return self._project(poses, self.cam)

    def project_image(self, poses: torch.Tensor) -> torch.Tensor:
        """``PoseCamera.project_image``: keypoints in pixels of the camera's image, behind the forward kinematics."""
        return self._project(poses, self.cam_image)

    def _project(self, poses: torch.Tensor, cam: torch.Tensor) -> torch.Tensor:
        xyz = self.joints(poses)
        t, j = xyz.shape[0], xyz.shape[1]
        kps = torch.empty(t, j, 2, device=xyz.device, dtype=torch.float32)
        ops._call("vunet_seq_pose_project", ops._p(xyz), 3 * j, ops._p(self._dims), ops._p(self._zero), ops._p(self._one), 3 * j, 0,
                  ops._p(cam), ops._p(kps), t, j, ops._stream())
        return kps


@torch.no_grad()
def behavior_video(flow, net, vunet, app_img: torch.Tensor, start_poses: torch.Tensor, length: int, camera: PoseCamera,
                   z: Optional[torch.Tensor] = None, start_frame: int = -1, joint_model=H36M_JOINT_MODEL, dtype: str = "bf16",
                   share_appearance: bool = True, chunk: int = 16, flow_weights: str = "f32"):
    """One synthesised sequence per row of ``start_poses`` [B, T, n_kps] (experiments/behavior_net.py:1173-1184 followed by
    data/data_conversions_3d.py:1130-1185): behaviour codes b = flow.reverse(z) with z ~ N(0, 1) (or the given ``z`` [B, C]),
    the decoder's roll-out of ``length`` poses from ``start_poses[:, start_frame]``, camera projection, stickman raster and
    ``VunetAlter.transfer`` of ``app_img`` [1, 3, H, W] for every frame.  ``flow_weights``: "f32" or "bf16", the flow's weight
    precision for this call (``seq.flow_weight_mode``; the flow's previous mode is restored afterwards).

    Returns (frames uint8 [B, length, H, W, 3], poses [B, length, n_kps], keypoints [B, length, J, 2])."""
    from .seq import flow_weight_mode
    bsz = start_poses.shape[0]
    if z is None:
        z = torch.randn(bsz, flow.in_channels, device=start_poses.device)
    with flow_weight_mode(flow, flow_weights):
        b = flow.reverse(z)
    b = b.reshape(bsz, -1)
    poses, *_ = net.generate_seq(b, start_poses, len=length, start_frame=start_frame % start_poses.shape[1])
    kps = camera.project(poses.reshape(bsz * length, -1)).reshape(bsz, length, -1, 2)
    frames = []
    for i in range(bsz):
        rgb, _ = render_sequence(vunet, app_img, kps[i], spatial_size=camera.spatial_size, joint_model=joint_model, chunk=chunk,
                                 dtype=dtype, share_appearance=share_appearance)
        frames.append(rgb)
    return torch.stack(frames), poses, kps


def _render_rows(vunet, app_img, poses: torch.Tensor, camera, joint_model, dtype, share_appearance, chunk):
    """poses [..., L, n] -> (frames uint8 [..., L, H, W, 3] or None, keypoints [..., L, J, 2]): one projection launch over every
    row, then ``render_sequence`` per row -- skipped without a synthesis model or an appearance image (the reference's
    pose-only branch)."""
    lead, length = poses.shape[:-2], poses.shape[-2]
    kps = camera.project(poses.reshape(-1, poses.shape[-1]))
    kps = kps.reshape(-1, length, kps.shape[-2], 2)
    frames = None
    if vunet is not None and app_img is not None:
        frames = torch.stack([render_sequence(vunet, app_img, k, spatial_size=camera.spatial_size, joint_model=joint_model,
                                              chunk=chunk, dtype=dtype, share_appearance=share_appearance)[0] for k in kps])
        frames = frames.reshape(*lead, *frames.shape[1:])
    return frames, kps.reshape(*lead, *kps.shape[1:])


@torch.no_grad()
def transfer_video(net, vunet, app_img: Optional[torch.Tensor], behavior_seq: torch.Tensor, start_poses: torch.Tensor, camera,
                   start_frame: int = 0, length: Optional[int] = None, sample: bool = False, eps: Optional[torch.Tensor] = None,
                   joint_model=H36M_JOINT_MODEL, dtype: str = "bf16", share_appearance: bool = True, chunk: int = 16):
    """Behaviour transfer (``visualize_transfer3d``, lib/logging.py:207-225, :331-370): the behaviour observed in
    ``behavior_seq`` [B, T, n] re-enacted from ``start_poses[:, start_frame]`` ([B, T', n]) and rendered with ``app_img``.

    The code is the posterior mean ``mu`` of ``net.infer_b(behavior_seq)``, or with ``sample`` the posterior sample
    ``eps * exp(logstd) + mu`` (``eps`` [B, H] given or drawn); ``length`` (default T) poses are rolled out and the start pose is
    put in front of them, as the reference does before it plots.

    Returns (frames uint8 [B, L + 1, H, W, 3], poses [B, L + 1, n], keypoints [B, L + 1, J, 2]); ``vunet`` or ``app_img`` None:
    no synthesis, frames is None."""
    if behavior_seq.dim() != 3 or start_poses.dim() != 3 or behavior_seq.shape[0] != start_poses.shape[0]:
        raise ValueError(f"transfer_video: behaviour {tuple(behavior_seq.shape)} and start poses {tuple(start_poses.shape)}: one "
                         "[B, T, n] row of each per video")
    if not net.ib:
        raise ValueError("transfer_video needs the behaviour net's information bottleneck (its posterior mean is the code)")
    start_frame = start_frame % start_poses.shape[1]
    length = behavior_seq.shape[1] if length is None else int(length)
    if sample and eps is None:
        eps = torch.randn(behavior_seq.shape[0], net.dim_hidden_b, device=behavior_seq.device)
    # the encoder alone: b = eps exp(logstd) + mu, and without noise b = mu (nothing is drawn for the mean)
    b, *_ = net.engine().infer_b(behavior_seq.contiguous(), eps.contiguous() if sample else None)
    xs, *_ = net.generate_seq(b, start_poses, len=length, start_frame=start_frame)
    poses = torch.cat([start_poses[:, start_frame].unsqueeze(1), xs], dim=1)
    frames, kps = _render_rows(vunet, app_img, poses, camera, joint_model, dtype, share_appearance, chunk)
    return frames, poses, kps


@torch.no_grad()
def interpolation_video(net, vunet, app_img: Optional[torch.Tensor], seq1: torch.Tensor, seq2: torch.Tensor, camera, steps=None,
                        joint_model=H36M_JOINT_MODEL, dtype: str = "bf16", share_appearance: bool = True, chunk: int = 16):
    """Latent interpolation (``latent_interpolate``, lib/logging.py:983-1040): a spherical walk between the behaviour codes of
    ``seq1`` and ``seq2`` ([P, T, n] each), in both directions, every step re-enacted from its direction's own start pose.

    The codes are the posterior means of both sequences; ``seq.slerp_codes`` interpolates all steps of both directions in one
    launch (``steps``: default ``np.linspace(0, 1, 6)``) and ONE roll-out decodes the 2 P S codes -- direction 0 from
    ``seq1[:, 0]``, direction 1 from ``seq2[:, 0]``, T poses each, the start pose in front.  The reference runs one host-side
    slerp and one batch-1 roll-out per step and direction.

    Returns (frames uint8 [2, P, S, T + 1, H, W, 3] or None, poses [2, P, S, T + 1, n], keypoints [2, P, S, T + 1, J, 2],
    codes [2, P, S, H])."""
    from .seq import slerp_codes
    if seq1.dim() != 3 or seq1.shape != seq2.shape:
        raise ValueError(f"interpolation_video: two [P, T, n] sequence tensors of one shape expected, got {tuple(seq1.shape)} and "
                         f"{tuple(seq2.shape)}")
    if not net.ib:
        raise ValueError("interpolation_video needs the behaviour net's information bottleneck (its posterior mean is the code)")
    pairs, t, n = seq1.shape
    mu = net.engine().infer_b(torch.cat([seq1, seq2]), None)[1]      # both sequences of every pair in one pass; no noise drawn
    codes = slerp_codes(mu[:pairs], mu[pairs:], steps)
    s = codes.shape[2]
    starts = torch.stack([seq1[:, :1], seq2[:, :1]]).unsqueeze(2).expand(2, pairs, s, 1, n).reshape(2 * pairs * s, 1, n)
    xs, *_ = net.generate_seq(codes.reshape(2 * pairs * s, -1), starts, len=t, start_frame=0)
    poses = torch.cat([starts, xs], dim=1).reshape(2, pairs, s, t + 1, n)
    frames, kps = _render_rows(vunet, app_img, poses, camera, joint_model, dtype, share_appearance, chunk)
    return frames, poses, kps, codes


@torch.no_grad()
def neighbour_video(net, vunet, app_img: Optional[torch.Tensor], behavior_seq: torch.Tensor, start_poses: torch.Tensor, bank, camera,
                    root: int, eps: Optional[torch.Tensor] = None, pose_space: bool = True, joint_model=H36M_JOINT_MODEL,
                    dtype: str = "bf16", share_appearance: bool = True, chunk: int = 16):
    """The four rows of the reference's ``nearest_neighbours`` figure (lib/figures.py:207-212, :255-278, :415-422), in its
    order: the behaviour sequence [B, T, n]; its nearest training sequence in code space (``bank.nearest_codes`` of its posterior
    mean); the generated sequence -- the posterior sample ``eps * exp(logstd) + mu`` (``eps`` [B, H] given or drawn, as the
    reference's ``net(poses_b, poses_in, len)`` draws it) rolled out for T poses from ``start_poses[:, 0]``, that pose in
    front; and the generated sequence's nearest training sequence in pose space (``bank.nearest_poses``, centred on joint
    ``root``).  ``bank``: a ``neighbours.TrainBank`` of [N, T + 1, n] sequences.

    Pose space compares joint positions (n = 3 J).  A model trained on ``angle_world_expmap`` poses (an ``AnglePoseCamera``) has
    none in its pose vectors -- the reference compares mismatched representations there -- so with ``pose_space`` that raises
    ``ValueError``; ``pose_space=False`` keeps the first three rows and returns None for the fourth.

    Returns (frames, poses, keypoints, found): three lists of four rows each (uint8 [B, L, H, W, 3], [B, L, n], [B, L, J, 2];
    ``frames`` is None without ``vunet`` or ``app_img``), and ``found`` = {"code_index", "code_distance", "pose_index",
    "pose_distance"}: int64 / float64 device tensors [B]."""
    if behavior_seq.dim() != 3 or start_poses.dim() != 3 or behavior_seq.shape[0] != start_poses.shape[0]:
        raise ValueError(f"neighbour_video: behaviour {tuple(behavior_seq.shape)} and start poses {tuple(start_poses.shape)}: one "
                         "[B, T, n] row of each per video")
    if not net.ib:
        raise ValueError("neighbour_video needs the behaviour net's information bottleneck (its posterior mean is the code)")
    if pose_space and isinstance(camera, AnglePoseCamera):
        raise ValueError("neighbour_video: the pose-space neighbour compares joint positions, and an angle_world_expmap model's pose "
                         "vectors are a root translation and joint rotations; pass pose_space=False to keep the code-space rows")
    bsz, t, _ = behavior_seq.shape
    if t + 1 != bank.sequences.shape[1]:
        raise ValueError(f"neighbour_video: a behaviour of T={t} frames needs a bank of T + 1={t + 1} frames, got {bank.sequences.shape[1]}")
    if eps is None:
        eps = torch.randn(bsz, net.dim_hidden_b, device=behavior_seq.device)
    b, mu, _, _ = net.engine().infer_b(behavior_seq.contiguous(), eps.contiguous())
    xs, *_ = net.generate_seq(b, start_poses, len=t, start_frame=0)
    generated = torch.cat([start_poses[:, :1], xs], dim=1)
    code_i, code_d = bank.nearest_codes(mu)
    rows = [behavior_seq, bank.sequences[code_i], generated, None]
    found = {"code_index": code_i, "code_distance": code_d, "pose_index": None, "pose_distance": None}
    if pose_space:
        found["pose_index"], found["pose_distance"] = bank.nearest_poses(generated, root)
        rows[3] = bank.sequences[found["pose_index"]]
    frames, kps = [], []
    for r in rows:
        f, k = (None, None) if r is None else _render_rows(vunet, app_img, r, camera, joint_model, dtype, share_appearance, chunk)
        frames.append(f)
        kps.append(k)
    if vunet is None or app_img is None:
        frames = None
    return frames, rows, kps, found


# ------------------------------------------------------------------------------------------------
# The pose-only branch: skeleton frames, crops, overlays and grids (data/data_conversions_3d.py:1068-1228
# project_onto_image_plane; lib/logging.py:1548-1868 make_eval_grid, :2680-2886 make_enrollment) on csrc/skeleton.hip
# ------------------------------------------------------------------------------------------------
def nearest_table(n_src: int, n_dst: int):
    """The source index of every output index of ``cv2.resize(..., interpolation=cv2.INTER_NEAREST)`` along one axis, int32
    [n_dst], built in float64 the way OpenCV 4.1.2's resizeNN does: ``ifx = 1 / (n_dst / n_src)``,
    ``min(floor(x * ifx), n_src - 1)``.  cv2 is absent here: the rule is restated from the published source, not pinned."""
    import numpy as np
    ifx = 1.0 / (float(n_dst) / n_src)
    return np.minimum(np.floor(np.arange(n_dst, dtype=np.float64) * ifx), n_src - 1).astype(np.int32)


def crop_spans(kps, image_size, target_size, target_width: int = 128, crop_joints=None, rgb_size: Optional[int] = None):
    """Host mirror of the kernel's crop rule (data/data_conversions_3d.py:1176-1184, :1194-1205): ``kps`` [F, J, 2] (numpy,
    image pixels) -> int64 [F, 2, 2], ``(min_x, max_x)`` of the skeleton strip and of the strip of an ``rgb_size``-wide
    synthesised frame (zeros without one).  float64, the joints added in index order.  Both strips scale x by the HEIGHT
    ratio, as upstream does (``img.shape[:2]`` over cv2's (w, h) ``dsize``; ``joint_scaling`` over ``(s[0], s[1])``)."""
    import numpy as np
    hs, (ht, wt), tw = int(image_size[0]), target_size, int(target_width)
    k = np.asarray(kps, dtype=np.float32).astype(np.float64)
    if crop_joints is not None:
        k = k[:, list(crop_joints)]
    skel_div = float(hs) / float(wt)
    rgb_mul = None if rgb_size is None else float(rgb_size) / float(hs)
    out = np.zeros((k.shape[0], 2, 2), dtype=np.int64)
    for f in range(k.shape[0]):
        s0 = s1 = 0.0
        for x in k[f, :, 0]:
            s0 += float(x) / skel_div
            if rgb_mul is not None:
                s1 += float(x) * rgb_mul
        o0 = int(min(max(0.0, s0 / k.shape[1] - tw // 2), wt - tw))
        out[f, 0] = (o0, o0 + tw)
        if rgb_mul is not None:
            o1 = int(min(max(0.0, s1 / k.shape[1] - tw // 2), int(rgb_size) - tw))
            out[f, 1] = (o1, o1 + tw)
    return out


_skeleton_tables = {}


def _skeleton_const(key, make):
    if key not in _skeleton_tables:
        _skeleton_tables[key] = make()
    return _skeleton_tables[key]


def _frame_strides(t: torch.Tensor, n_lead: int):
    """(frame stride, row stride) in bytes of a uint8 [*lead, H, W, 3] view whose pixels are packed and whose leading
    dimensions advance by one common stride."""
    if t.stride(-1) != 1 or t.stride(-2) != 3:
        raise ValueError("skeleton_frames: `out` must keep its pixels packed (strides 3 and 1 over the last two dimensions)")
    for i in range(n_lead - 1):
        if t.shape[i + 1] != 1 and t.stride(i) != t.stride(i + 1) * t.shape[i + 1]:
            raise ValueError("skeleton_frames: the leading dimensions of `out` must advance by one common stride")
    return (t.stride(n_lead - 1) if n_lead else 0), t.stride(-3)


@torch.no_grad()
def skeleton_frames(kps: torch.Tensor, image_size, limbs=H36M_LIMBS, colors=None, target_size=(256, 256), background: int = 255,
                    thickness: int = 3, crop: bool = False, target_width: int = 128, crop_joints=None,
                    rgb: Optional[torch.Tensor] = None, overlay: bool = False, out: Optional[torch.Tensor] = None):
    """Skeleton frames of ``kps`` [..., J, 2] (fp32 device tensor, (x, y) in pixels of an ``image_size`` = (h, w) camera image):
    what ``project_onto_image_plane`` returns first -- every pair of ``limbs`` a ``cv2.line`` of its ``colors`` entry
    (``skeleton_colors(None, overlay)`` by default) and of ``thickness`` on a ``background``-filled canvas of the image size,
    resized to ``target_size`` = (Ht, Wt) with INTER_NEAREST (None: the canvas itself).  One launch for every frame; the canvas
    is never built (csrc/skeleton.hip).  ``cv2.putText`` is left out.

    ``crop``: cut the ``target_width`` strip around the mean x of the joints (``crop_joints``: a subset, the ``kps_to_use`` of
    a small joint model) and also return the spans, int32 [..., 2, 2] -- ``(min_x, max_x)`` of the skeleton strip and of the
    rgb strip, the reference's ``masks``.  ``rgb``: synthesised frames, uint8 [..., Ht, S, 3] (square with ``crop``); cut to
    their own strip with ``crop``, and with ``overlay`` laid under the skeleton wherever that is (255, 255, 255).
    ``out``: a uint8 view [..., Ht, W', 3] to draw the skeleton frames into (packed pixels; any row stride, one frame stride).

    Returns the skeleton frames uint8 [..., Ht, Wt or target_width, 3]; with more than one result a tuple in the order
    (frames, spans if crop, rgb strips if rgb and crop, overlays if rgb and overlay)."""
    ops._dev(kps)
    if kps.dim() < 2 or kps.shape[-1] != 2:
        raise ValueError(f"skeleton_frames: keypoints [..., J, 2] expected, got {tuple(kps.shape)}")
    lead, j = tuple(kps.shape[:-2]), int(kps.shape[-2])
    k = kps.reshape(-1, j, 2).contiguous()
    f, dev = k.shape[0], k.device
    hs, ws = int(image_size[0]), int(image_size[1])
    limbs = tuple((int(a), int(b)) for a, b in limbs)
    colors = skeleton_colors(None, overlay) if colors is None else [[int(v) for v in c] for c in colors]
    if len(colors) == 1:
        colors = colors * len(limbs)
    if len(colors) != len(limbs):
        raise ValueError(f"skeleton_frames: {len(limbs)} limbs need as many colours, got {len(colors)}")
    if any(not (0 <= a < j and 0 <= b < j) for a, b in limbs):
        raise ValueError(f"skeleton_frames: a limb names a joint outside the {j} given")
    if any(not 0 <= v <= 255 for c in colors for v in c) or any(len(c) != 3 for c in colors):
        raise ValueError("skeleton_frames: colours are (r, g, b) bytes")
    ckey = tuple(tuple(c) for c in colors)
    d_limbs, d_colors = _skeleton_const(("limbs", limbs, ckey, dev), lambda: (
        torch.tensor(limbs, dtype=torch.int32, device=dev).reshape(-1, 2), torch.tensor(ckey, dtype=torch.uint8, device=dev).reshape(-1, 3)))
    if target_size is None:
        ht, wt, sy, sx = hs, ws, None, None
    else:
        ht, wt = int(target_size[0]), int(target_size[1])
        sy = _skeleton_const(("table", hs, ht, dev), lambda: torch.as_tensor(nearest_table(hs, ht), device=dev))
        sx = _skeleton_const(("table", ws, wt, dev), lambda: torch.as_tensor(nearest_table(ws, wt), device=dev))
    tw = int(target_width) if crop else 0
    if crop and not 1 <= tw <= wt:
        raise ValueError(f"skeleton_frames: a strip of {tw} columns does not fit frames {wt} wide")
    wo = tw if crop else wt
    d_cj, n_cj = None, 0
    if crop and crop_joints is not None:
        cj = tuple(int(c) for c in crop_joints)
        if not cj or any(not 0 <= c < j for c in cj):
            raise ValueError(f"skeleton_frames: crop_joints must name some of the {j} joints")
        d_cj, n_cj = _skeleton_const(("cj", cj, dev), lambda: torch.tensor(cj, dtype=torch.int32, device=dev)), len(cj)
    sw, r = 0, None
    if rgb is not None:
        if not rgb.is_cuda or rgb.dtype != torch.uint8 or tuple(rgb.shape[:-3]) != lead or rgb.shape[-1] != 3 or rgb.shape[-3] != ht:
            raise ValueError(f"skeleton_frames: rgb must be a uint8 device tensor [..., {ht}, S, 3] over the same frames, got "
                             f"{tuple(rgb.shape)} {rgb.dtype}")
        sw = int(rgb.shape[-2])
        if (crop and (sw != ht or sw < tw)) or (not crop and sw != wt):
            raise ValueError(f"skeleton_frames: rgb frames {tuple(rgb.shape[-3:])} do not match "
                             + (f"a square frame of at least {tw} columns" if crop else f"the {ht} x {wt} skeleton frames"))
        r = rgb.reshape(-1, ht, sw, 3).contiguous()
    if out is None:
        frames = torch.empty(*lead, ht, wo, 3, dtype=torch.uint8, device=dev)
    else:
        if not out.is_cuda or out.dtype != torch.uint8 or tuple(out.shape) != lead + (ht, wo, 3):
            raise ValueError(f"skeleton_frames: `out` must be a uint8 device tensor {lead + (ht, wo, 3)}, got {tuple(out.shape)} {out.dtype}")
        frames = out
    fs, rs = _frame_strides(frames, len(lead))
    span = torch.zeros(*lead, 2, 2, dtype=torch.int32, device=dev) if crop else None
    strip = torch.empty(*lead, ht, wo, 3, dtype=torch.uint8, device=dev) if (r is not None and crop) else None
    over = torch.empty(*lead, ht, wo, 3, dtype=torch.uint8, device=dev) if (r is not None and overlay) else None
    # upstream divides x by img.shape[0] / dsize[0] = Hs / Wt (cv2's dsize is (w, h)) and multiplies it by S / Hs
    ops._call("vunet_skeleton_raster", ops._p(k), f, j, ops._p(d_limbs), ops._p(d_colors), len(limbs), hs, ws, int(thickness),
              int(background), ops._p(sy), ops._p(sx), ht, wt, tw, ops._p(d_cj), n_cj, float(hs) / float(wt),
              (float(sw) / float(hs)) if sw else 0.0, ops._p(r), sw, ops._p(frames), fs, rs, ops._p(over), ops._p(strip),
              ops._p(span), ops._stream())
    res = [frames] + [t for t in (span, strip, over) if t is not None]
    return res[0] if len(res) == 1 else tuple(res)


def skeleton_video(poses, camera, **style):
    """The pose-only video of the ``poses`` [..., L, n] any of ``transfer_video`` / ``interpolation_video`` /
    ``neighbour_video`` / ``behavior_video`` returns (a list of such rows: a list, None entries kept): one
    ``camera.project_image`` launch, then ``skeleton_frames`` at the camera's ``image_size``; ``style``: its keyword arguments."""
    if isinstance(poses, (list, tuple)):
        return [None if p is None else skeleton_video(p, camera, **style) for p in poses]
    kps = camera.project_image(poses.reshape(-1, poses.shape[-1]))
    return skeleton_frames(kps.reshape(*poses.shape[:-1], kps.shape[-2], 2), camera.image_size, **style)


@torch.no_grad()
def transfer_grid(net, vunet, app_img: Optional[torch.Tensor], behaviors: torch.Tensor, starts: torch.Tensor, camera,
                  behavior_frames: Optional[torch.Tensor] = None, start_frame: int = 0, target_size=(256, 256),
                  joint_model=H36M_JOINT_MODEL, dtype: str = "bf16", share_appearance: bool = True, chunk: int = 16, **style):
    """The evaluation grid of ``make_eval_grid`` (lib/logging.py:1662-1790): ``behaviors`` [Nb, T, n] re-enacted from
    ``starts[:, start_frame]`` ([Ns, T', n]).  The codes are the posterior means (as ``transfer_video``); all Nb Ns of them are
    rolled out in ONE ``generate_seq`` batch, the start pose put in front, and the result cut to L = T frames, the length of
    the behaviour row (upstream's ``min_time``).  Layout, tiles of ``target_size`` = (Ht, Wt): the first column holds each
    start pose's first skeleton frame held still under a black tile; then one column per behaviour -- its own skeleton video
    on top, its re-enactment from every start pose below.  Every tile is drawn in place (``skeleton_frames(out=...)``).
    With ``vunet`` and ``app_img`` a second grid holds the synthesised frames (Ht = Wt = the synthesis size): ``behavior_frames``
    uint8 [Nb, L, Ht, Wt, 3] on top where given, white where not, and a white first column (the ground-truth stills upstream
    puts there are the caller's to read).  ``camera``: one camera, or Ns + 1 of them -- one per start pose, then the behaviour
    row's.  ``style``: ``skeleton_frames`` keywords other than crop / rgb / out.

    Returns (grid uint8 [L, (1 + Ns) Ht, (1 + Nb) Wt, 3], grid_rgb or None, poses [Nb, Ns, L, n])."""
    if behaviors.dim() != 3 or starts.dim() != 3 or behaviors.shape[-1] != starts.shape[-1]:
        raise ValueError(f"transfer_grid: behaviours [Nb, T, n] and start sequences [Ns, T', n] expected, got "
                         f"{tuple(behaviors.shape)} and {tuple(starts.shape)}")
    if not net.ib:
        raise ValueError("transfer_grid needs the behaviour net's information bottleneck (its posterior mean is the code)")
    if any(key in style for key in ("crop", "rgb", "out", "overlay")):
        raise ValueError("transfer_grid draws plain tiles: crop / rgb / overlay / out are not grid options")
    nb, t, n = behaviors.shape
    ns = starts.shape[0]
    cams = list(camera) if isinstance(camera, (list, tuple)) else [camera] * (ns + 1)
    if len(cams) != ns + 1:
        raise ValueError(f"transfer_grid: one camera or {ns + 1} (one per start pose, then the behaviour row's), got {len(cams)}")
    start_frame = start_frame % starts.shape[1]
    ht, wt = int(target_size[0]), int(target_size[1])
    mu = net.engine().infer_b(behaviors.contiguous(), None)[0]
    x0 = starts[:, start_frame]                                                  # [Ns, n]
    codes = mu.unsqueeze(1).expand(nb, ns, mu.shape[-1]).reshape(nb * ns, -1).contiguous()
    first = x0.unsqueeze(0).expand(nb, ns, n).reshape(nb * ns, 1, n).contiguous()
    if t > 1:
        xs, *_ = net.generate_seq(codes, first, len=t - 1, start_frame=0)
        poses = torch.cat([first, xs], dim=1)
    else:
        poses = first
    poses = poses.reshape(nb, ns, t, n)
    grid = torch.empty(t, (1 + ns) * ht, (1 + nb) * wt, 3, dtype=torch.uint8, device=behaviors.device)

    def tile(g, row, col):
        return g[:, row * ht:(row + 1) * ht, col * wt:(col + 1) * wt]

    tile(grid, 0, 0).zero_()
    for b in range(nb):
        kb = cams[ns].project_image(behaviors[b])
        skeleton_frames(kb, cams[ns].image_size, target_size=(ht, wt), out=tile(grid, 0, 1 + b), **style)
    for s in range(ns):
        ks = cams[s].project_image(poses[:, s].reshape(nb * t, n)).reshape(nb, t, -1, 2)
        for b in range(nb):
            skeleton_frames(ks[b], cams[s].image_size, target_size=(ht, wt), out=tile(grid, 1 + s, 1 + b), **style)
        tile(grid, 1 + s, 0).copy_(tile(grid, 1 + s, 1)[:1].expand(t, ht, wt, 3))
    grid_rgb = None
    if vunet is not None and app_img is not None:
        if any(c.spatial_size != ht or c.spatial_size != wt for c in cams[:ns]):
            raise ValueError(f"transfer_grid: synthesised tiles are {cams[0].spatial_size} pixels square, the grid's tiles {ht} x {wt}")
        grid_rgb = torch.full_like(grid, 255)
        if behavior_frames is not None:
            if tuple(behavior_frames.shape) != (nb, t, ht, wt, 3) or behavior_frames.dtype != torch.uint8:
                raise ValueError(f"transfer_grid: behavior_frames must be uint8 {(nb, t, ht, wt, 3)}, got {tuple(behavior_frames.shape)}")
            for b in range(nb):
                tile(grid_rgb, 0, 1 + b).copy_(behavior_frames[b])
        for s in range(ns):
            ks = cams[s].project(poses[:, s].reshape(nb * t, n)).reshape(nb, t, -1, 2)
            for b in range(nb):
                rgb, _ = render_sequence(vunet, app_img, ks[b], spatial_size=cams[s].spatial_size, joint_model=joint_model,
                                         chunk=chunk, dtype=dtype, share_appearance=share_appearance)
                tile(grid_rgb, 1 + s, 1 + b).copy_(rgb)
    return grid, grid_rgb, poses


def enrollment(frames: torch.Tensor, step: int = 4) -> torch.Tensor:
    """The still image of ``make_enrollment`` (lib/logging.py:2823-2828): every ``step``-th frame of ``frames`` [L, H, W, 3] side
    by side -> [H, ceil(L / step) W, 3]; rows of videos [R, L, H, W, 3] are stacked below each other -> [R H, ..., 3]."""
    if frames.dim() not in (4, 5) or step < 1:
        raise ValueError(f"enrollment: frames [L, H, W, 3] or [R, L, H, W, 3] and a positive step expected, got {tuple(frames.shape)}")
    rows = frames.unsqueeze(0) if frames.dim() == 4 else frames
    return torch.cat([torch.cat(list(v[::step]), dim=1) for v in rows], dim=0)
