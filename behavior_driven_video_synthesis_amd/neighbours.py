"""Nearest training-set neighbours of generated behaviour (the reference's ``nearest_neighbours`` figure, lib/figures.py:23-455):
for a generated sequence, the closest training sequence in behaviour-code space and in pose space -- the check that the model has
not memorised its training set.

The reference defines that function against ``ResidualBehaviorNet``'s own API (``infer_b``, ``b_enc.reparametrize``,
``generate_seq``) and imports it in experiments/mt_vae.py:606, but never calls it: it belongs to the behaviour path, not to the
MT-VAE baseline.  There the lookup is a host loop -- per query one numpy scan of all codes (:258-262) and one of all float64
training poses (:268-277).  Here the training set stays on the device (``TrainBank``) and each lookup is one streaming pass over
it for a whole tile of queries (csrc/seq_nn.hip, include/vunet_seq_nn.h); indices and distances stay on the device.

The reference adds the training set's mean pelvis to both sides before it subtracts them in pose space (:146-164, :268-272);
the term cancels in the difference and is left out.
"""
from __future__ import annotations

import ctypes
from typing import Iterable, Optional, Tuple

import torch

from . import _lib
from .behavior_eval import PoseStats
from .ops import _call, _p, _stream

# include/vunet_seq_nn.h
QT_CODES, QT_POSES, CHUNK, MAX_H, MAX_TN = (_lib.const("VUNET_NN_" + n) for n in ("QT_CODES", "QT_POSES", "CHUNK", "MAX_H", "MAX_TN"))


def scratch_bytes(n: int, q: int) -> int:
    out = ctypes.c_int64(0)
    _call("vunet_nn_scratch_bytes", int(n), int(q), ctypes.byref(out))
    return int(out.value)


def _results(n: int, q: int, dev):
    scratch = torch.empty(scratch_bytes(n, q), device=dev, dtype=torch.uint8)
    return scratch, torch.empty(q, device=dev, dtype=torch.float64), torch.empty(q, device=dev, dtype=torch.int32)


class TrainBank:
    """The training set on the device: ``sequences`` [N, T + 1, n] normalised fp32 keypoint sequences (what the reference's
    ``sequences.npy`` holds before its un-normalisation) and ``codes`` [N, H], their posterior means (its ``zbs.npy``);
    ``stats``: the dataset's ``PoseStats``."""

    def __init__(self, codes: torch.Tensor, sequences: torch.Tensor, stats: PoseStats):
        if codes.dim() != 2 or sequences.dim() != 3 or codes.shape[0] != sequences.shape[0] or codes.shape[0] < 1:
            raise ValueError(f"codes: [N, H] and sequences: [N, T + 1, n] expected, got {tuple(codes.shape)} and {tuple(sequences.shape)}")
        if sequences.shape[2] != stats.n_use:
            raise ValueError(f"pose vectors of {stats.n_use} used dimensions expected, got {sequences.shape[2]}")
        for name, v in (("codes", codes), ("sequences", sequences)):
            if not v.is_cuda or v.device != stats.mean.device:
                raise RuntimeError(f"{name} must be on {stats.mean.device} (hand-written gfx950 kernels; no CPU fallback)")
        self.codes = codes.to(torch.float32).contiguous()
        self.sequences = sequences.to(torch.float32).contiguous()
        self.stats = stats

    def __len__(self) -> int:
        return int(self.codes.shape[0])

    @classmethod
    @torch.no_grad()
    def build(cls, net, batches: Iterable[torch.Tensor], stats: PoseStats, batch: int = 1024) -> "TrainBank":
        """From an iterable of normalised ``keypoints`` tensors [B, T + 1, n]: the sequences are kept whole, their codes are
        ``mu`` of the encoder over ``x[:, :-1]`` (``prepare_input`` then ``infer_b(poses_in, False)``, lib/figures.py:85-101),
        ``batch`` rows per pass."""
        if not net.ib:
            raise ValueError("TrainBank.build needs the behaviour net's information bottleneck (its posterior mean is the code)")
        eng = net.engine()
        seqs, codes = [], []
        for x in batches:
            if x.dim() != 3 or x.shape[1] < 2:
                raise ValueError(f"keypoints: [B, T + 1, n] expected, got {tuple(x.shape)}")
            if not x.is_cuda or x.device != stats.mean.device:
                raise RuntimeError(f"keypoints must be on {stats.mean.device} (hand-written gfx950 kernels; no CPU fallback)")
            x = x.to(torch.float32)
            seqs.append(x)
            for s in range(0, x.shape[0], int(batch)):
                codes.append(eng.infer_b(x[s:s + int(batch), :-1].contiguous(), None)[1])
        if not seqs:
            raise ValueError("TrainBank.build: no batches")
        return cls(torch.cat(codes), torch.cat(seqs), stats)

    def nearest_codes(self, mu: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """``np.argmin(np.linalg.norm(codes - mu[q], axis=1))`` for every row of ``mu`` [Q, H] (lib/figures.py:258-262):
        -> (index int64 [Q], distance float64 [Q]), device tensors, no host sync.  The difference is the float32 one numpy
        takes; its squares, their sum and the root are float64."""
        n, h = self.codes.shape
        if mu.dim() != 2 or mu.shape[1] != h or mu.shape[0] < 1:
            raise ValueError(f"mu: [Q, H={h}] expected, got {tuple(mu.shape)}")
        if not mu.is_cuda or mu.device != self.codes.device:
            raise RuntimeError(f"mu must be on {self.codes.device} (hand-written gfx950 kernels; no CPU fallback)")
        if h > MAX_H:
            raise ValueError(f"codes of at most {MAX_H} dimensions (the query tile is held in LDS), got {h}")
        mu = mu.to(torch.float32).contiguous()
        q = int(mu.shape[0])
        scratch, dist, idx = _results(n, q, mu.device)
        _call("vunet_nn_codes", _p(self.codes), h, n, _p(mu), q, h, _p(scratch), _p(dist), _p(idx), _stream())
        return idx.to(torch.int64), dist

    def nearest_poses(self, xs: torch.Tensor, root: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """The training sequence closest to each row of ``xs`` [Q, T + 1, n] (normalised pose vectors of n = 3 J joint
        positions) in pose space (lib/figures.py:268-277): both sides un-normalised and centred on joint ``root`` (the
        reference's pelvis) frame by frame, the distance the sum over frames and joints of the joints' Euclidean distances,
        float64.  -> (index int64 [Q], distance float64 [Q]), device tensors, no host sync."""
        n, t, d = self.sequences.shape
        if xs.dim() != 3 or tuple(xs.shape[1:]) != (t, d) or xs.shape[0] < 1:
            raise ValueError(f"xs: [Q, T + 1={t}, n={d}] expected, got {tuple(xs.shape)}")
        if d % 3:
            raise ValueError(f"pose space compares joint positions: n = 3 J expected, got n = {d}")
        if not 0 <= int(root) < d // 3:
            raise ValueError(f"root must be in [0, J={d // 3}), got {root}")
        if not xs.is_cuda or xs.device != self.sequences.device:
            raise RuntimeError(f"xs must be on {self.sequences.device} (hand-written gfx950 kernels; no CPU fallback)")
        if t * d > MAX_TN:
            raise ValueError(f"sequences of at most {MAX_TN} values (the query tile is held in LDS), got {t} x {d}")
        xs = xs.to(torch.float32).contiguous()
        q = int(xs.shape[0])
        scratch, dist, idx = _results(n, q, xs.device)
        _call("vunet_nn_poses", _p(self.sequences), n, _p(xs), q, t, d // 3, int(root), _p(self.stats.mean), _p(self.stats.std),
              self.stats.f32_math, _p(scratch), _p(dist), _p(idx), _stream())
        return idx.to(torch.int64), dist


@torch.no_grad()
def posterior_neighbourhood(net, behavior_seq: torch.Tensor, start_poses: torch.Tensor, n: int = 5, logstd_scale: float = 0.8,
                            eps: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``n`` roll-outs per behaviour sequence from codes drawn around its posterior mean (lib/figures.py:213-233):
    b = eps * exp(logstd_scale * logstd) + mu, eps [B, n, H] given or drawn, each rolled out for T poses from
    ``start_poses[:, 0]`` with that pose put in front.  One encoder pass (the reference repeats it ``n`` times for the same
    mu) and one batched ``generate_seq``.  ``behavior_seq`` [B, T, n_kps], ``start_poses`` [B, T', n_kps]
    -> [B, n, T + 1, n_kps]."""
    if behavior_seq.dim() != 3 or start_poses.dim() != 3 or behavior_seq.shape[0] != start_poses.shape[0]:
        raise ValueError(f"posterior_neighbourhood: behaviour {tuple(behavior_seq.shape)} and start poses {tuple(start_poses.shape)}: "
                         "one [B, T, n] row of each per sequence")
    if not net.ib:
        raise ValueError("posterior_neighbourhood needs the behaviour net's information bottleneck")
    bsz, t, _ = behavior_seq.shape
    n, h = int(n), net.dim_hidden_b
    _, mu, logstd, _ = net.engine().infer_b(behavior_seq.contiguous(), None)
    if eps is None:
        eps = torch.randn(bsz, n, h, device=behavior_seq.device)
    if tuple(eps.shape) != (bsz, n, h):
        raise ValueError(f"eps: [B={bsz}, n={n}, H={h}] expected, got {tuple(eps.shape)}")
    b = (eps * torch.exp(logstd_scale * logstd).unsqueeze(1) + mu.unsqueeze(1)).reshape(bsz * n, h)
    starts = start_poses[:, :1].repeat_interleave(n, dim=0)
    xs, *_ = net.generate_seq(b, starts, len=t, start_frame=0)
    return torch.cat([starts, xs], dim=1).reshape(bsz, n, t + 1, xs.shape[-1])
