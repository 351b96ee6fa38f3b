"""Scoring a behaviour model the way the reference does (experiments/behavior_net.py:1112-1301, lib/logging.py:2079-2093):
sample S behaviours per test sequence, roll them out, and measure their diversity (ASD, FSD, APD) and their best fit to the
ground-truth future (ADE, FDE); plus the "three characters" transfer numbers (ADE_c, FDE_c, recon / distance of mu).

The reference draws the S samples one after another (a flow reverse and a roll-out on B / 4 rows each), copies every sampled
sequence to the host, un-normalises it in numpy and builds the distance tables with two host syncs per row.  Here the S samples
of every sequence are one batched pass through ``FlowEngine`` / ``BehaviorEngine`` (their 64-row chunks and recorded graphs),
and the un-normalisation, the distance tables and the selections are two HIP launches (csrc/seq_eval.hip,
include/vunet_seq_eval.h) whose results stay on the device until ``BehaviorEvaluator.summary``.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from .ops import _call, _p, _stream

METRICS = ("APD", "ASD", "FSD", "minADE", "minFDE")      # per sequence, in the kernel's output order
TRANSFER = ("ADE_c", "FDE_c", "recon_mu", "recon_std", "distance_mu", "distance_std")


class PoseStats:
    """The dataset's normalisation statistics on the device (``data_mean``, ``data_std``, ``dim_to_ignore``: what
    ``revert_output_format`` / ``unNormalizeData`` take, data/data_conversions_3d.py:178-211).  The statistics' dtype decides the
    precision of the un-normalisation, as numpy's promotion does: float32 statistics mean float32 arithmetic, anything else
    float64.  Only the used dimensions are kept: the ignored ones hold ``mean`` in every vector and add 0 to any distance."""

    def __init__(self, data_mean, data_std, dim_to_ignore, device="cuda"):
        mean, std = np.asarray(data_mean), np.asarray(data_std)
        if mean.shape != std.shape or mean.ndim != 1:
            raise ValueError(f"data_mean {mean.shape} and data_std {std.shape}: two vectors of the same length expected")
        self.f32_math = int(mean.dtype == np.float32 and std.dtype == np.float32)
        ignore = {int(d) for d in np.asarray(dim_to_ignore).reshape(-1)}
        use = np.asarray([d for d in range(mean.size) if d not in ignore], dtype=np.int64)
        self.dim, self.n_use = int(mean.size), int(use.size)
        self.dims_to_use = torch.as_tensor(use, device=device)
        self.mean = torch.as_tensor(mean[use].astype(np.float64), device=device)
        self.std = torch.as_tensor(std[use].astype(np.float64), device=device)


def _rows_of(z: torch.Tensor, n: int, s: int) -> torch.Tensor:
    """[S, N, H] noise in the reference's draw order (one ``randn_like(b[::skip])`` per sample) -> [N S, H], row i S + s = z[s, i]."""
    if z.dim() != 3 or z.shape[0] != s or z.shape[1] != n:
        raise ValueError(f"z: [n_samples={s}, N={n}, H] expected, got {tuple(z.shape)}")
    return z.transpose(0, 1).reshape(n * s, z.shape[2]).contiguous()


@torch.no_grad()
def sample_behaviors(net, flow, start_poses: torch.Tensor, n_samples: int, length: int, start_frame: int = -1,
                     z: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """The sampling loop of experiments/behavior_net.py:1182-1217 as one batched pass: -> [N, S, length, n] normalised poses.

    ``start_poses`` [N, T, n] (the reference passes ``target_s[::skip]``), the roll-out starts from frame ``start_frame`` of each.
    Behaviour codes b = flow.reverse(z), z ~ N(0, 1) drawn for all N S rows at once (or the given ``z`` [S, N, H]); with ``flow``
    None, b is the prior noise itself -- the reference's ``net(..., sample=True)`` branch, whose encoder output is discarded and
    is therefore not computed."""
    if n_samples < 2:
        raise ValueError(f"n_samples must be >= 2 (the self-distance comes first in every row), got {n_samples}")
    n_seq = start_poses.shape[0]
    h = net.dim_hidden_b
    if z is None:
        z = torch.randn(n_samples, n_seq, h, device=start_poses.device, generator=generator)
    zr = _rows_of(z.to(start_poses.device, torch.float32), n_seq, n_samples)
    b = flow.reverse(zr).reshape(n_seq * n_samples, h) if flow is not None else zr
    x = start_poses.repeat_interleave(n_samples, dim=0)           # row i S + s starts from sequence i
    xs, *_ = net.generate_seq(b, x, len=length, start_frame=start_frame % start_poses.shape[1])
    return xs.reshape(n_seq, n_samples, length, xs.shape[-1])


def sample_metrics(samples: torch.Tensor, future: torch.Tensor, stats: PoseStats) -> Dict[str, torch.Tensor]:
    """ASD / FSD / APD / min ADE / min FDE per sequence and the batch's ADE / FDE, float64 device tensors, no host sync.

    ``samples`` [N, S, T, n] normalised poses (``sample_behaviors``); ``future`` [N, T + 1, n] the normalised ground truth, of
    which frames 1 .. T are scored (the reference's ``seq_gt[:, :, 1:]``, :1235)."""
    if samples.dim() != 4:
        raise ValueError(f"samples: [N, S, T, n] expected, got {tuple(samples.shape)}")
    n_seq, s, t, n = samples.shape
    if s < 2:
        raise ValueError(f"n_samples must be >= 2, got {s}")
    if tuple(future.shape) != (n_seq, t + 1, n):
        raise ValueError(f"future: [N={n_seq}, T + 1={t + 1}, n={n}] expected, got {tuple(future.shape)}")
    if n != stats.n_use:
        raise ValueError(f"pose vectors of {stats.n_use} used dimensions expected, got {n}")
    for name, v in (("samples", samples), ("future", future)):
        if not v.is_cuda or v.device != stats.mean.device:
            raise RuntimeError(f"{name} must be on {stats.mean.device} (hand-written gfx950 kernels; no CPU fallback)")
    x = samples.to(torch.float32).contiguous()
    g = future.to(torch.float32).contiguous()
    dev = x.device
    scratch = torch.empty(n_seq * s * (3 * s + 2), device=dev, dtype=torch.float64)
    per_seq = torch.empty(len(METRICS), n_seq, device=dev, dtype=torch.float64)
    batch = torch.empty(2, device=dev, dtype=torch.float64)
    _call("vunet_seq_eval_pairs", _p(x), _p(g), _p(stats.mean), _p(stats.std), stats.f32_math, n_seq, s, t, n, _p(scratch), _stream())
    _call("vunet_seq_eval_select", _p(scratch), n_seq, s, _p(per_seq), _p(batch), _stream())
    out = {k: per_seq[j] for j, k in enumerate(METRICS)}
    out["ADE"], out["FDE"] = batch[0], batch[1]
    return out


@torch.no_grad()
def transfer_metrics(net, x_s: torch.Tensor, x_t: torch.Tensor, x_related: torch.Tensor,
                     eps: Optional[torch.Tensor] = None, return_mu: bool = False):
    """The "three characters" numbers of experiments/behavior_net.py:1262-1278 (printed at :1299-1301), 0-dim device tensors:
    ``seq_cross`` = net(x_s, x_t) (x_s's behaviour on x_t's start pose; ``eps``: its reparametrisation noise, None: drawn);
    mu2, mu3 = the encoder's mu of ``seq_cross`` and of ``x_related``.  ADE_c / FDE_c against x_s in normalised space;
    recon_* over ||mu - mu2||, distance_* over ||mu - mu3|| (``torch.std``: unbiased).  ``return_mu``: -> (metrics, mu), the
    behaviour codes the classifier study collects (:1263) without a second encoder pass."""
    t = x_s.shape[1]
    seq_cross, _, _, _, mu, *_ = net(x_s, x_t, t, sample=False, eps=eps)
    eng = net.engine()
    mu2 = eng.infer_b(seq_cross.contiguous(), None)[1]       # the encoder alone: mu does not depend on the noise
    mu3 = eng.infer_b(x_related.contiguous(), None)[1]
    r, d = torch.norm(mu - mu2, dim=1), torch.norm(mu - mu3, dim=1)
    out = {"ADE_c": torch.mean(torch.norm(seq_cross - x_s, dim=2)), "FDE_c": torch.mean(torch.norm(seq_cross[:, -1] - x_s[:, -1], dim=1)),
           "recon_mu": torch.mean(r), "recon_std": torch.std(r), "distance_mu": torch.mean(d), "distance_std": torch.std(d)}
    return (out, mu) if return_mu else out


class BehaviorEvaluator:
    """The reference's metric lists (experiments/behavior_net.py:1112-1121, lib/logging.py APD): per-sequence ASD, FSD and APD,
    per-batch ADE, FDE and transfer metrics.  ``add`` keeps device tensors; ``summary`` copies them to the host once and returns
    ``np.mean`` of every non-empty list -- plus, when an evaluation ran with ``latent_diagnostics``, the numbers of
    ``latent_diag.LatentDiagnostics.summary``."""

    def __init__(self):
        self.per_seq: Dict[str, List[torch.Tensor]] = {k: [] for k in ("APD", "ASD", "FSD")}
        self.per_batch: Dict[str, List[torch.Tensor]] = {k: [] for k in ("ADE", "FDE") + TRANSFER}
        self.latent = None      # latent_diag.LatentDiagnostics, set by BehaviorNet.evaluate(..., latent_diagnostics=...)

    def add(self, metrics: Dict[str, torch.Tensor]):
        for k, v in metrics.items():
            if k in self.per_seq:
                self.per_seq[k].append(v.reshape(-1))
            elif k in self.per_batch:
                self.per_batch[k].append(v.reshape(1))

    def lists(self) -> Dict[str, np.ndarray]:
        """Every list as a float64 array (one device-to-host copy)."""
        parts = [(k, torch.cat(v).to(torch.float64)) for d in (self.per_seq, self.per_batch) for k, v in d.items() if v]
        if not parts:
            return {}
        flat = torch.cat([p for _, p in parts]).cpu().numpy()
        out, o = {}, 0
        for k, p in parts:
            out[k] = flat[o:o + p.numel()]
            o += p.numel()
        return out

    def summary(self) -> Dict[str, float]:
        out = {k: float(np.mean(v)) for k, v in self.lists().items()}
        if self.latent is not None:      # self_recon_eval and, with a flow, the four FlowLoss means and ks_p_mean
            out.update(self.latent.summary())
        return out


# ---- the real-vs-fake classifier study (experiments/behavior_net.py:1262-1295 collection, :1302-1521 study)

STUDY_TIMES = (0, 10, 20, 30, 40, 49)
STUDY_SETS = ("orig", "prior", "cross", "self", "flow")


class StudySet:
    """The sequences ``run_inference`` keeps for the classifier study, on the device: X_orig, X_prior, X_cross, X_self and (with
    a flow) X_flow [rows, T, 51], and X_embed = mu [rows, H].  The reference's cap (:1260, :1294-1295): a batch is collected
    while fewer than ``max_rows`` rows are held, so the batch that crosses the cap is kept whole; once ``full``, the scoring loop
    still scores the next batch and then ends."""

    def __init__(self, max_rows: int = 25000):
        self.max_rows = int(max_rows)
        self.parts: Dict[str, List[torch.Tensor]] = {k: [] for k in STUDY_SETS + ("embed",)}
        self.rows = 0

    @property
    def full(self) -> bool:
        return self.rows >= self.max_rows

    def add(self, orig, prior, cross, self_, mu, flow=None):
        for k, v in (("orig", orig), ("prior", prior), ("cross", cross), ("self", self_), ("embed", mu), ("flow", flow)):
            if v is not None:
                self.parts[k].append(v.detach().to(torch.float32))
        self.rows += int(orig.shape[0])

    def tensors(self) -> Dict[str, torch.Tensor]:
        return {k: torch.cat(v, 0).contiguous() for k, v in self.parts.items() if v}


class _Classifier(torch.nn.Module):
    """models/pose_behavior_rnn.py:6-17 in torch layout (its default initialisation draws the weights of ``init=None``)."""

    def __init__(self, n_in=51, n_c=1):
        super().__init__()
        self.dim = 256
        self.GRU = torch.nn.GRU(n_in, self.dim, 1, batch_first=True)
        self.act = torch.nn.ReLU()
        self.fc1 = torch.nn.Linear(self.dim, n_c)


class _Regressor(torch.nn.Module):
    """models/pose_behavior_rnn.py:33-44 in torch layout."""

    def __init__(self, n_dim, n_key=51):
        super().__init__()
        self.act = torch.nn.ReLU()
        self.fc1 = torch.nn.Linear(n_dim, n_dim // 2)
        self.fc2 = torch.nn.Linear(n_dim // 2, n_dim // 4)
        self.fc3 = torch.nn.Linear(n_dim // 4, n_key)


def default_study_init(times, dim_hidden_b: int, flow: bool) -> List[Dict[str, Dict[str, torch.Tensor]]]:
    """Initial weights the way the reference draws them (:1331-1356), per start time, from torch's global CPU generator:
    modules built in the order real1, real2, flow (with a flow), self, regressor, self -- the second ``class_real_self``
    replaces the first."""
    out = []
    for _ in times:
        d = {"prior": _Classifier().state_dict(), "cross": _Classifier().state_dict()}
        if flow:
            d["flow"] = _Classifier().state_dict()
        _Classifier()
        d["regressor"] = _Regressor(dim_hidden_b).state_dict()
        d["self"] = _Classifier().state_dict()
        out.append(d)
    return out


def classifier_study(study_set, times=STUDY_TIMES, bs: int = 256, iterations: int = 2000, init=None, graph: bool = True) -> Dict:
    """The reference's discriminative evaluation (experiments/behavior_net.py:1302-1521) on the HIP kernels of csrc/seq_cls.hip.

    ``study_set``: a ``StudySet`` or a dict of its tensors (orig, prior, cross, self, optional flow: [N, T, 51]; embed [N, H]).
    For every start time in ``times``, fresh GRU classifiers learn real (target 1) vs fake (target 0) with SGD(lr 1e-3,
    momentum 0.9) -- prior, cross and, with a flow, flow samples -- and a regressor maps mu to the pose at frame ``start`` with
    Adam(lr 1e-3).  The reference's semantics, kept as they are:
    * ``epochs = iterations // (N // bs)``; batches in fixed order, no shuffling, the last partial batch dropped.  N < bs raises
      ``ValueError`` (the reference divides by zero).
    * ``class_real_self`` never trains: its optimiser is built over ``class_real2``'s parameters (:1349, :1358), and stepping it
      after its own ``zero_grad`` moves nothing.  "Acc Self" is an untrained classifier's mean sigmoid on X_self, so neither
      its backward nor its forward on the real half (a loss nothing reads) is run.
    * The final pass (:1459-1517) measures the accuracies with the trained classifiers on the fake half and goes on training
      the regressor: ``Loss_regressor`` is that pass's mean, ``DE`` = mean ||X_cross[:, start] - X_orig[:, start]||.
    ``init``: None (``default_study_init``) or, per start time, torch-layout state dicts {"prior", "cross", "flow", "self":
    ``GRU.weight_ih_l0``, ..., ``fc1.*``; "regressor": ``fc1-3.*``}.  All start times train together, batched into every launch;
    ``graph`` replays one recorded iteration (False: the same launches issued one by one).

    -> {"final": [per start time {"Acc Prior", "Acc Cross", "Acc Self", ("Acc Flow"), "Loss_regressor", "DE"}], "curves":
    [per start time {"acc1", "loss1", "acc2", "loss2", "acc_self", ("acc_flow", "loss_flow"), "loss_regressor"} float32 arrays
    over the training iterations], "times", "epochs", "num_samples"}."""
    from . import seq_cls as C
    sets = study_set.tensors() if isinstance(study_set, StudySet) else dict(study_set)
    for k in ("orig", "prior", "cross", "self", "embed"):
        if k not in sets:
            raise ValueError(f"the study set has no {k!r} sequences")
    orig = sets["orig"]
    if not orig.is_cuda:
        raise RuntimeError("the study runs on the GPU (hand-written gfx950 kernels; no CPU fallback)")
    n, t = int(orig.shape[0]), int(orig.shape[1])
    if orig.dim() != 3 or orig.shape[2] != C.NIN:
        raise ValueError(f"sequences [N, T, {C.NIN}] expected, got {tuple(orig.shape)}")
    for k in STUDY_SETS[1:]:
        if k in sets and tuple(sets[k].shape) != tuple(orig.shape):
            raise ValueError(f"{k}: {tuple(sets[k].shape)} differs from orig {tuple(orig.shape)}")
    if sets["embed"].shape[0] != n or sets["embed"].dim() != 2 or sets["embed"].shape[1] % 4:
        raise ValueError(f"embed: [N={n}, H] with H % 4 == 0 expected, got {tuple(sets['embed'].shape)}")
    if not 1 <= bs <= C.MAX_BS:
        raise ValueError(f"bs must be in [1, {C.MAX_BS}], got {bs}")
    if n < bs:
        raise ValueError(f"{n} rows is fewer than one batch of {bs}")
    times = [int(s) for s in times]
    if not times or any(s < 0 or s >= t for s in times):
        raise ValueError(f"every start time must be in [0, T={t}), got {times}")
    flow = "flow" in sets
    h = int(sets["embed"].shape[1])
    if init is None:
        init = default_study_init(times, h, flow)
    if len(init) != len(times):
        raise ValueError(f"init: one entry per start time ({len(times)}) expected, got {len(init)}")
    kinds = C.KINDS if flow else C.KINDS[:2]
    cls_blocks = torch.stack([torch.stack([C.pack_classifier(d[k]) for k in kinds + ("self",)]) for d in init])
    reg_blocks = torch.stack([C.pack_regressor(d["regressor"], h) for d in init])
    eng = C.StudyEngine(sets, sets["embed"], times, bs, iterations, cls_blocks, reg_blocks)
    eng.run(graph=graph)
    loss_c, acc_c, acc_s, reg_loss, de = eng.results()
    it, nk = eng.iters, eng.nk
    names = {"prior": ("acc1", "loss1", "Acc Prior"), "cross": ("acc2", "loss2", "Acc Cross"), "flow": ("acc_flow", "loss_flow", "Acc Flow")}
    finals, curves = [], []
    for si in range(len(times)):
        fin, cur = {}, {}
        for ki, k in enumerate(kinds):
            g = si * nk + ki
            a, l, f = names[k]
            cur[a], cur[l] = acc_c[g, :it].copy(), loss_c[g, :it].copy()
            fin[f] = float(np.mean(acc_c[g, it:].astype(np.float64)))
        cur["acc_self"] = acc_s[si, :it].copy()
        cur["loss_regressor"] = reg_loss[si, :it].copy()
        fin["Acc Self"] = float(np.mean(acc_s[si, it:].astype(np.float64)))
        fin["Loss_regressor"] = float(np.mean(reg_loss[si, it:].astype(np.float64)))
        fin["DE"] = float(np.mean(de[si, it:].astype(np.float64)))
        finals.append(fin)
        curves.append(cur)
    return {"final": finals, "curves": curves, "times": times, "epochs": eng.epochs, "num_samples": n}
