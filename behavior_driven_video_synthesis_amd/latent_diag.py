"""The latent diagnostics of the reference's evaluation loop (lib/logging.py ``eval_nets``): the held-out flow likelihood
(``FlowLoss`` on test data, :2228-2236, :2656-2660), the Kolmogorov-Smirnov test of every dimension of the flow's Gaussianised
codes against N(0, 1) (:2549-2562), and the sample sets its latent plots are drawn from (:2242-2262).

The reference copies every code to the host and loops ``scipy.stats.kstest`` over the code dimensions.  Here the codes stay in
one column-major device buffer per set (``LatentCollector``), one HIP launch sorts every column in LDS and takes the statistic
and the asymptotic p-value in float64 (csrc/seq_latent.hip, include/vunet_seq_latent.h), and the four ``FlowLoss`` entries of a
batch of any size are two launches with float64 accumulation.  Nothing syncs with the host until a result is read.
"""
from __future__ import annotations

import math
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from .ops import _call, _p, _stream

FLOW_KEYS = ("flow_loss", "reference_nll_loss", "nlogdet_loss", "nll_loss")     # the kernel's output order
KS_MAX_LDS_N = _lib.const("VUNET_SEQ_KS_MAX_LDS_N")   # the longest column one workgroup sorts in LDS
SETS = ("b", "mu", "pre", "prior_samples", "flow_samples", "gaussian_samples")
P_METHODS = ("reference", "asymptotic", "exact")

ks_routes = {"lds": 0, "torch_sort": 0}    # how often ``ks_normal`` took each route (what the tests assert on)


def _device_f32(name: str, t: torch.Tensor) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a device tensor (hand-written gfx950 kernels; no CPU fallback)")
    return t.detach().to(torch.float32)


class FlowNLL:
    """``flow_nll``'s result, device tensors: ``scalars`` [4] f64 in ``FLOW_KEYS`` order, ``nll`` [B] f64 (0.5 sum z^2 per
    row), ``log_prob`` [B] f64 (-nll + logdet - 0.5 C log 2 pi)."""

    def __init__(self, scalars, nll, log_prob):
        self.scalars, self.nll, self.log_prob = scalars, nll, log_prob

    def log(self) -> Dict[str, float]:
        """The four entries under the reference's keys as Python floats (one device-to-host copy)."""
        return dict(zip(FLOW_KEYS, self.scalars.tolist()))


def flow_nll(gauss: torch.Tensor, logdet: torch.Tensor, noise: Optional[torch.Tensor] = None) -> FlowNLL:
    """lib/losses.py:295-311 on the device in float64: ``gauss`` [B, C] or [B, C, 1, 1] (any strides with unit stride along
    C), ``logdet`` [B], ``noise`` the standard-normal draw behind ``reference_nll_loss`` (None: that entry is NaN)."""
    z = _device_f32("gauss", gauss)
    if z.dim() == 4 and z.shape[2] == 1 and z.shape[3] == 1:
        z = z[:, :, 0, 0]
    if z.dim() != 2 or z.shape[0] < 1 or z.shape[1] < 1:
        raise ValueError(f"gauss: [B, C] or [B, C, 1, 1] expected, got {tuple(gauss.shape)}")
    b, c = z.shape
    if z.stride(1) != 1 or z.stride(0) < c:
        z = z.contiguous()
    ld = _device_f32("logdet", logdet)
    if ld.dim() != 1 or ld.shape[0] != b:
        raise ValueError(f"logdet: [B={b}] expected, got {tuple(logdet.shape)}")
    ld = ld.contiguous()
    nz = None
    if noise is not None:
        nz = _device_f32("noise", noise).reshape(noise.shape[0], -1).contiguous()
        if tuple(nz.shape) != (b, c):
            raise ValueError(f"noise: {(b, c)} expected, got {tuple(noise.shape)}")
    per_row = torch.empty(2, b, device=z.device, dtype=torch.float64)
    scalars = torch.empty(4, device=z.device, dtype=torch.float64)
    with torch.cuda.device(z.device):
        _call("vunet_seq_latent_nll", _p(z), z.stride(0), _p(ld), _p(nz), b, c, _p(per_row), _p(scalars), _stream())
    return FlowNLL(scalars, per_row[0], per_row[1])


def kolmogorov_sf(t: float) -> float:
    """The asymptotic p-value at t = D sqrt(N) on the host: the same series as the kernel's, for a caller who holds a statistic
    only.  ``KSResult`` does not use it: its asymptotic values come from the launch."""
    if not t > 0.0:
        return t if t != t else 1.0
    if t < 0.2:
        w, s = math.pi * math.pi / (8.0 * t * t), 0.0
        for k in range(1, 257):
            m = float(2 * k - 1)
            term = math.exp(-m * m * w)
            s += term
            if term < 1e-17:
                break
        p = 1.0 - math.sqrt(2.0 * math.pi) / t * s
    else:
        s, sign = 0.0, 1.0
        for k in range(1, 257):
            term = math.exp(-2.0 * float(k) * float(k) * t * t)
            s += sign * term
            sign = -sign
            if term < 1e-17:
                break
        p = 2.0 * s
    return min(max(p, 0.0), 1.0)


def reference_rule_takes_asymptotic(n: int, p_asym: np.ndarray) -> np.ndarray:
    """``kstest(mode='approx')`` of scipy 1.3.3 (the reference's pinned version): the asymptotic p-value when N > 2666 or
    p_asym > 0.80 - 0.0003 N, else twice the one-sided exact value."""
    p_asym = np.asarray(p_asym, dtype=np.float64)
    return np.logical_or(n > 2666, p_asym > 0.80 - n * 0.3 / 1000.0)


class KSResult:
    """Per column of the tested set, device tensors [C] f64: ``statistic`` (D), ``d_plus``, ``d_minus``, ``p_asymptotic``;
    ``n`` rows.  A column holding a NaN has NaN everywhere (scipy's ``nan_policy='propagate'``)."""

    def __init__(self, statistic, d_plus, d_minus, p_asymptotic, n: int):
        self.statistic, self.d_plus, self.d_minus, self.p_asymptotic, self.n = statistic, d_plus, d_minus, p_asymptotic, int(n)

    def pvalues(self, method: str = "reference") -> np.ndarray:
        """Host float64 [C].  "asymptotic": the device series.  "exact": ``scipy.stats.kstwo.sf(D, N)``, what a current
        scipy's ``kstest`` returns.  "reference": scipy 1.3.3's ``mode='approx'`` rule (``reference_rule_takes_asymptotic``);
        for N > 2666 that is the asymptotic value and scipy is not imported."""
        if method not in P_METHODS:
            raise ValueError(f"method must be one of {P_METHODS}, got {method!r}")
        both = torch.stack([self.statistic, self.p_asymptotic]).cpu().numpy()
        d, p = both[0], both[1].copy()
        if method == "asymptotic":
            return p
        if method == "exact":
            from scipy import stats
            out = stats.kstwo.sf(d, self.n)
            return np.where(np.isnan(d), np.nan, out)
        take = reference_rule_takes_asymptotic(self.n, p) | np.isnan(d)
        if not take.all():
            from scipy import stats
            p[~take] = np.minimum(2.0 * stats.ksone.sf(d[~take], self.n), 1.0)
        return p

    def p_mean(self, method: str = "reference") -> float:
        """``np.mean`` of the p-values: the number ``eval_nets`` logs (lib/logging.py:2556)."""
        return float(np.mean(self.pvalues(method)))


def ks_normal(x: torch.Tensor, col_major: bool = False) -> KSResult:
    """``scipy.stats.kstest(column, "norm")``'s statistic for every column of ``x`` in one launch.  ``x``: [N, C] (rows are
    samples), or with ``col_major`` [C, N] (each column contiguous: ``LatentCollector.columns``); unit stride along the last
    dimension is read in place.  Up to 32768 rows the kernel sorts in LDS; longer columns are sorted by ``torch.sort`` first
    and the kernel only evaluates the statistic."""
    x = _device_f32("x", x)
    if x.dim() != 2 or x.shape[0] < 1 or x.shape[1] < 1:
        raise ValueError(f"x: a non-empty 2-D tensor expected, got {tuple(x.shape)}")
    n, c = (x.shape[1], x.shape[0]) if col_major else (x.shape[0], x.shape[1])
    sorted_ = 0
    if n > KS_MAX_LDS_N:
        # sort ascending with NaN last (torch.sort's order); the kernel flags the NaN itself
        x = torch.sort(x, dim=1 if col_major else 0)[0]
        sorted_ = 1
        ks_routes["torch_sort"] += 1
    else:
        ks_routes["lds"] += 1
    if x.stride(1) != 1 or x.stride(0) < x.shape[1]:
        x = x.contiguous()
    stat = torch.empty(3, c, device=x.device, dtype=torch.float64)
    p = torch.empty(c, device=x.device, dtype=torch.float64)
    with torch.cuda.device(x.device):
        _call("vunet_seq_ks_norm", _p(x), x.stride(0), int(bool(col_major)), n, c, sorted_, _p(stat), _p(p), None, _stream())
    return KSResult(stat[0], stat[1], stat[2], p, n)


class LatentCollector:
    """The sets ``eval_nets`` collects for its latent plots and the KS test (lib/logging.py:2242-2262), on the device: per name
    one preallocated COLUMN-major buffer [C, cap] (a code dimension is contiguous: what the KS launch reads) with a row count,
    plus the int64 ``actions``.  ``dims``: {name: C} for the sets wanted (names from ``SETS``)."""

    def __init__(self, dims: Dict[str, int], cap: int, device="cuda"):
        for k in dims:
            if k not in SETS:
                raise ValueError(f"unknown set {k!r}: one of {SETS}")
        self.cap = int(cap)
        self.device = torch.device(device)
        self.buf = {k: torch.empty(int(c), max(self.cap, 1), device=self.device, dtype=torch.float32) for k, c in dims.items()}
        self.rows = {k: 0 for k in dims}
        self.actions = torch.empty(max(self.cap, 1), device=self.device, dtype=torch.int64)
        self.rows["actions"] = 0

    def add(self, name: str, rows: torch.Tensor):
        """Append a [B, C] batch ([B] int64 for ``actions``)."""
        if not rows.is_cuda:
            raise RuntimeError(f"{name} must be a device tensor (no CPU fallback)")
        n, b = self.rows[name], int(rows.shape[0])
        have = self.actions.shape[0] if name == "actions" else self.buf[name].shape[1]
        if n + b > have:       # batches of unequal size can pass the strict rule with more than ``cap`` rows in all: grow
            if name == "actions":
                self.actions = torch.cat([self.actions, self.actions.new_empty(max(have, n + b - have))])
            else:
                old = self.buf[name]
                self.buf[name] = torch.cat([old, old.new_empty(old.shape[0], max(have, n + b - have))], dim=1)
        if name == "actions":
            self.actions[n:n + b].copy_(rows.reshape(b))
        else:
            r = rows.detach().reshape(b, -1)
            if r.shape[1] != self.buf[name].shape[0]:
                raise ValueError(f"{name}: [B, {self.buf[name].shape[0]}] expected, got {tuple(rows.shape)}")
            self.buf[name][:, n:n + b].copy_(r.t())
        self.rows[name] = n + b

    def get(self, name: str) -> torch.Tensor:
        """The [n, C] view of a set ([n] for ``actions``)."""
        if name == "actions":
            return self.actions[:self.rows[name]]
        return self.buf[name][:, :self.rows[name]].t()

    def columns(self, name: str) -> torch.Tensor:
        """The [C, n] buffer itself: ``ks_normal(..., col_major=True)`` reads it without a copy."""
        return self.buf[name][:, :self.rows[name]]


class LatentDiagnostics:
    """What ``BehaviorNet.evaluate(..., latent_diagnostics=...)`` leaves in ``ev.latent``: the per-batch ``FlowLoss`` entries and
    self-reconstruction errors (device tensors until ``summary``), the collector, and after ``finish`` the KS result."""

    def __init__(self, collector: LatentCollector, n_max: int, ks_method: str, with_flow: bool):
        if ks_method not in P_METHODS:
            raise ValueError(f"ks_method must be one of {P_METHODS}, got {ks_method!r}")
        self.collector, self.n_max, self.ks_method, self.with_flow = collector, int(n_max), ks_method, with_flow
        self.flow_scalars, self.recon = [], []
        self.ks: Optional[KSResult] = None
        self._summary = None

    def admits(self, batch_nr: int, rows: int) -> bool:
        """The reference's collection rule, a strict inequality (lib/logging.py:2242, :2256)."""
        return (batch_nr + 1) * rows < self.n_max

    def finish(self):
        if self.with_flow and self.collector.rows.get("gaussian_samples", 0) > 0:
            self.ks = ks_normal(self.collector.columns("gaussian_samples"), col_major=True)

    def summary(self) -> Dict[str, float]:
        """``self_recon_eval`` (sum of the batch values over the number of batches, :2623) and, with a flow, the four entries'
        means over the batches (:2657-2659) and ``ks_p_mean`` (:2556).  One device-to-host copy, cached."""
        if self._summary is None:
            out: Dict[str, float] = {}
            if self.recon:
                r = torch.stack(self.recon).to(torch.float64).cpu().numpy()
                out["self_recon_eval"] = float(np.sum(r) / r.size)
            if self.with_flow and self.flow_scalars:
                f = torch.stack(self.flow_scalars).cpu().numpy()
                for j, k in enumerate(FLOW_KEYS):
                    out[k] = float(np.mean(f[:, j]))
            if self.ks is not None:
                out["ks_p_mean"] = self.ks.p_mean(self.ks_method)
            self._summary = out
        return dict(self._summary)

    def __getattr__(self, k):
        if k in FLOW_KEYS + ("self_recon_eval", "ks_p_mean"):
            s = self.summary()
            if k in s:
                return s[k]
        raise AttributeError(k)
