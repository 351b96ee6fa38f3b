"""The FID statistic on the device (reference ``lib/metrics.py:211-212, 272-322``): feature mean and covariance, the traces and
``tr sqrtm(S1 S2)`` without the features, a 2048 x 2048 matrix or a ``scipy.linalg.sqrtm`` call on the host.

With ``Y_i = (F_i - mean F_i) / sqrt(N_i - 1)`` ([N_i, D]; ``S_i = Y_i^T Y_i`` is ``np.cov(F_i, rowvar=False)``):
``tr S_i = |Y_i|_F^2`` and ``tr sqrtm(S1 S2) = |Y2 S1^(1/2)|_*`` (the nuclear norm).  Both the nuclear norm of a matrix ``B`` and
``(B^T B)^(1/2)`` come out of the inverse-free Newton-Schulz iteration for the unitary polar factor (``polar_trace``), which needs
matrix products only and takes a rank-deficient ``B`` -- fewer samples than dimensions -- as it comes.  Derivation: DESIGN.md 4.

* ``gemm_f64``         ``alpha op(a) op(b) + diag I`` in float64 on the matrix cores (``vunet_f64_gemm``, csrc/fid.hip);
* ``feature_moments``  features [N, D] -> (mean [D], covariance [D, D]), float64 on the device;
* ``polar_trace``      ``B`` -> ``(|B|_*, (B^T B)^(1/2), iterations, converged)``;
* ``fid_device``       two feature sets -> ``FIDResult``.

The iteration's loop runs on the host: two GEMM launches and one dot product per step, and one 8-byte readback to decide
whether to stop.  Every sum is taken in a fixed order, so two runs agree bit for bit.  There is no CPU path; a run that reaches
``max_iter`` warns and takes the value from the host route (``lib.metrics._calculate_fid`` on the device's moments).
"""
from __future__ import annotations

import math
import warnings
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _lib
from .ops import _call, _p, _stream

_DOT_WORK = _lib.const("VUNET_F64_DOT_WORK")


class FIDResult(NamedTuple):
    fid: float
    iters: Tuple[int, int]       # steps of the two runs: S1^(1/2), then |Y2 S1^(1/2)|_*
    converged: bool              # both runs stopped by the tolerance (False: the value is the host route's, or nan)
    trace_gt: float              # tr S1
    trace_gen: float             # tr S2
    trace_sqrt: float            # tr sqrtm(S1 S2)


def _f64(t: torch.Tensor, what: str) -> torch.Tensor:
    if not (torch.is_tensor(t) and t.is_cuda):
        raise RuntimeError(f"{what} must be on the GPU (hand-written gfx950 kernels; no CPU fallback)")
    if t.dtype != torch.float64 or t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"{what}: float64 [rows >= 1, columns >= 1] expected, got {t.dtype} {tuple(t.shape)}")
    return t.detach().contiguous()


def gemm_f64(a: torch.Tensor, b: torch.Tensor, trans_a: bool = False, trans_b: bool = False, alpha: float = 1.0,
             diag: float = 0.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``alpha * op(a) @ op(b) + diag * I`` on float64 device matrices, ``op`` the transpose where ``trans_*``.  ``out``: a
    float64 [M, N] view whose rows are contiguous (its row stride is the leading dimension) that overlaps neither operand."""
    a, b = _f64(a, "a"), _f64(b, "b")
    m, k = (a.shape[1], a.shape[0]) if trans_a else (a.shape[0], a.shape[1])
    kb, n = (b.shape[1], b.shape[0]) if trans_b else (b.shape[0], b.shape[1])
    if k != kb:
        raise ValueError(f"gemm_f64: op(a) is [{m}, {k}], op(b) is [{kb}, {n}]")
    if out is None:
        out = torch.empty(m, n, device=a.device, dtype=torch.float64)
    elif (not out.is_cuda or out.dtype != torch.float64 or tuple(out.shape) != (m, n) or out.stride(1) != 1
          or (m > 1 and out.stride(0) < n)):
        raise ValueError(f"gemm_f64: out must be a float64 device [{m}, {n}] with contiguous rows")
    ldc = int(out.stride(0)) if m > 1 else max(int(out.stride(0)), n)
    with torch.cuda.device(a.device):
        _call("vunet_f64_gemm", _p(a), int(a.shape[1]), _p(b), int(b.shape[1]), _p(out), ldc, int(m), int(n), int(k),
              int(bool(trans_a)), int(bool(trans_b)), float(alpha), float(diag), _stream())
    return out


def _dot(a: torch.Tensor, b: torch.Tensor, work: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    with torch.cuda.device(a.device):
        _call("vunet_f64_dot", _p(a), _p(b), int(a.numel()), _p(work), _p(out), _stream())
    return out


def _center(feats: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """features [N >= 2, D] fp32 / float64 on the device -> (mu [D], Y [N, D]) float64, ``Y^T Y`` the covariance."""
    if not (torch.is_tensor(feats) and feats.is_cuda):
        raise RuntimeError("features must be on the GPU (hand-written gfx950 kernels; no CPU fallback)")
    if feats.dim() != 2 or feats.shape[0] < 2 or feats.shape[1] < 1:
        raise ValueError(f"features [N >= 2, D >= 1] expected, got {tuple(feats.shape)}")
    x = feats.detach()
    if x.dtype != torch.float64:
        x = x.to(torch.float32)
    x = x.contiguous()
    n, d = int(x.shape[0]), int(x.shape[1])
    mu = torch.empty(d, device=x.device, dtype=torch.float64)
    y = torch.empty(n, d, device=x.device, dtype=torch.float64)
    with torch.cuda.device(x.device):
        _call("vunet_fid_center_f64" if x.dtype == torch.float64 else "vunet_fid_center", _p(x), n, d, _p(mu), _p(y), _stream())
    return mu, y


def feature_moments(feats: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(np.mean(feats, axis=0), np.cov(feats, rowvar=False))`` in float64 on the device: the centring launch, then
    ``Y^T Y`` on the matrix cores (bit-symmetric)."""
    mu, y = _center(feats)
    return mu, gemm_f64(y, y, trans_a=True)


def polar_trace(B: torch.Tensor, tol: float = 1e-14, max_iter: int = 100, want_h: bool = False):
    """The nuclear norm of ``B`` [n, d] and, with ``want_h``, ``H = (B^T B)^(1/2)`` [d, d], by the inverse-free Newton-Schulz
    iteration for the polar factor: ``X_0 = B / |B|_F``, ``X <- X (1.5 I - 0.5 X^T X)`` -- or ``(1.5 I - 0.5 X X^T) X`` where ``B``
    has fewer rows than columns, so that the Gram matrix is the smaller side.  ``t_k = sum X_k * B`` rises to ``|B|_*``; the loop
    stops when ``t_k - t_(k-1) <= tol * t_k`` (a non-positive step included) or after ``max_iter`` steps, and ends at once with
    ``nan`` where ``t`` is not finite.  ``H = sym(X^T B)``.  -> ``(trace, H or None, iters, converged)``."""
    B = _f64(B, "B")
    n, d = int(B.shape[0]), int(B.shape[1])
    dev = B.device
    work = torch.empty(_DOT_WORK, device=dev, dtype=torch.float64)
    t_dev = torch.empty(1, device=dev, dtype=torch.float64)
    norm2 = float(_dot(B, B, work, t_dev).item())
    if not math.isfinite(norm2):
        return float("nan"), None, 0, False
    if norm2 == 0.0:
        return 0.0, (torch.zeros(d, d, device=dev, dtype=torch.float64) if want_h else None), 0, True
    X = torch.empty_like(B)
    with torch.cuda.device(dev):
        _call("vunet_f64_scale", _p(B), int(B.numel()), 1.0 / math.sqrt(norm2), _p(X), _stream())
    wide = n < d
    g = min(n, d)
    G = torch.empty(g, g, device=dev, dtype=torch.float64)
    Xn = torch.empty_like(X)
    t_prev = float(_dot(X, B, work, t_dev).item())   # = |B|_F
    iters, converged = 0, False
    while iters < int(max_iter):
        if wide:
            gemm_f64(X, X, trans_b=True, alpha=-0.5, diag=1.5, out=G)
            gemm_f64(G, X, out=Xn)
        else:
            gemm_f64(X, X, trans_a=True, alpha=-0.5, diag=1.5, out=G)
            gemm_f64(X, G, out=Xn)
        X, Xn = Xn, X
        iters += 1
        t = float(_dot(X, B, work, t_dev).item())
        if not math.isfinite(t):
            return float("nan"), None, iters, False
        step, t_prev = t - t_prev, t
        if step <= tol * t:
            converged = True
            break
    H = None
    if want_h:
        H = gemm_f64(X, B, trans_a=True)
        with torch.cuda.device(dev):
            _call("vunet_f64_symmetrize", _p(H), d, d, _stream())
    return t_prev, H, iters, converged


def _upload(feats, device) -> torch.Tensor:
    if torch.is_tensor(feats):
        return feats if feats.is_cuda else feats.to(device)
    a = np.asarray(feats)
    return torch.from_numpy(np.ascontiguousarray(a if a.dtype == np.float64 else a.astype(np.float32))).to(device)


def fid_device(gt_feats, gen_feats, tol: float = 1e-14, max_iter: int = 100) -> FIDResult:
    """``|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrtm(S1 S2)`` of two feature sets [N >= 2, D] (fp32 or float64 device tensors; host
    arrays are uploaded) on the device: one ``polar_trace`` on ``Y1`` for ``S1^(1/2)``, one on ``Y2 S1^(1/2)`` for the trace.
    A run that reaches ``max_iter`` emits a ``RuntimeWarning`` and the value is ``lib.metrics._calculate_fid`` of
    ``feature_moments`` copied to the host; a non-finite feature gives ``nan``."""
    device = next((f.device for f in (gt_feats, gen_feats) if torch.is_tensor(f) and f.is_cuda), None)
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    gt, gen = _upload(gt_feats, device), _upload(gen_feats, device)
    if gt.dim() != 2 or gen.dim() != 2 or gt.shape[1] != gen.shape[1]:
        raise ValueError(f"two feature sets [N, D] of one D expected, got {tuple(gt.shape)} and {tuple(gen.shape)}")
    mu1, y1 = _center(gt)
    mu2, y2 = _center(gen)
    work = torch.empty(_DOT_WORK, device=device, dtype=torch.float64)
    sums = torch.empty(3, device=device, dtype=torch.float64)
    diff = mu1 - mu2
    _dot(diff, diff, work, sums[0:1])
    _dot(y1, y1, work, sums[1:2])
    _dot(y2, y2, work, sums[2:3])
    d2, tr1, tr2 = (float(v) for v in sums.cpu().numpy())
    nan = float("nan")
    if not (math.isfinite(d2) and math.isfinite(tr1) and math.isfinite(tr2)):
        return FIDResult(nan, (0, 0), False, tr1, tr2, nan)
    _, h1, it1, ok1 = polar_trace(y1, tol, max_iter, want_h=True)
    if h1 is None:
        return FIDResult(nan, (it1, 0), False, tr1, tr2, nan)
    tr_sqrt, _, it2, ok2 = polar_trace(gemm_f64(y2, h1), tol, max_iter, want_h=False)
    if not math.isfinite(tr_sqrt):
        return FIDResult(nan, (it1, it2), False, tr1, tr2, nan)
    if ok1 and ok2:
        return FIDResult(d2 + tr1 + tr2 - 2.0 * tr_sqrt, (it1, it2), True, tr1, tr2, tr_sqrt)
    warnings.warn(f"fid_device: the polar iteration took {it1} and {it2} steps without meeting tol = {tol} within max_iter = "
                  f"{max_iter}; the value is the host route's (_calculate_fid on the device's moments)", RuntimeWarning, stacklevel=2)
    from .lib.metrics import _calculate_fid
    s1, s2 = gemm_f64(y1, y1, trans_a=True), gemm_f64(y2, y2, trans_a=True)
    fid = _calculate_fid(mu1.cpu().numpy(), s1.cpu().numpy(), mu2.cpu().numpy(), s2.cpu().numpy())
    return FIDResult(float(fid), (it1, it2), False, tr1, tr2, 0.5 * (d2 + tr1 + tr2 - float(fid)))
