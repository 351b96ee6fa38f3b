"""Host side of the FID tests: the seeded feature sets of tests/golden/g21_fid.npz and two float64 restatements of
``|mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrtm(S1 S2)`` that never call ``scipy.linalg.sqrtm`` -- a symmetric-eigenvalue form and the
polar iteration of fid_device.py in numpy -- plus the exact and extended-precision references of the GEMM tests."""
import numpy as np

from synth import seeded_randn

SEED = 21
# name -> (D, N1, N2, halvings of the column scale from the first column to the last, dead leading columns)
FULL_RANK = {"d64": (64, 200, 168, 0, 0), "d50_odd": (50, 131, 77, 3, 0), "d256_dead": (256, 1000, 900, 8, 5),
             "d128_illcond": (128, 700, 650, 15, 0)}
RANK_DEFICIENT = {"d64_n40": (64, 40, 40, 0, 0), "d96_n17": (96, 17, 23, 2, 0), "d48_n2": (48, 2, 3, 0, 0)}
CASES = {**FULL_RANK, **RANK_DEFICIENT}
SHIFTS = (0.5, 0.75)      # the two sets of a case differ in seed and in shift


def feature_set(case: str, which: int) -> np.ndarray:
    """Set ``which`` (0: ground truth, 1: generated) of ``case`` as fp32 [N, D]: relu(scale_d (r[n, d] + r[n, d + 1] / 2 + g[n] / 2) +
    shift scale_d) with scale_d an exact power of two, element-wise float64 arithmetic on seeded normals only (no matrix product:
    nothing here depends on a BLAS), then the leading ``dead`` columns zeroed."""
    D, N1, N2, halvings, dead = CASES[case]
    N = (N1, N2)[which]
    r = seeded_randn(f"fid.{case}.{which}.r", (N, D + 1), SEED).double().numpy()
    g = seeded_randn(f"fid.{case}.{which}.g", (N, 1), SEED).double().numpy()
    scale = np.ldexp(1.0, -((np.arange(D) * halvings) // max(D - 1, 1)))[None, :]
    x = np.maximum(scale * (r[:, :D] + 0.5 * r[:, 1:] + 0.5 * g) + SHIFTS[which] * scale, 0.0)
    x[:, :dead] = 0.0
    return x.astype(np.float32)


def moments(x: np.ndarray):
    x = np.asarray(x, dtype=np.float64)
    return np.mean(x, axis=0), np.cov(x, rowvar=False)


def _psd_sqrt(s: np.ndarray) -> np.ndarray:
    w, v = np.linalg.eigh(0.5 * (s + s.T))
    return (v * np.sqrt(np.maximum(w, 0.0))) @ v.T


def fid_sym(gt: np.ndarray, gen: np.ndarray) -> float:
    """tr sqrtm(S1 S2) as the sum of the square roots of the eigenvalues of S1^(1/2) S2 S1^(1/2), both roots by ``eigh``."""
    (mu1, s1), (mu2, s2) = moments(gt), moments(gen)
    h1 = _psd_sqrt(s1)
    w = np.linalg.eigvalsh(h1 @ s2 @ h1)
    diff = mu1 - mu2
    return float(diff @ diff + np.trace(s1) + np.trace(s2) - 2.0 * np.sum(np.sqrt(np.maximum(w, 0.0))))


def polar_trace(B: np.ndarray, tol: float = 1e-14, max_iter: int = 100, want_h: bool = False):
    """fid_device.polar_trace in numpy: -> (nuclear norm, H or None, iters, converged)."""
    B = np.asarray(B, dtype=np.float64)
    n, d = B.shape
    norm2 = float(np.sum(B * B))
    if norm2 == 0.0:
        return 0.0, (np.zeros((d, d)) if want_h else None), 0, True
    X = B / np.sqrt(norm2)
    t_prev = float(np.sum(X * B))
    iters, converged = 0, False
    while iters < max_iter:
        if n < d:
            X = (1.5 * np.eye(n) - 0.5 * (X @ X.T)) @ X
        else:
            X = X @ (1.5 * np.eye(d) - 0.5 * (X.T @ X))
        iters += 1
        t = float(np.sum(X * B))
        step, t_prev = t - t_prev, t
        if not np.isfinite(t):
            return float("nan"), None, iters, False
        if step <= tol * t:
            converged = True
            break
    H = None
    if want_h:
        H = X.T @ B
        H = 0.5 * (H + H.T)
    return t_prev, H, iters, converged


def fid_polar(gt: np.ndarray, gen: np.ndarray, tol: float = 1e-14, max_iter: int = 100):
    """-> (fid, (iters of the two runs), converged)."""
    gt, gen = np.asarray(gt, dtype=np.float64), np.asarray(gen, dtype=np.float64)
    mu1, mu2 = gt.mean(axis=0), gen.mean(axis=0)
    y1 = (gt - mu1) / np.sqrt(gt.shape[0] - 1)
    y2 = (gen - mu2) / np.sqrt(gen.shape[0] - 1)
    _, h1, it1, ok1 = polar_trace(y1, tol, max_iter, want_h=True)
    t, _, it2, ok2 = polar_trace(y2 @ h1, tol, max_iter)
    diff = mu1 - mu2
    return float(diff @ diff + np.sum(y1 * y1) + np.sum(y2 * y2) - 2.0 * t), (it1, it2), bool(ok1 and ok2)


def group_bar(golden_meta: dict, group) -> float:
    """The bar of a group of cases: four times the largest relative distance from ``fid_ref`` of the fixture's two host methods
    (``fid_sym``, ``fid_polar``) over the group -- the spread the reference's own float64 arithmetic allows, times 4 for another
    summation order in the products."""
    spread = 0.0
    for case in group:
        c = golden_meta["cases"][case]
        spread = max(spread, abs(c["fid_sym"] - c["fid_ref"]) / abs(c["fid_ref"]), abs(c["fid_polar"] - c["fid_ref"]) / abs(c["fid_ref"]))
    return 4.0 * spread


# ---- GEMM references
def op(a: np.ndarray, trans: bool) -> np.ndarray:
    return a.T if trans else a


def gemm_exact_int(a, b, trans_a, trans_b, alpha: int, diag: int) -> np.ndarray:
    """alpha op(a) op(b) + diag I on integer-valued operands in int64."""
    c = alpha * (op(np.asarray(a).astype(np.int64), trans_a) @ op(np.asarray(b).astype(np.int64), trans_b))
    idx = np.arange(min(c.shape))
    c[idx, idx] += diag
    return c


def gemm_longdouble(a, b, trans_a, trans_b):
    """(op(a) op(b), sum_k |a_k b_k|) in np.longdouble."""
    A, B = op(np.asarray(a), trans_a).astype(np.longdouble), op(np.asarray(b), trans_b).astype(np.longdouble)
    return A @ B, np.abs(A) @ np.abs(B)
