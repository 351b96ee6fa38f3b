"""Float64 restatement of the two nearest-neighbour distances of lib/figures.py:258-277 and of numpy's ``argmin``, what
``vunet_nn_codes`` / ``vunet_nn_poses`` (csrc/seq_nn.hip) are held to -- as tests/behavior_interp_ref.py is for the slerp kernel.

Code space: the difference is the float32 one numpy takes on float32 codes; its square is exact in float64; the sum is exactly
rounded (``math.fsum``) and the root is the C library's.  Pose space: un-normalisation as ``unNormalizeData`` with numpy's
promotion (float32 statistics keep ``x * std + mean`` in float32), then float64: centring on the root joint, the difference,
(dx^2 + dy^2) + dz^2, the root, and an exactly rounded sum over frames and joints.  The reference's mean pelvis is added to both
sides there and cancels; it is left out here (tests/golden/make_golden_behavior_neighbours.py keeps it, and
tests/test_behavior_neighbours_golden.py holds this file to that).

U = 2^-53.  A device sum of K non-negative float64 terms in any order is within (K - 1) U of the exact sum, relative; each
term of the pose sum carries at most a few U of its own (three products, two adds, a root), and the root of the code sum halves
the sum's error and adds U / 2.  ``bound`` = (K + 8) U covers both, K = H, or T J + 3.
"""
import math

import numpy as np

U = 2.0 ** -53


def bound(k):
    """Relative distance bound for a sum of ``k`` terms."""
    return (k + 8) * U


def code_distances(bank, q):
    """bank [N, H], q [Q, H] float32 -> float64 [Q, N]."""
    bank, q = np.asarray(bank, dtype=np.float32), np.asarray(q, dtype=np.float32)
    out = np.empty((q.shape[0], bank.shape[0]))
    for a in range(q.shape[0]):
        e = (bank - q[a]).astype(np.float64)          # one float32 rounding, then exact squares
        sq = e * e
        for j in range(bank.shape[0]):
            s = math.fsum(sq[j])
            out[a, j] = math.sqrt(s) if s == s else float("nan")
    return out


def centred(x, mean, std, root):
    """[..., T, 3 J] normalised float32 -> [..., T, J, 3] float64 un-normalised joints minus the root joint."""
    x, mean, std = np.asarray(x, dtype=np.float32), np.asarray(mean), np.asarray(std)
    if mean.dtype == np.float32 and std.dtype == np.float32:
        u = (x * std + mean).astype(np.float64)       # numpy keeps float32 statistics in float32
    else:
        u = x.astype(np.float64) * std.astype(np.float64) + mean.astype(np.float64)
    u = u.reshape(*x.shape[:-1], x.shape[-1] // 3, 3)
    return u - u[..., root:root + 1, :]


def pose_distances(bank, q, mean, std, root):
    """bank [N, T, 3 J], q [Q, T, 3 J] float32 -> float64 [Q, N]."""
    cb, cq = centred(bank, mean, std, root), centred(q, mean, std, root)
    out = np.empty((cq.shape[0], cb.shape[0]))
    with np.errstate(invalid="ignore"):
        for a in range(cq.shape[0]):
            d = cq[a] - cb
            norms = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).reshape(cb.shape[0], -1)
            for j in range(cb.shape[0]):
                out[a, j] = math.fsum(norms[j]) if np.isfinite(norms[j]).all() else float(np.sum(norms[j]))
    return out


def argmin_rows(dist):
    """numpy's argmin per row of [Q, N]: the smallest value, the lowest index among equals, the first NaN before any number.
    -> (index int64 [Q], minimum float64 [Q], gap float64 [Q]): gap = (second best - best) / best over the other rows, inf
    for one row, NaN where a NaN is involved."""
    dist = np.asarray(dist, dtype=np.float64)
    idx = np.empty(dist.shape[0], dtype=np.int64)
    for a, row in enumerate(dist):
        nan = np.flatnonzero(row != row)
        if nan.size:
            idx[a] = nan[0]
            continue
        best = 0
        for j in range(1, row.size):
            if row[j] < row[best]:
                best = j
        idx[a] = best
    assert np.array_equal(idx, np.argmin(dist, axis=1))
    best = dist[np.arange(dist.shape[0]), idx]
    gap = np.full(dist.shape[0], np.inf)
    if dist.shape[1] > 1:
        rest = dist.copy()
        rest[np.arange(dist.shape[0]), idx] = np.inf
        with np.errstate(invalid="ignore", divide="ignore"):
            gap = (rest.min(axis=1) - best) / best
    return idx, best, gap
