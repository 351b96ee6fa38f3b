"""NumPy float64 restatement of the part-normalised appearance input (include/vunet_inplane.h): the four source points of a part
(the reference's t5p / t4p / t3p / t2p, lib/utils.py:70-232, and valid_joints, :515-517), the eight-unknown system of
cv2.getPerspectiveTransform solved by Gaussian elimination with partial pivoting, the inverse of the 3x3, and the bilinear warp
with the border replicated (data/base_dataset.py:685-725).  Everything here is float64, the blend included; the kernels blend in
fp32.  Written for reading, one part and one pixel grid at a time.  Not a test module."""
import numpy as np

T2P, T3P, T4P, T5P = 2, 3, 4, 5

MARKET = [(T4P, (8, 9, 3, 2)), (T3P, (8, 9, 13)), (T2P, (0, 1)), (T2P, (1, 2)), (T2P, (6, 7)), (T2P, (7, 8)), (T2P, (3, 4)),
          (T2P, (4, 5)), (T2P, (9, 10)), (T2P, (10, 11))]                          # data/market.py:45, :25-32
DEEPFASHION = [(T4P, (8, 2, 5, 11)), (T3P, (2, 5, 0)), (T2P, (2, 3)), (T2P, (3, 4)), (T2P, (5, 6)), (T2P, (6, 7)), (T2P, (8, 9)),
               (T2P, (9, 10)), (T2P, (11, 12)), (T2P, (12, 13))]                   # data/deepfashion.py:61-72, :26-33


def _box(p0, p1, alpha):
    seg = p1 - p0
    n = np.array([-seg[1], seg[0]])
    return p0 + alpha * n, p0 - alpha * n, p1 - alpha * n, p1 + alpha * n     # a, b, c, d


def dst_points(kind, wh):
    wh = float(wh)
    if kind in (T4P, T5P):
        return np.array([[0.0, 0.0], [wh, 0.0], [wh, wh], [0.0, wh]])
    d = np.array([[0.0, 0.0], [0.0, wh], [wh, wh], [wh, 0.0]])
    return d - 1.0 if kind == T2P else d                                      # t2p: np.multiply(dst, wh) - 1.0 (:228)


def src_points(kps, kind, ids, oh):
    """kps [J, 2] -> the four source points [4, 2] float64 in the builder's order, or None where the builder returns None."""
    k = np.asarray(kps, dtype=np.float32).astype(np.float64)[list(ids)]
    if kind == T4P:
        return k.copy()
    if kind == T5P:
        rhip, rs, neck, ls, lhip = k
        ls_to_rs, rh_to_rs, lh_to_ls = rs - ls, rs - rhip, ls - lhip
        with np.errstate(all="ignore"):
            den_l = ls_to_rs[1] * lh_to_ls[0] - ls_to_rs[0] * lh_to_ls[1]
            den_r = ls_to_rs[1] * rh_to_rs[0] - ls_to_rs[0] * rh_to_rs[1]
            lam_l = (lhip[1] - neck[1]) * lh_to_ls[0] / den_l + (neck[0] - lhip[0]) * lh_to_ls[1] / den_l
            lam_r = (rhip[1] - neck[1]) * rh_to_rs[0] / den_r + (neck[0] - rhip[0]) * rh_to_rs[1] / den_r
            return np.stack([neck + lam_r * ls_to_rs, neck + lam_l * ls_to_rs, lhip, rhip])
    if kind == T3P:
        rs, ls, head = k
        if (k >= 0).all():
            neck = 0.5 * (rs + ls)
            a, b, c, d = _box(neck + 2.0 * (head - neck), neck, 0.5)
        else:
            if not (k[:2] >= 0).all():
                return None
            seg = rs - ls
            n = np.array([-seg[1], seg[0]])
            if n[1] > 0.0:
                n = -n
            a, b, c, d = ls + n, ls, rs, rs + n
        return np.stack([b, c, d, a])
    assert kind == T2P
    if np.any(np.all(k <= 0.0, axis=1)):
        pos = np.nonzero(np.all(k > 0.0, axis=1))[0]
        if pos.size == 0:
            return None
        t = k[int(pos[0])]
        return np.stack(_box(t, np.array([t[0], float(oh) - 1.0]), 0.25))
    return np.stack(_box(k[0], k[1], 0.25))


def solve_inverse(src, dst):
    """The homography src -> dst with bottom-right entry 1, inverted: [9] float64 (dst -> src), or None where a pivot or the
    determinant is not usable (non-finite, a pivot below 1e-9 x the largest magnitude of the 8x8 matrix, a zero determinant)."""
    A = np.zeros((8, 9))
    for i in range(4):
        x, y = src[i]
        X, Y = dst[i]
        A[i] = [x, y, 1.0, 0.0, 0.0, 0.0, -x * X, -y * X, X]
        A[i + 4] = [0.0, 0.0, 0.0, x, y, 1.0, -x * Y, -y * Y, Y]
    amax = np.abs(A[:, :8]).max()
    if not np.isfinite(amax):
        return None
    with np.errstate(all="ignore"):
        for c in range(8):
            r = c + int(np.argmax(np.abs(A[c:, c])))      # the first of equal maxima
            best = abs(A[r, c])
            if not np.isfinite(best) or best < 1e-9 * amax:
                return None
            if r != c:
                A[[c, r]] = A[[r, c]]
            for i in range(c + 1, 8):
                f = A[i, c] / A[c, c]
                A[i, c + 1:] = A[i, c + 1:] - f * A[c, c + 1:]
                A[i, c] = 0.0
        h = np.zeros(9)
        for c in range(7, -1, -1):
            s = A[c, 8]
            for j in range(c + 1, 8):
                s = s - A[c, j] * h[j]
            h[c] = s / A[c, c]
        h[8] = 1.0
        c0, c1, c2 = h[4] * h[8] - h[5] * h[7], h[3] * h[8] - h[5] * h[6], h[3] * h[7] - h[4] * h[6]
        det = (h[0] * c0 - h[1] * c1) + h[2] * c2
        if not np.isfinite(det) or det == 0.0:
            return None
        m = np.array([c0, h[2] * h[7] - h[1] * h[8], h[1] * h[5] - h[2] * h[4],
                      -c1, h[0] * h[8] - h[2] * h[6], h[2] * h[3] - h[0] * h[5],
                      c2, h[1] * h[6] - h[0] * h[7], h[0] * h[4] - h[1] * h[3]]) / det
    return m if np.isfinite(m).all() else None


def part_transforms(kps, parts, s_out, oh):
    """kps [N, J, 2] -> (minv [N, P, 9], src [N, P, 4, 2], valid [N, P] int32); an absent part: zeros in minv (and in src where the
    builder returns None)."""
    kps = np.asarray(kps)
    n, p = kps.shape[0], len(parts)
    minv, src, valid = np.zeros((n, p, 9)), np.zeros((n, p, 4, 2)), np.zeros((n, p), dtype=np.int32)
    for i in range(n):
        for q, (kind, ids) in enumerate(parts):
            s = src_points(kps[i], kind, ids, oh)
            if s is None:
                continue
            src[i, q] = s
            m = solve_inverse(s, dst_points(kind, s_out)) if np.isfinite(s).all() else None
            if m is not None:
                minv[i, q], valid[i, q] = m, 1
    return minv, src, valid


def source_coords(m, s_out, hs, ws):
    """The clamped source coordinate (sx, sy) [s_out, s_out] of every output pixel under one homography m [9]."""
    y, x = np.meshgrid(np.arange(s_out, dtype=np.float64), np.arange(s_out, dtype=np.float64), indexing="ij")
    u, v, w = (m[0] * x + m[1] * y) + m[2], (m[3] * x + m[4] * y) + m[5], (m[6] * x + m[7] * y) + m[8]
    with np.errstate(all="ignore"):
        sx, sy = np.where(w != 0.0, u / w, 0.0), np.where(w != 0.0, v / w, 0.0)     # w == 0 samples (0, 0)
    sx, sy = np.where(np.isnan(sx), 0.0, sx), np.where(np.isnan(sy), 0.0, sy)
    return np.clip(sx, 0.0, ws - 1.0), np.clip(sy, 0.0, hs - 1.0)


def warp(img, minv, valid, s_out, absent=-1.0):
    """img [N, 3, Hs, Ws], minv [N, P, 9], valid [N, P] -> [N, 3 P, s_out, s_out] float64."""
    img = np.asarray(img, dtype=np.float64)
    n, _, hs, ws = img.shape
    p = minv.shape[1]
    out = np.full((n, 3 * p, s_out, s_out), float(absent))
    for i in range(n):
        for q in range(p):
            if not valid[i, q]:
                continue
            sx, sy = source_coords(minv[i, q], s_out, hs, ws)
            x0, y0 = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
            x1, y1 = np.minimum(x0 + 1, ws - 1), np.minimum(y0 + 1, hs - 1)
            fx, fy = sx - x0, sy - y0
            for c in range(3):
                pl = img[i, c]
                top = pl[y0, x0] + fx * (pl[y0, x1] - pl[y0, x0])
                bot = pl[y1, x0] + fx * (pl[y1, x1] - pl[y1, x0])
                out[i, 3 * q + c] = top + fy * (bot - top)
    return out


def part_crops(img, kps, parts, s_out, oh=None, absent=-1.0):
    minv, _, valid = part_transforms(kps, parts, s_out, np.asarray(img).shape[2] if oh is None else oh)
    return warp(img, minv, valid, s_out, absent)


def apply_h(m, pts):
    """Homography m [9] applied to points [K, 2]."""
    pts = np.asarray(pts, dtype=np.float64)
    u = m[0] * pts[:, 0] + m[1] * pts[:, 1] + m[2]
    v = m[3] * pts[:, 0] + m[4] * pts[:, 1] + m[5]
    w = m[6] * pts[:, 0] + m[7] * pts[:, 1] + m[8]
    return np.stack([u / w, v / w], axis=1)


def quad_area(q):
    """Area of the quad q [4, 2] (shoelace, absolute)."""
    x, y = q[:, 0], q[:, 1]
    return 0.5 * abs(np.dot(x, np.roll(y, -1)) - np.dot(y, np.roll(x, -1)))


def threshold_margin(kps, parts):
    """The smallest distance of a coordinate a builder tests from its validity threshold (0), over the joints the T2P and T3P parts
    read: the GPU tests draw keypoints with this >= 0.5 so that no rounding decides a branch."""
    k = np.asarray(kps, dtype=np.float64)
    ids = sorted({j for kind, i in parts if kind in (T2P, T3P) for j in i})
    return float(np.abs(k[:, ids]).min()) if ids else float("inf")
