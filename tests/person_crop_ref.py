"""Plain torch / numpy restatements (float64, no kernel) of the person-box crop and of the Inception score's statistic:
what csrc/person_crop.hip and csrc/inception_score.hip are tested against."""
import math

import numpy as np
import torch
import torch.nn.functional as F


# ------------------------------------------------------------------------------------------------
# the box rule (lib/utils.py:560-585 with cv2.boundingRect ASSUMED to be floor(min), floor(max) - floor(min) + 1)
# ------------------------------------------------------------------------------------------------
def keypoint_boxes_ref(kps):
    """kps [N, J, C] -> (boxes [N, 4] int32 (x, y, w, h), valid [N] int32)."""
    kps = np.asarray(kps, dtype=np.float32)
    boxes, valid = np.zeros((kps.shape[0], 4), np.int32), np.zeros(kps.shape[0], np.int32)
    for n, pts in enumerate(kps):
        pts = pts[np.all(pts > 0., axis=1)]
        if len(pts) == 0:
            continue
        x, y = math.floor(pts[:, 0].min()), math.floor(pts[:, 1].min())
        boxes[n] = (x, y, math.floor(pts[:, 0].max()) - x + 1, math.floor(pts[:, 1].max()) - y + 1)
        valid[n] = 1
    return boxes, valid


# ------------------------------------------------------------------------------------------------
# the crop: kornia 0.2.0's steps literally, and the closed form of include/vunet_person_crop.h
# ------------------------------------------------------------------------------------------------
def _perspective(src, dst):
    """The 3x3 map of four points src -> dst [4, 2]: the eight-unknown system (bottom-right entry 1), float64."""
    rows, rhs = [], []
    for (x, y), (X, Y) in zip(src.tolist(), dst.tolist()):
        rows += [[x, y, 1.0, 0.0, 0.0, 0.0, -x * X, -y * X], [0.0, 0.0, 0.0, x, y, 1.0, -x * Y, -y * Y]]
        rhs += [X, Y]
    h = torch.linalg.solve(torch.tensor(rows, dtype=torch.float64), torch.tensor(rhs, dtype=torch.float64))
    return torch.cat([h, torch.ones(1, dtype=torch.float64)]).view(3, 3)


def _normal(size_h, size_w):
    """kornia 0.2.0's pixel -> [-1, 1] matrix: 2 / (size - 1)."""
    return torch.tensor([[2.0 / (size_w - 1), 0.0, -1.0], [0.0, 2.0 / (size_h - 1), -1.0], [0.0, 0.0, 1.0]], dtype=torch.float64)


def kornia_crop_literal(img, boxes, S):
    """``kornia.crop_and_resize(img, corners(boxes), (S, S))`` as kornia 0.2.0 over torch 1.3.1 runs it, step by step: the
    perspective transform box corners -> (0, 0) .. (S - 1, S - 1), normalised on both sides with 2 / (size - 1), inverted, applied to
    a linspace(-1, 1) mesh of the output, then ``F.grid_sample(bilinear, zeros, align_corners=False)`` -- the default of the torch
    the reference pins.  img float64 [N, Ch, Hs, Ws], boxes [N, 4] (x, y, w, h)."""
    img = torch.as_tensor(img, dtype=torch.float64)
    n, _, hs, ws = img.shape
    out = []
    lin = torch.linspace(-1.0, 1.0, S, dtype=torch.float64)
    gy, gx = torch.meshgrid(lin, lin, indexing="ij")
    mesh = torch.stack([gx, gy, torch.ones_like(gx)], dim=-1).view(-1, 3)          # (x, y, 1) of every output pixel
    dst = torch.tensor([[0.0, 0.0], [S - 1.0, 0.0], [S - 1.0, S - 1.0], [0.0, S - 1.0]], dtype=torch.float64)
    for i in range(n):
        x, y, w, h = (float(v) for v in boxes[i])
        src = torch.tensor([[x, y], [x + w, y], [x + w, y + h], [x, y + h]], dtype=torch.float64)
        m = _perspective(src, dst)                                                  # source pixel -> output pixel
        m_norm = _normal(S, S) @ m @ torch.linalg.inv(_normal(hs, ws))              # normalised source -> normalised output
        p = mesh @ torch.linalg.inv(m_norm).t()                                     # output mesh -> normalised source
        grid = (p[:, :2] / p[:, 2:3]).view(1, S, S, 2)
        out.append(F.grid_sample(img[i:i + 1], grid, mode="bilinear", padding_mode="zeros", align_corners=False))
    return torch.cat(out, dim=0)


def crop_coords(boxes, S, hs, ws, sampling):
    """The sampled pixel coordinates (u [N, S], v [N, S], float64) of the closed form, operation for operation as the kernel."""
    b = torch.as_tensor(np.asarray(boxes), dtype=torch.float64)
    idx = torch.arange(S, dtype=torch.float64)
    u = b[:, 0:1] + (idx[None] * b[:, 2:3]) / float(S - 1)
    v = b[:, 1:2] + (idx[None] * b[:, 3:4]) / float(S - 1)
    if sampling == "reference":
        u = (u * float(ws)) / float(ws - 1) - 0.5
        v = (v * float(hs)) / float(hs - 1) - 0.5
    elif sampling != "exact":
        raise ValueError(sampling)
    return u, v


def _sample_zeros(img, u, v):
    """Bilinear taps with zero padding at pixel coordinates u [N, S] (columns), v [N, S] (rows), in img's dtype."""
    n, ch, hs, ws = img.shape
    x0, y0 = torch.floor(u), torch.floor(v)
    fx, fy = (u - x0).to(img.dtype), (v - y0).to(img.dtype)
    x0, y0 = x0.long(), y0.long()

    def tap(yy, xx):   # [N, S] rows, [N, S] columns -> [N, Ch, S, S]
        ok = ((yy >= 0) & (yy < hs))[:, :, None] & ((xx >= 0) & (xx < ws))[:, None, :]
        yi, xi = yy.clamp(0, hs - 1), xx.clamp(0, ws - 1)
        g = img[torch.arange(n)[:, None, None], :, yi[:, :, None], xi[:, None, :]]   # [N, S, S, Ch]
        return g.permute(0, 3, 1, 2) * ok[:, None].to(img.dtype)
    a, b, c, d = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
    fx, fy = fx[:, None, None, :], fy[:, None, :, None]
    top, bot = a + fx * (b - a), c + fx * (d - c)
    return top + fy * (bot - top)


def crop_closed_form(img, boxes, S, sampling="reference", valid=None):
    """The formulas of include/vunet_person_crop.h in float64: u = x + j w / (S - 1) (and the REFERENCE shift), floor, four taps
    with zero padding, three lerps.  ``valid`` == 0 rows are zeros."""
    img = torch.as_tensor(img, dtype=torch.float64)
    u, v = crop_coords(boxes, S, img.shape[2], img.shape[3], sampling)
    out = _sample_zeros(img, u, v)
    if valid is not None:
        out = out * torch.as_tensor(np.asarray(valid) != 0, dtype=torch.float64)[:, None, None, None]
    return out


def crop_grid_sample_fp32(img, boxes, S, sampling="reference"):
    """The same restatement the way plain torch runs it in fp32 on the CPU: the sampled pixel coordinates rounded to fp32,
    normalised for ``F.grid_sample(align_corners=False)`` ((2 p + 1) / size - 1) and sampled in fp32.  Its error against the
    float64 closed form is fp32's own figure for this crop: the yardstick of the kernel's tolerance."""
    img = torch.as_tensor(img, dtype=torch.float32)
    n, _, hs, ws = img.shape
    u, v = crop_coords(boxes, S, hs, ws, sampling)
    gx = ((2.0 * u.float() + 1.0) / ws - 1.0)[:, None, :].expand(n, S, S)
    gy = ((2.0 * v.float() + 1.0) / hs - 1.0)[:, :, None].expand(n, S, S)
    return F.grid_sample(img, torch.stack([gx, gy], dim=-1), mode="bilinear", padding_mode="zeros", align_corners=False)


# ------------------------------------------------------------------------------------------------
# the Inception score's statistic (lib/metrics.py:403-415, scipy.stats.entropy(pk, qk)), float64
# ------------------------------------------------------------------------------------------------
def inception_score_ref(logits, splits=1):
    """logits [N, K] -> scores [splits] float64: softmax by log-sum-exp, then per split exp(mean_i KL(p_i || mean p)) with both
    vectors renormalised and 0 log 0 = 0.  A split without rows is NaN (the reference's mean of nothing)."""
    l = np.asarray(logits, dtype=np.float64)
    e = np.exp(l - l.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    n = p.shape[0]
    rows = n // splits
    scores = np.full(splits, np.nan)
    for k in range(splits):
        part = p[k * rows:(k + 1) * rows]
        if rows == 0:
            continue
        q = part.mean(axis=0)
        q = q / q.sum()
        kls = []
        for row in part:
            ph = row / row.sum()
            nz = ph > 0
            kls.append(np.sum(ph[nz] * np.log(ph[nz] / q[nz])))
        scores[k] = np.exp(np.mean(kls))
    return scores
