"""NumPy restatement of the random appearance augmentation (csrc/appearance_aug.hip, include/vunet_appearance_aug.h): Pillow's
``Image.transform(AFFINE, BILINEAR, fillcolor)`` of a reflect-padded RGB frame, cut to a window, and the fixture loader.  Shared by
the CPU tests (tests/test_appearance_aug_ref.py), the fixture's writer (tests/golden/make_golden_appearance_aug.py, which does NOT
use it to make the expected bytes -- those are Pillow's) and the kernel's tests (tests/test_hip_appearance_aug.py).

float64 NumPy arithmetic rounds every multiply and add on its own, as Pillow's C does; the store truncates.  Nothing here has a
tolerance."""
import os

import numpy as np

import image_input_ref as I

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g22_appearance_aug.npz")
PAD_BYTE = I.PAD_BYTE


def refl(i, n: int) -> np.ndarray:
    """NumPy's ``mode="reflect"`` of any integer index (dcb|abcd|cba): period ``2 (n - 1)``; ``n == 1`` maps everything to 0."""
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    period = 2 * (n - 1)
    m = np.mod(i, period)
    return np.where(m >= n, period - m, m)


def affine_u8(frame: np.ndarray, mat, pad: int = 0, origin=(0, 0), out_hw=None, fill=(0, 0, 0)):
    """frame uint8 [h, w, 3] and one output-to-input affine (six float64) -> ``(bytes [oh, ow, 3], status)``: the rule of
    include/vunet_appearance_aug.h, operation by operation."""
    h, w = frame.shape[:2]
    H, W = h + 2 * pad, w + 2 * pad
    oh, ow = (H, W) if out_hw is None else out_hw
    m = np.asarray(mat, dtype=np.float64)
    out = np.empty((oh, ow, 3), dtype=np.uint8)
    out[:] = np.asarray(fill, dtype=np.uint8)
    if not np.isfinite(m).all():
        return out, 1
    xin = (np.arange(ow, dtype=np.int64) + origin[0]).astype(np.float64)[None, :] + 0.5
    yin = (np.arange(oh, dtype=np.int64) + origin[1]).astype(np.float64)[:, None] + 0.5
    with np.errstate(over="ignore", invalid="ignore"):
        xs = (m[0] * xin + m[1] * yin) + m[2]
        ys = (m[3] * xin + m[4] * yin) + m[5]
        inside = (xs >= 0.0) & (xs < W) & (ys >= 0.0) & (ys < H)
    xs, ys = np.where(inside, xs, 0.5) - 0.5, np.where(inside, ys, 0.5) - 0.5
    x0, y0 = np.floor(xs), np.floor(ys)
    dx, dy = (xs - x0)[..., None], (ys - y0)[..., None]
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
    ra, rb = refl(np.clip(y0, 0, H - 1) - pad, h), refl(np.clip(y0 + 1, 0, H - 1) - pad, h)
    ca, cb = refl(np.clip(x0, 0, W - 1) - pad, w), refl(np.clip(x0 + 1, 0, W - 1) - pad, w)
    f = frame.astype(np.float64)
    a, b = f[ra, ca], f[ra, cb]
    v1 = a + (b - a) * dx
    a, b = f[rb, ca], f[rb, cb]
    v2 = a + (b - a) * dx
    v = v1 + (v2 - v1) * dy
    out[inside] = np.trunc(v).astype(np.uint8)[inside]
    return out, 0


def affine_stack(frames, hw, mats, pad=0, origin=(0, 0), out_hw=None, fill=(0, 0, 0), size=None):
    """A padded stack [N, Hmax, Wmax, 3], its frame sizes [N, 2] and matrices [N, 6] -> ``(bytes [N, oh, ow, 3], status [N])``;
    with ``size`` that is not the window, Pillow's bicubic resize of the bytes after it (tests/image_input_ref.py)."""
    if out_hw is None:
        out_hw = (frames.shape[1] + 2 * pad, frames.shape[2] + 2 * pad)
    outs, status = [], []
    for f, (h, w), m in zip(frames, hw, mats):
        o, s = affine_u8(f[:h, :w], m, pad, origin, out_hw, fill)
        if size is not None and (size, size) != tuple(out_hw):
            o = I.resize(o, size)
        outs.append(o)
        status.append(s)
    return np.stack(outs), np.asarray(status, dtype=np.int32)


def to_float(u8: np.ndarray) -> np.ndarray:
    """bytes [N, h, w, 3] -> fp32 [N, 3, h, w], ``ToTensor`` and ``x * 2 - 1`` with every operation rounded once."""
    return I.to_float(u8)


def stack(frames, hmax: int, wmax: int) -> np.ndarray:
    return I.stack(frames, hmax, wmax)


def load_fixture():
    """tests/golden/g22_appearance_aug.npz (tests/golden/make_golden_appearance_aug.py) as ``{name: dict(frames [N, Hmax, Wmax, 3]
    padded with PAD_BYTE, hw [N, 2], mats [N, 6], angles [N] (NaN: not a rotation), kw = dict(pad, origin, out_hw, fill, size),
    expect [N, oh, ow, 3] or [N, size, size, 3])}``."""
    z = np.load(FIXTURE)
    cases = {}
    for name in (str(s) for s in z["case_names"]):
        fr = [z["frame_" + str(i)] for i in z[name + "_frames"]]
        hmax, wmax = (int(v) for v in z[name + "_stack"])
        pad, ox, oy, oh, ow, r, g, b, size = (int(v) for v in z[name + "_args"])
        cases[name] = dict(frames=stack(fr, hmax, wmax), hw=np.asarray([f.shape[:2] for f in fr], dtype=np.int32),
                           mats=z[name + "_mats"].astype(np.float64), angles=z[name + "_angles"].astype(np.float64),
                           kw=dict(pad=pad, origin=(ox, oy), out_hw=(oh, ow), fill=(r, g, b), size=size if size else None),
                           expect=z[name + "_expect"])
    return cases
