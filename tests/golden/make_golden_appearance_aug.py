"""Writes tests/golden/g22_appearance_aug.npz: seeded uint8 frames, one output-to-input affine per image and what Pillow makes of
them -- ``Image.transform(AFFINE, BILINEAR, fillcolor)``, ``Image.rotate(BILINEAR)`` after ``np.pad(mode="reflect")``, slicing,
``Image.resize(BICUBIC)``.  Pillow and NumPy only; written with Pillow 12.2.0.

    python tests/golden/make_golden_appearance_aug.py

Every case is a small batch with one set of launch arguments.  No source is larger than 48 x 48."""
import math
import os
import random

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
WHITE, BLACK = (255, 255, 255), (0, 0, 0)


def affine_matrix(center, angle, translate, scale):
    """The inverse affine of torchvision 0.4.x's RandomAffine with shear 0 (its published formula, restated)."""
    a = math.radians(angle)
    s = 1.0 / scale
    d = math.cos(a) * math.cos(a) + math.sin(a) * math.sin(a)
    m = [s / d * v for v in (math.cos(a), math.sin(a), 0, -math.sin(a), math.cos(a), 0)]
    m[2] += m[0] * (-center[0] - translate[0]) + m[1] * (-center[1] - translate[1])
    m[5] += m[3] * (-center[0] - translate[0]) + m[4] * (-center[1] - translate[1])
    m[2] += center[0]
    m[5] += center[1]
    return [float(v) for v in m]


def rotate_matrix(w, h, angle):
    """The matrix ``Image.rotate`` hands to ``Image.transform`` (PIL/Image.py), restated; ``pillow_rotate`` checks it."""
    angle = angle % 360.0
    cx, cy = w / 2.0, h / 2.0
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def padded(frame, pad):
    return np.pad(frame, ((pad, pad), (pad, pad), (0, 0)), mode="reflect") if pad else frame


def pillow_affine(frame, mat, pad, origin, out_hw, fill):
    """``Image.transform`` of the reflect-padded frame, output size up to the window's far corner, sliced to the window."""
    (ox, oy), (oh, ow) = origin, out_hw
    assert ox >= 0 and oy >= 0
    im = Image.fromarray(padded(frame, pad), "RGB").transform((ox + ow, oy + oh), Image.AFFINE, tuple(mat), Image.BILINEAR, fillcolor=fill)
    return np.asarray(im)[oy:oy + oh, ox:ox + ow].copy()


def pillow_rotate(frame, angle, pad, origin, out_hw):
    """``Pad(reflect) -> Image.rotate(angle, BILINEAR) -> crop``: the window must lie inside the padded image."""
    (ox, oy), (oh, ow) = origin, out_hw
    p = padded(frame, pad)
    assert 0 <= ox and ox + ow <= p.shape[1] and 0 <= oy and oy + oh <= p.shape[0]
    im = Image.fromarray(p, "RGB").rotate(angle, resample=Image.BILINEAR)
    return np.asarray(im)[oy:oy + oh, ox:ox + ow].copy()


def center_origin(frame_hw, pad, crop):
    """torchvision's CenterCrop origin (x, y) on the padded image."""
    H, W = frame_hw[0] + 2 * pad, frame_hw[1] + 2 * pad
    return int(round((W - crop) / 2.)), int(round((H - crop) / 2.))


def build_cases():
    """-> (frames list, {name: dict(frames idx list, stack (hmax, wmax), mats, angles, args, expect)})."""
    g = np.random.default_rng(22)
    rnd = random.Random(22)
    frames, cases = [], {}

    def frame(h, w):
        frames.append(g.integers(0, 256, size=(h, w, 3), dtype=np.uint8))
        return len(frames) - 1

    def draw(h, w):
        angle, tx, _, scale = rnd.uniform(-30, 30), round(rnd.uniform(-0.3 * w, 0.3 * w)), rnd.uniform(-0.0, 0.0), rnd.uniform(0.7, 1)
        return affine_matrix((w * 0.5 + 0.5, h * 0.5 + 0.5), angle, (tx, 0), scale)

    def add(name, idx, mats, angles, pad, origin, out_hw, fill, size=0, stack=None):
        hs, ws = [frames[i].shape[0] for i in idx], [frames[i].shape[1] for i in idx]
        outs = []
        for i, m, a in zip(idx, mats, angles):
            o = pillow_affine(frames[i], m, pad, origin, out_hw, fill)
            if not math.isnan(a):   # Pillow's own rotate, and the restated matrix gives its bytes
                assert np.array_equal(o, pillow_rotate(frames[i], a, pad, origin, out_hw)), (name, a)
                o = pillow_rotate(frames[i], a, pad, origin, out_hw)
            if size:
                o = np.asarray(Image.fromarray(o, "RGB").resize((size, size), Image.BICUBIC))
            outs.append(o)
        cases[name] = dict(frames=np.asarray(idx, dtype=np.int32), stack=np.asarray(stack or (max(hs), max(ws)), dtype=np.int32),
                           mats=np.asarray(mats, dtype=np.float64), angles=np.asarray(angles, dtype=np.float64),
                           args=np.asarray([pad, *origin, *out_hw, *fill, size], dtype=np.int32), expect=np.stack(outs))

    nan = float("nan")
    sizes = [(24, 24), (17, 29), (32, 20)]
    src = [frame(h, w) for h, w in sizes]
    for i, (h, w) in zip(src, sizes):                                # random draws, window = frame
        add(f"affine_{h}x{w}", [i], [draw(h, w)], [nan], 0, (0, 0), (h, w), WHITE)
    add("affine_identity", [src[0]], [affine_matrix((12.5, 12.5), 0.0, (0, 0), 1.0)], [nan], 0, (0, 0), (24, 24), WHITE)
    assert np.array_equal(cases["affine_identity"]["expect"][0], frames[src[0]])
    h, w = sizes[2]                                                  # scale 0.7 and the largest translation: large filled regions
    add("affine_far", [src[2], src[2]], [affine_matrix((w * 0.5 + 0.5, h * 0.5 + 0.5), a, (t, 0), 0.7) for a, t in ((30.0, 6), (-30.0, -6))],
        [nan, nan], 0, (0, 0), (h, w), WHITE)
    assert (cases["affine_far"]["expect"] == 255).all(axis=-1).mean() > 0.25
    # the three sizes in one stack (padding 0xAB), the window the whole 34 x 31 slot: more than any frame
    add("affine_mixed", src, [draw(h, w) for h, w in sizes], [nan] * 3, 0, (0, 0), (34, 31), WHITE, stack=(34, 31))
    r = frame(32, 16)                                                # Market's form: pad, rotate, centre crop
    ang = rnd.uniform(-90, 90)
    add("rotate_32x16", [r], [rotate_matrix(32, 48, ang)], [ang], 8, center_origin((32, 16), 8, 16), (16, 16), BLACK)
    angs = [90.0, -90.0, 0.0, 45.0, rnd.uniform(-90, 90)]
    add("rotate_24x24", [src[0]] * 5, [rotate_matrix(36, 36, a) for a in angs], angs, 6, center_origin((24, 24), 6, 24), (24, 24), BLACK)
    t = frame(20, 6)                                                 # pad 8 > w - 1: the reflection repeats
    angs = [rnd.uniform(-90, 90), 77.0]
    add("rotate_20x6", [t, t], [rotate_matrix(22, 36, a) for a in angs], angs, 8, center_origin((20, 6), 8, 16), (16, 16), BLACK)
    o = frame(12, 1)                                                 # one pixel wide: every column is column 0
    angs = [rnd.uniform(-90, 90), -35.0]
    add("rotate_12x1", [o, o], [rotate_matrix(9, 20, a) for a in angs], angs, 4, center_origin((12, 1), 4, 8), (8, 8), BLACK)
    ang = rnd.uniform(-90, 90)                                       # the chain: crop 16, then Resize(12, BICUBIC)
    add("chain_32x16", [r], [rotate_matrix(32, 48, ang)], [ang], 8, center_origin((32, 16), 8, 16), (16, 16), BLACK, size=12)
    return frames, cases


def main():
    frames, cases = build_cases()
    arrays = {"case_names": np.asarray(list(cases))}
    for i, f in enumerate(frames):
        arrays[f"frame_{i}"] = f
    for name, c in cases.items():
        for k, v in c.items():
            arrays[f"{name}_{k}"] = v
    path = os.path.join(HERE, "g22_appearance_aug.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {len(cases)} cases, {os.path.getsize(path)} bytes (Pillow {Image.__version__})")


if __name__ == "__main__":
    main()
