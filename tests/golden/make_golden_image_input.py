"""Writes tests/golden/g19_image_input.npz: seeded uint8 frames, crop geometry and what Pillow's ``Image.resize(..., BICUBIC)``
makes of each reflected crop window.  Needs Pillow (the fixture was written with 12.2.0); the tests need only the file.

    python tests/golden/make_golden_image_input.py

Every expected output is made without the restatement of the tests: the frame is padded with ``np.pad(mode="symmetric")`` (the
border rule of cv2.BORDER_REFLECT, repeated where the pad exceeds the frame), the window sliced out of the padded frame and
handed to Pillow.  Keys: ``frame_<f>`` [h, w, 3] uint8; ``case_names`` / ``case_frame`` (strings), ``case_size`` (S),
``case_geom`` [K, 6] (h, w, x0, y0, cw, ch), ``case_stack`` [K, 2] (Hmax, Wmax of the padded stack the single case runs in);
``expect_<case>`` [S, S, 3] uint8; ``batch_cases``: the cases of the mixed batch (one 64 x 64 stack, S = 16)."""
import os

import numpy as np
import PIL
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))


def frames():
    g = np.random.default_rng(19)
    f = {name: g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
         for name, (h, w) in {"37x53": (37, 53), "16x40": (16, 40), "1x7": (1, 7), "61x64": (61, 64), "23x17": (23, 17),
                              "40x10": (40, 10)}.items()}
    f["8x5"] = (g.integers(0, 2, size=(8, 5, 3)) * 255).astype(np.uint8)        # both clamp ends: the overshoot of an upscaled edge
    yy, xx = np.mgrid[0:40, 0:48]
    smooth = np.stack([4 * xx + yy, 255 - 5 * yy, (xx * yy) // 8], axis=2)      # a frame with structure: a shifted window shows
    f["40x48"] = ((smooth + g.integers(0, 24, size=smooth.shape)) % 256).astype(np.uint8)
    return f


# name, frame, S, (x0, y0, cw, ch) or None for the whole frame, (Hmax, Wmax) or None for the frame's own size
CASES = [("down_37x53", "37x53", 16, None, None),
         ("up_8x5", "8x5", 16, None, None),
         ("skip_16x40", "16x40", 16, None, None),
         ("flat_1x7", "1x7", 4, None, None),
         ("down_61x64", "61x64", 32, None, None),
         ("down_23x17", "23x17", 16, None, None),
         ("crop_inside", "40x48", 16, (5, 6, 30, 25), None),
         ("crop_left_top", "40x48", 16, (-7, -4, 33, 29), None),
         ("crop_right_bottom", "40x48", 16, (20, 18, 37, 31), (40, 57)),
         ("crop_wider_than_frame", "40x10", 16, (-17, -5, 45, 50), (64, 64))]
BATCH = ["crop_inside", "down_37x53", "crop_left_top", "up_8x5", "crop_right_bottom", "skip_16x40", "crop_wider_than_frame",
         "down_23x17"]


def pillow_window(frame, x0, y0, cw, ch, size):
    h, w = frame.shape[:2]
    left, top = max(0, -x0), max(0, -y0)
    right, bottom = max(0, x0 + cw - w), max(0, y0 + ch - h)
    padded = np.pad(frame, ((top, bottom), (left, right), (0, 0)), mode="symmetric")
    win = np.ascontiguousarray(padded[y0 + top:y0 + top + ch, x0 + left:x0 + left + cw])
    assert win.shape == (ch, cw, 3)
    return np.asarray(Image.fromarray(win, "RGB").resize((size, size), Image.BICUBIC))


def main():
    f = frames()
    out = {f"frame_{k}": v for k, v in f.items()}
    geom, stack = [], []
    for name, fr, size, win, st in CASES:
        h, w = f[fr].shape[:2]
        x0, y0, cw, ch = win or (0, 0, w, h)
        geom.append((h, w, x0, y0, cw, ch))
        stack.append(st or (max(h, ch), max(w, cw)))
        out[f"expect_{name}"] = pillow_window(f[fr], x0, y0, cw, ch, size)
    out.update(case_names=np.array([c[0] for c in CASES]), case_frame=np.array([c[1] for c in CASES]),
               case_size=np.array([c[2] for c in CASES], dtype=np.int32), case_geom=np.array(geom, dtype=np.int32),
               case_stack=np.array(stack, dtype=np.int32), batch_cases=np.array(BATCH))
    lo, hi = out["expect_up_8x5"].min(), out["expect_up_8x5"].max()
    assert lo == 0 and hi == 255, (lo, hi)
    path = os.path.join(HERE, "g19_image_input.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(CASES)} cases, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
