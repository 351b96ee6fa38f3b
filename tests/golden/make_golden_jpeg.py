"""Writes tests/golden/g23_jpeg.npz: small baseline JPEG streams as Pillow (libjpeg-turbo) encodes them, Pillow's decoded RGB of
each (``Image.open(..).convert("RGB")``), and -- for the host decoder's test -- the coefficient and quantisation arrays of the
restatement (tests/jpeg_ref.py), which is first held to Pillow's bytes here.  Pillow and NumPy only; written with Pillow 12.2.0.

    python tests/golden/make_golden_jpeg.py [--dump DIR]

``--dump DIR`` also writes every stream (the refused ones included) as ``DIR/<name>.jpg``: the input of tools/jpeg_host_check.cpp.
No image is larger than 50 x 70."""
import argparse
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_ref as R  # noqa: E402

# name, (H, W), Pillow's save arguments (subsampling 0 / 1 / 2 = 4:4:4 / 4:2:2 / 4:2:0; None = grayscale)
CASES = [("s444_8x8", (8, 8), dict(subsampling=0)),
         ("s420_16x16", (16, 16), dict(subsampling=2)),
         ("s420_17x23", (17, 23), dict(subsampling=2, quality=75)),
         ("s422_33x41", (33, 41), dict(subsampling=1)),
         ("s444_40x56_rst4", (40, 56), dict(subsampling=0, restart_marker_blocks=4)),
         ("s420_41x39_rstrow", (41, 39), dict(subsampling=2, restart_marker_rows=1)),
         ("s420_50x70_q30opt", (50, 70), dict(subsampling=2, quality=30, optimize=True)),
         ("s420_50x70_q100", (50, 70), dict(subsampling=2, quality=100)),
         ("gray_24x31", (24, 31), dict(subsampling=None)),
         ("checker_24x24", (24, 24), dict(subsampling=2, quality=50))]
TRUNCATED = "s420_17x23_smooth"


def content(name, kind, h, w, g):
    if name.startswith("checker"):      # hard 0 / 255: cells of 4 pixels, or one random bit per pixel
        yy, xx = np.mgrid[0:h, 0:w]
        bit = ((yy // 4 + xx // 4) % 2) if kind == "smooth" else g.integers(0, 2, size=(h, w))
        return np.repeat((bit * 255).astype(np.uint8)[:, :, None], 3, axis=2)
    if kind == "noise":
        return g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(np.sin(xx / (4.0 + k) + k) + np.cos(yy / (6.0 - k) - k)) * 55 + 128 for k in range(3)], axis=2)
    return np.clip(img + g.normal(0, 2, img.shape), 0, 255).astype(np.uint8)


def encode(img, subsampling=0, **kw):
    buf = io.BytesIO()
    if subsampling is None:
        Image.fromarray(img, "RGB").convert("L").save(buf, "JPEG", **kw)
    else:
        Image.fromarray(img, "RGB").save(buf, "JPEG", subsampling=subsampling, **kw)
    return buf.getvalue()


def pillow_rgb(data):
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB")).copy()


def build():
    g = np.random.default_rng(23)
    arrays, names, streams = {}, [], {}
    for name, (h, w), kw in CASES:
        for kind in ("smooth", "noise"):
            data = encode(content(name, kind, h, w, g), **kw)
            rgb = pillow_rgb(data)
            assert rgb.shape == (h, w, 3)
            coef, qtab = R.entropy_decode(data)
            got = R.to_rgb(R.planes(coef, qtab), R.parse(data))
            assert np.array_equal(got, rgb), (name, kind, int((got != rgb).sum()))   # the restatement IS Pillow here
            full = f"{name}_{kind}"
            names.append(full)
            streams[full] = data
            arrays[full + "_data"] = np.frombuffer(data, dtype=np.uint8)
            arrays[full + "_rgb"] = rgb
            arrays[full + "_coef"] = R.flat_coef(coef)
            arrays[full + "_qtab"] = qtab
    smooth = content("x", "smooth", 24, 24, g)
    buf = io.BytesIO()
    Image.fromarray(smooth, "RGB").save(buf, "JPEG", progressive=True)
    refused = {"progressive": buf.getvalue()}
    buf = io.BytesIO()
    Image.fromarray(smooth, "RGB").convert("CMYK").save(buf, "JPEG")
    refused["cmyk"] = buf.getvalue()
    for k, v in refused.items():
        arrays["refused_" + k] = np.frombuffer(v, dtype=np.uint8)
        streams["refused_" + k] = v
    arrays["refused_names"] = np.asarray(sorted(refused))
    data = streams[TRUNCATED]
    hdr = R.parse(data)
    dqt, dht, scan, n = data.index(b"\xff\xdb"), data.index(b"\xff\xc4"), hdr["scan"], len(data)
    offs = sorted({1, 2, 3, dqt + 3, dqt + 30, data.index(b"\xff\xc0") + 6, dht + 2, dht + 25, scan - 3, scan, scan + 1,
                   scan + (n - scan) // 4, scan + (n - scan) // 2, n - 10, n - 3, n - 2, n - 1})
    arrays["truncated_case"] = np.asarray(TRUNCATED)
    arrays["truncated_offsets"] = np.asarray(offs, dtype=np.int32)
    arrays["case_names"] = np.asarray(names)
    return arrays, streams


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", default=None, help="also write every stream as DIR/<name>.jpg")
    a = ap.parse_args()
    arrays, streams = build()
    path = os.path.join(HERE, "g23_jpeg.npz")
    np.savez_compressed(path, **arrays)
    print(f"wrote {path}: {len(arrays['case_names'])} streams, {os.path.getsize(path)} bytes (Pillow {Image.__version__})")
    if a.dump:
        os.makedirs(a.dump, exist_ok=True)
        for name, data in streams.items():
            with open(os.path.join(a.dump, name + ".jpg"), "wb") as f:
                f.write(data)
        print(f"wrote {len(streams)} streams to {a.dump}")


if __name__ == "__main__":
    main()
