"""Writes tests/golden/g24_jpeg_encode.npz: small images, the baseline JPEG stream Pillow (libjpeg-turbo) writes for each at every
quality and sampling of the case list (tests/jpeg_enc_ref.py ``case_list``), and the quantised coefficients and tables decoded from
Pillow's bytes with the decoder's restatement (tests/jpeg_ref.py).  The encoder's restatement (tests/jpeg_enc_ref.py) is held to
Pillow's bytes here, but the stored bytes are Pillow's.  Pillow and NumPy only; written with Pillow 12.2.0.

    python tests/golden/make_golden_jpeg_encode.py

One image per (size, content) is stored once and shared by its 12 streams; streams and coefficients are stored as two long arrays
with offsets (a thousand zip members would cost more than their contents)."""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_enc_ref as E  # noqa: E402
import jpeg_ref as R  # noqa: E402

PILLOW_SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


def pillow_bytes(img, quality, subsampling):
    buf = io.BytesIO()
    if img.ndim == 2:
        Image.fromarray(img, "L").save(buf, "JPEG", quality=quality)
    else:
        Image.fromarray(img, "RGB").save(buf, "JPEG", quality=quality, subsampling=PILLOW_SUBSAMPLING[subsampling])
    return buf.getvalue()


def build():
    g = np.random.default_rng(24)
    arrays = {}
    for h, w in E.SIZES:
        for kind in E.CONTENTS:
            arrays[f"img_{h}x{w}_{kind}"] = E.content(kind, h, w, g)
    for _, (h, w), kind, _ in E.GRAY:
        arrays[f"gray_{h}x{w}_{kind}"] = np.ascontiguousarray(arrays[f"img_{h}x{w}_{kind}"][..., 1])
    datas, coefs, qtabs = [], [], {}
    for name, key, q, s in E.case_list():
        img = arrays[("gray_" if s is None else "img_") + key]
        data = pillow_bytes(img, q, s)
        coef, qtab = R.entropy_decode(data)
        want = E.quant_tables(q)
        assert np.array_equal(qtab, want[[0, 1, 1][:len(qtab)]]), name
        if len(qtab) == 3:
            qtabs.setdefault(q, np.stack([qtab[0], qtab[1]]))
            assert np.array_equal(qtabs[q], qtab[:2]), name
        mine = E.encode(img, q, s or "4:4:4")
        assert mine == data, (name, len(mine), len(data))        # the restatement IS Pillow here
        datas.append(np.frombuffer(data, dtype=np.uint8))
        coefs.append(R.flat_coef(coef))
    arrays["data"], arrays["coef"] = np.concatenate(datas), np.concatenate(coefs)
    arrays["data_off"] = np.concatenate([[0], np.cumsum([len(d) for d in datas])]).astype(np.int64)
    arrays["coef_off"] = np.concatenate([[0], np.cumsum([len(c) for c in coefs])]).astype(np.int64)
    arrays["qualities"] = np.asarray(sorted(qtabs), dtype=np.int32)
    arrays["qtabs"] = np.stack([qtabs[q] for q in sorted(qtabs)])
    return arrays


def main():
    arrays = build()
    np.savez_compressed(E.FIXTURE, **arrays)
    print(f"wrote {E.FIXTURE}: {len(arrays['data_off']) - 1} streams, {os.path.getsize(E.FIXTURE)} bytes (Pillow {Image.__version__})")


if __name__ == "__main__":
    main()
