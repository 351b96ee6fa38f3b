"""Writes tests/golden/g25_jpeg_optimize.npz: for every case of g24_jpeg_encode.npz (whose images and coefficients it reuses) the
stream Pillow (libjpeg-turbo) writes with ``optimize=True``, and the length-limit case -- 17 distinct 8 x 8 gray blocks, their order
over a 2048 x 2048 image and Pillow's optimised stream of it at quality 50, whose AC table has been through the 16-bit limiter
(tests/jpeg_opt_ref.py ``limit_blocks``).  The restatement (tests/jpeg_opt_ref.py) is held to every stream here, but the stored
bytes are Pillow's.  Pillow and NumPy only; written with Pillow 12.2.0.

    python tests/golden/make_golden_jpeg_optimize.py"""
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_enc_ref as E  # noqa: E402
import jpeg_opt_ref as O  # noqa: E402
import jpeg_ref as R  # noqa: E402

PILLOW_SUBSAMPLING = {"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}


def pillow_bytes(img, quality, subsampling):
    buf = io.BytesIO()
    if img.ndim == 2:
        Image.fromarray(img, "L").save(buf, "JPEG", quality=quality, optimize=True)
    else:
        Image.fromarray(img, "RGB").save(buf, "JPEG", quality=quality, subsampling=PILLOW_SUBSAMPLING[subsampling], optimize=True)
    return buf.getvalue()


def build():
    cases, datas = E.load_fixture(), []
    for name, c in cases.items():
        gray = c["img"].ndim == 2
        data = pillow_bytes(c["img"], c["quality"], c["subsampling"])
        coef, qtab = R.entropy_decode(data)
        assert np.array_equal(R.flat_coef(coef), c["coef"]) and np.array_equal(qtab, c["qtab"]), name   # the same coefficients
        geo = E.geometry(*c["img"].shape[:2], 1 if gray else 3, *E.SAMPLING[c["subsampling"]])
        assert O.encode_optimized(E.split_coef(c["coef"], geo), geo, c["qtab"]) == data, name           # the restatement IS Pillow here
        datas.append(np.frombuffer(data, dtype=np.uint8))
    arrays = dict(data=np.concatenate(datas), data_off=np.concatenate([[0], np.cumsum([len(d) for d in datas])]).astype(np.int64))
    blocks, order = O.limit_blocks(), O.limit_order()
    img = O.limit_image(blocks, order)
    data = pillow_bytes(img, O.LIMIT_QUALITY, None)
    coef, qtab = R.entropy_decode(data)
    assert np.array_equal(R.flat_coef(coef), O.limit_coefficients(order)), "a block's coefficients are not the single term meant"
    tables = O.dht_tables(data)
    assert tables[1][0] == O.LIMIT_AC_COUNTS, tables[1][0]                                              # the limiter has acted
    geo = E.geometry(O.LIMIT_SIDE, O.LIMIT_SIDE, 1, 1, 1)
    assert O.encode_optimized(coef, geo, qtab) == data
    arrays.update(limit_blocks=blocks, limit_order=order, limit_data=np.frombuffer(data, dtype=np.uint8))
    return arrays


def main():
    arrays = build()
    np.savez_compressed(O.FIXTURE, **arrays)
    print(f"wrote {O.FIXTURE}: {len(arrays['data_off']) - 1} streams and the length-limit case, {os.path.getsize(O.FIXTURE)} bytes "
          f"(Pillow {Image.__version__})")


if __name__ == "__main__":
    main()
