"""NumPy restatement of the raw-frame input route (csrc/image_input.hip, include/vunet_image_input.h): the crop window with the
border reflected, then Pillow's 8-bit bicubic ``Image.resize`` -- integer arithmetic on 22-bit fixed-point coefficients, horizontal
pass first -- restated so that it can be compared bit for bit: with Pillow itself where it is installed
(tests/test_image_input_ref.py, tests/golden/make_golden_image_input.py) and with the kernels (tests/test_hip_image_input.py).

Every coefficient is computed in Python floats (IEEE float64, one rounding per operation, no fused multiply-add) in the order
Pillow's ``precompute_coeffs`` / ``normalize_coeffs_8bpc`` use; the pixel sums are exact integers."""
import math
import os

import numpy as np

PRECISION_BITS = 22
PAD_BYTE = 0xAB
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g19_image_input.npz")


def bicubic(t: float) -> float:
    a = -0.5
    t = abs(t)
    if t < 1.0:
        return ((a + 2.0) * t - (a + 3.0)) * t * t + 1
    if t < 2.0:
        return (((t - 5) * t + 8) * t - 4) * a
    return 0.0


def ksize_of(in_size: int, out_size: int) -> int:
    scale = float(np.float32(in_size)) / out_size
    return int(math.ceil(2.0 * max(scale, 1.0))) * 2 + 1


def ksize_max(hmax: int, wmax: int, out_size: int) -> int:
    """The row length of the tables of a padded stack: the ksize of its larger side."""
    return ksize_of(max(hmax, wmax), out_size)


def tables(in_size: int, out_size: int, kmax: int = None):
    """(bounds [out, 2] int32: first source index and tap count; coef [out, kmax] int32, zeros past the count) of one axis.
    ``in_size == out_size`` -- the axis Pillow skips -- is the identity table (one tap of 2^22 on the pixel itself): with the
    rounding constant 2^21 the pass value is ``(2^21 + p 2^22) >> 22 == p``, the same bytes as no pass."""
    ks = ksize_of(in_size, out_size)
    kmax = ks if kmax is None else kmax
    assert kmax >= ks
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    coef = np.zeros((out_size, kmax), dtype=np.int32)
    if in_size == out_size:
        bounds[:, 0] = np.arange(out_size)
        bounds[:, 1] = 1
        coef[:, 0] = 1 << PRECISION_BITS
        return bounds, coef
    scale = float(np.float32(in_size)) / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, xmax)
        for x, v in enumerate(w):
            coef[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
    return bounds, coef


def _pass(img: np.ndarray, bounds: np.ndarray, coef: np.ndarray) -> np.ndarray:
    """One pass along axis 1 of img [rows, in, 3] uint8 -> [rows, out, 3] uint8."""
    out = np.empty((img.shape[0], bounds.shape[0], 3), dtype=np.uint8)
    src = img.astype(np.int64)
    for xx, (xmin, xmax) in enumerate(bounds):
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(src[:, xmin:xmin + xmax], coef[xx, :xmax].astype(np.int64), axes=([1], [0]))
        assert np.abs(acc).max() < 2 ** 31            # Pillow's (and the kernels') accumulator is an int32
        out[:, xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def resize(img: np.ndarray, size: int) -> np.ndarray:
    """``Image.fromarray(img).resize((size, size), Image.BICUBIC)`` of an [h, w, 3] uint8 image."""
    h, w = img.shape[:2]
    tmp = _pass(img, *tables(w, size))
    return _pass(tmp.transpose(1, 0, 2), *tables(h, size)).transpose(1, 0, 2)


def reflect(p, length: int):
    """cv2.BORDER_REFLECT (fedcba|abcdefgh|hgfedcb) of an index array: ``p = -p-1`` below 0, ``2 len - p - 1`` from len on,
    repeated until inside -- a triangle wave of period 2 len, taken here with one modulo."""
    q = np.mod(np.asarray(p, dtype=np.int64), 2 * length)
    return np.where(q >= length, 2 * length - 1 - q, q)


def reflect_loop(p: int, length: int) -> int:
    """The rule as the interface states it, one index at a time (the check of ``reflect``)."""
    if length == 1:
        return 0
    while p < 0 or p >= length:
        p = -p - 1 if p < 0 else 2 * length - p - 1
    return p


def window(frames: np.ndarray, n: int, row) -> np.ndarray:
    """The [ch, cw, 3] crop window of image n of a padded stack [N, Hmax, Wmax, 3] with geometry row (h, w, x0, y0, cw, ch)."""
    h, w, x0, y0, cw, ch = (int(v) for v in row)
    ys, xs = reflect(y0 + np.arange(ch), h), reflect(x0 + np.arange(cw), w)
    return frames[n][ys[:, None], xs[None, :]]


def geom_ok(row, hmax: int, wmax: int) -> bool:
    h, w, _, _, cw, ch = (int(v) for v in row)
    return 1 <= h <= hmax and 1 <= w <= wmax and 1 <= cw <= wmax and 1 <= ch <= hmax


def frames_to_u8(frames: np.ndarray, geom: np.ndarray, size: int):
    """(uint8 [N, size, size, 3], status [N] int32): a row that breaks the contract gives zeros and status 1."""
    n, hmax, wmax = frames.shape[:3]
    out = np.zeros((n, size, size, 3), dtype=np.uint8)
    status = np.zeros(n, dtype=np.int32)
    for i in range(n):
        if geom_ok(geom[i], hmax, wmax):
            out[i] = resize(window(frames, i, geom[i]), size)
        else:
            status[i] = 1
    return out, status


def to_float(u8: np.ndarray) -> np.ndarray:
    """torchvision's ``ToTensor`` and the ``x * 2 - 1`` lambda on [N, S, S, 3] uint8 -> [N, 3, S, S] float32."""
    x = u8.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255.0)
    return x * np.float32(2.0) - np.float32(1.0)


def bounding_rect(pts):
    """The assumed rule of ``cv2.boundingRect`` on float points (unpinned: cv2 is no dependency): x = floor(min),
    w = floor(max) - x + 1."""
    pts = np.asarray(pts, dtype=np.float64)[:, :2]
    x, y = int(math.floor(pts[:, 0].min())), int(math.floor(pts[:, 1].min()))
    return x, y, int(math.floor(pts[:, 0].max())) - x + 1, int(math.floor(pts[:, 1].max())) - y + 1


def stack(frames, hmax: int, wmax: int) -> np.ndarray:
    """Frames [h, w, 3] in one [N, hmax, wmax, 3] stack whose padding bytes are PAD_BYTE (they must never show)."""
    out = np.full((len(frames), hmax, wmax, 3), PAD_BYTE, dtype=np.uint8)
    for i, f in enumerate(frames):
        out[i, :f.shape[0], :f.shape[1]] = f
    return out


def load_fixture():
    """tests/golden/g19_image_input.npz (tests/golden/make_golden_image_input.py) as
    ``{name: dict(frames [1, Hmax, Wmax, 3], geom [1, 6], size, expect [1, S, S, 3])}`` plus the mixed batch under "batch"."""
    z = np.load(FIXTURE)
    cases = {}
    for i, name in enumerate(str(s) for s in z["case_names"]):
        hmax, wmax = (int(v) for v in z["case_stack"][i])
        cases[name] = dict(frames=stack([z["frame_" + str(z["case_frame"][i])]], hmax, wmax), geom=z["case_geom"][i:i + 1].copy(),
                           size=int(z["case_size"][i]), expect=z["expect_" + name][None])
    names = [str(s) for s in z["batch_cases"]]
    idx = [list(cases).index(n) for n in names]
    cases["batch"] = dict(frames=stack([z["frame_" + str(z["case_frame"][i])] for i in idx], 64, 64), geom=z["case_geom"][idx].copy(),
                          size=16, expect=np.stack([z["expect_" + n] for n in names]))
    return cases
