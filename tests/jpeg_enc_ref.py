"""NumPy / pure-Python restatement of the baseline JPEG encoder (csrc/jpeg_enc.hip, csrc/jpeg_huff_enc.h, include/vunet_jpeg_enc.h):
libjpeg's RGB -> YCbCr tables, its chroma down-sampling and edge padding, the integer "islow" forward DCT, the quantiser, the dummy
blocks of partial MCUs, the Annex K Huffman coding and the stream's segments, operation by operation: image -> coefficients -> bytes.
Shared by the CPU tests (tests/test_jpeg_enc_ref.py, tests/test_jpeg_enc_host.py), the fixture's writer
(tests/golden/make_golden_jpeg_encode.py, whose expected bytes are Pillow's, not this file's) and the kernels' tests
(tests/test_hip_jpeg_encode.py).  The coefficient layout is the decoder's (tests/jpeg_ref.py): one int16 array [bh, bw, 64] per
component, natural order, MCU-padded."""
from __future__ import annotations

import os

import numpy as np

from jpeg_ref import ZIGZAG

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g24_jpeg_encode.npz")
SAMPLING = {"4:4:4": (1, 1), "4:2:2": (2, 1), "4:2:0": (2, 2)}

# ---- Annex K: the base quantisation tables (natural order) and the four Huffman tables (code counts per length, symbols)
BASE_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51,
                      87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120,
                      101, 72, 92, 95, 98, 112, 100, 103, 99], dtype=np.int64)
BASE_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99,
                        99, 99, 99, 99] + [99] * 32, dtype=np.int64)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
           [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32,
            0x81, 0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16,
            0x17, 0x18, 0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45,
            0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
            0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94,
            0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6,
            0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8,
            0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
            0xf9, 0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
             [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
              0x08, 0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34,
              0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44,
              0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
              0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92,
              0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4,
              0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
              0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8,
              0xf9, 0xfa])


class OutOfRange(ValueError):
    """A coefficient outside baseline's range: a DC difference of more than 11 bits or an AC term of more than 10."""


def quant_tables(quality: int) -> np.ndarray:
    """libjpeg's jpeg_set_quality(.., force_baseline): [2, 64] uint16 in natural order, table 0 for luma, 1 for chroma."""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((b * scale + 50) // 100, 1, 255) for b in (BASE_LUMA, BASE_CHROMA)]).astype(np.uint16)


def geometry(H: int, W: int, ncomp: int, hs: int, vs: int) -> dict:
    """The decoder's header fields (tests/jpeg_ref.py ``parse``) of an H x W image and ``real``: per component the (hb, wb) blocks
    that hold image samples -- the rest of the MCU-padded grid are dummy blocks."""
    if ncomp == 1:
        hs = vs = 1
    mcu_cols, mcu_rows = -(-W // (8 * hs)), -(-H // (8 * vs))
    blocks = [(mcu_rows * vs, mcu_cols * hs)] + [(mcu_rows, mcu_cols)] * (ncomp - 1)
    real = [(-(-H // 8), -(-W // 8))] + [(-(-(-(-H // vs)) // 8), -(-(-(-W // hs)) // 8))] * (ncomp - 1)
    return dict(height=H, width=W, ncomp=ncomp, hsamp=hs, vsamp=vs, mcu_cols=mcu_cols, mcu_rows=mcu_rows, blocks=blocks, real=real,
                ncoef=64 * sum(a * b for a, b in blocks), restart=0)


def _fix(x: float) -> int:
    return int(x * 65536 + 0.5)


def from_rgb(img, hs: int, vs: int):
    """uint8 [H, W, 3] (or [H, W]: gray) -> (planes, geometry): one uint8 plane [bh * 8, bw * 8] per component, MCU-padded, level
    NOT shifted.  jccolor.c's tables; jcsample.c's h2v1 / h2v2 box filters on rows edge-replicated to the right (every full-resolution
    read is clamped to the last column); the full-resolution rows replicated only to a multiple of vsamp and the DOWN-SAMPLED last row
    replicated below that (jcprepct.c).  Luma is edge-replicated both ways."""
    img = np.asarray(img)
    gray = img.ndim == 2
    H, W = img.shape[:2]
    geo = geometry(H, W, 1 if gray else 3, hs, vs)
    hs, vs = geo["hsamp"], geo["vsamp"]
    (bh0, bw0) = geo["blocks"][0]
    ys, xs = np.minimum(np.arange(bh0 * 8), H - 1), np.minimum(np.arange(bw0 * 8), W - 1)
    if gray:
        return [img[ys][:, xs].astype(np.uint8)], geo
    r, g, b = (img[..., k].astype(np.int64) for k in range(3))
    y = (_fix(.299) * r + _fix(.587) * g + _fix(.114) * b + 32768) >> 16
    cb = (-_fix(.16874) * r - _fix(.33126) * g + _fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(.5) * r - _fix(.41869) * g - _fix(.08131) * b + (128 << 16) + 32767) >> 16
    out = [y[ys][:, xs].astype(np.uint8)]
    (bh1, bw1) = geo["blocks"][1]
    ch = -(-H // vs)
    cj, ci = np.minimum(np.arange(bh1 * 8), ch - 1), np.arange(bw1 * 8)
    for p in (cb, cr):
        if hs == 1:
            d = p[np.minimum(cj, H - 1)][:, np.minimum(ci, W - 1)]
        else:
            x0, x1 = np.minimum(2 * ci, W - 1), np.minimum(2 * ci + 1, W - 1)
            if vs == 1:
                rows = p[cj]
                d = (rows[:, x0] + rows[:, x1] + (ci & 1)) >> 1                                   # bias 0, 1, 0, 1, ...
            else:
                top, bot = p[np.minimum(2 * cj, H - 1)], p[np.minimum(2 * cj + 1, H - 1)]
                d = (top[:, x0] + top[:, x1] + bot[:, x0] + bot[:, x1] + 1 + (ci & 1)) >> 2      # bias 1, 2, 1, 2, ...
        out.append(d.astype(np.uint8))
    return out, geo


# ---- libjpeg's jfdctint.c (jpeg_fdct_islow): CONST_BITS 13, PASS1_BITS 2
_F = dict(f0_298=2446, f0_390=3196, f0_541=4433, f0_765=6270, f0_899=7373, f1_175=9633, f1_501=12299, f1_847=15137, f1_961=16069,
          f2_053=16819, f2_562=20995, f3_072=25172)


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_1d(v, first: bool):
    """One pass over the LAST axis of ``v`` [..., 8] int64.  The row pass (``first``) scales outputs 0 and 4 up by PASS1_BITS and
    descales the others by CONST_BITS - PASS1_BITS = 11; the column pass descales 0 and 4 by PASS1_BITS and the others by 15."""
    F = _F
    d = [v[..., k] for k in range(8)]
    tmp0, tmp7, tmp1, tmp6 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6]
    tmp2, tmp5, tmp3, tmp4 = d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    n = 11 if first else 15
    o = [None] * 8
    o[0] = (tmp10 + tmp11) << 2 if first else _descale(tmp10 + tmp11, 2)
    o[4] = (tmp10 - tmp11) << 2 if first else _descale(tmp10 - tmp11, 2)
    z1 = (tmp12 + tmp13) * F["f0_541"]
    o[2] = _descale(z1 + tmp13 * F["f0_765"], n)
    o[6] = _descale(z1 + tmp12 * -F["f1_847"], n)
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * F["f1_175"]
    tmp4, tmp5, tmp6, tmp7 = tmp4 * F["f0_298"], tmp5 * F["f2_053"], tmp6 * F["f3_072"], tmp7 * F["f1_501"]
    z1, z2, z3, z4 = z1 * -F["f0_899"], z2 * -F["f2_562"], z3 * -F["f1_961"], z4 * -F["f0_390"]
    z3, z4 = z3 + z5, z4 + z5
    o[7], o[5], o[3], o[1] = _descale(tmp4 + z1 + z3, n), _descale(tmp5 + z2 + z4, n), _descale(tmp6 + z2 + z3, n), \
        _descale(tmp7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def fdct_quant(blocks, q):
    """Sample blocks [..., 8, 8] uint8 and one table [64] -> coefficients [..., 64] int16: level shift, rows then columns, and the
    quantiser sign(c) * ((|c| + (d >> 1)) // d) with d = 8 q."""
    v = blocks.astype(np.int64) - 128
    rows = _fdct_1d(v, True)
    c = np.swapaxes(_fdct_1d(np.swapaxes(rows, -1, -2), False), -1, -2).reshape(blocks.shape[:-2] + (64,))
    d = q.astype(np.int64) * 8
    return (np.sign(c) * ((np.abs(c) + (d >> 1)) // d)).astype(np.int16)


def dummy_source(by: int, bx: int, hb: int, wb: int, hs: int):
    """The real block whose DC a dummy block (by >= hb or bx >= wb) repeats: jccoefct.c's "DC of the previous block of the MCU"
    chain in closed form (valid for vsamp <= 2).  ``hs``: the component's blocks per MCU row."""
    if by >= hb:
        return hb - 1, min((bx // hs) * hs + hs - 1, wb - 1)
    return by, wb - 1


def coefficients(planes, geo, qtab):
    """Planes of ``from_rgb`` -> one int16 array [bh, bw, 64] per component.  Dummy blocks are not transformed: AC 0, DC copied."""
    out = []
    for c, (p, (bh, bw), (hb, wb)) in enumerate(zip(planes, geo["blocks"], geo["real"])):
        blk = p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)
        co = np.zeros((bh, bw, 64), dtype=np.int16)
        co[:hb, :wb] = fdct_quant(blk[:hb, :wb], qtab[min(c, 1)])
        hs = geo["hsamp"] if c == 0 else 1
        for by in range(bh):
            for bx in range(bw):
                if by >= hb or bx >= wb:
                    co[by, bx, 0] = co[dummy_source(by, bx, hb, wb, hs) + (0,)]
        out.append(co)
    return out


def image_coefficients(img, quality=75, subsampling="4:2:0"):
    """-> (coefficients, qtab [ncomp, 64] uint16, geometry)."""
    planes, geo = from_rgb(img, *SAMPLING[subsampling])
    q2 = quant_tables(quality)
    return coefficients(planes, geo, q2), q2[[0, 1, 1][:geo["ncomp"]]], geo


# ---- the entropy coder and the stream
def _codes(table):
    counts, symbols = table
    book, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            book[symbols[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return book


class _BitWriter:
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code: int, length: int):
        self.acc, self.n = (self.acc << length) | code, self.n + length
        while self.n >= 8:
            self.n -= 8
            b = (self.acc >> self.n) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)                    # a stuffed zero after every 0xFF
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)    # the last byte is padded with 1-bits


def _block(bw, blk, pred, dc, ac):
    diff = int(blk[0]) - pred
    n = abs(diff).bit_length()
    if n > 11:
        raise OutOfRange(f"DC difference {diff}")
    bw.put(*dc[n])
    if n:
        bw.put((diff if diff >= 0 else diff - 1) & ((1 << n) - 1), n)
    zz = blk[ZIGZAG]
    last = 0
    for k in (np.flatnonzero(zz[1:]) + 1).tolist():
        v, run = int(zz[k]), k - last - 1
        while run > 15:
            bw.put(*ac[0xF0])
            run -= 16
        n = abs(v).bit_length()
        if n > 10:
            raise OutOfRange(f"AC term {v}")
        bw.put(*ac[(run << 4) | n])
        bw.put((v if v >= 0 else v - 1) & ((1 << n) - 1), n)
        last = k
    if last < 63:
        bw.put(*ac[0x00])


def _segment(marker: int, body: bytes) -> bytes:
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body


def _dht(cls_id: int, table) -> bytes:
    return _segment(0xC4, bytes([cls_id]) + bytes(table[0]) + bytes(table[1]))


def header(geo, qtab) -> bytes:
    """SOI, APP0, DQT(s), SOF0, DHTs, SOS as libjpeg's jcmarker.c writes them for a JFIF file with the default tables."""
    nc = geo["ncomp"]
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\0\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in range(2 if nc == 3 else 1):
        out += _segment(0xDB, bytes([t]) + bytes(int(v) for v in np.asarray(qtab[t])[ZIGZAG]))
    comps = b"".join(bytes([c + 1, (geo["hsamp"] << 4 | geo["vsamp"]) if c == 0 else 0x11, min(c, 1)]) for c in range(nc))
    out += _segment(0xC0, b"\x08" + geo["height"].to_bytes(2, "big") + geo["width"].to_bytes(2, "big") + bytes([nc]) + comps)
    out += _dht(0x00, DC_LUMA) + _dht(0x10, AC_LUMA)
    if nc == 3:
        out += _dht(0x01, DC_CHROMA) + _dht(0x11, AC_CHROMA)
    sel = b"".join(bytes([c + 1, 0x00 if c == 0 else 0x11]) for c in range(nc))
    return out + _segment(0xDA, bytes([nc]) + sel + b"\x00\x3f\x00")


def entropy_encode(coef, geo, qtab) -> bytes:
    """Coefficients (one [bh, bw, 64] array per component) and qtab [ncomp, 64] (component 0's and component 1's tables are
    written) -> the whole stream, SOI to EOI."""
    nc, hs, vs = geo["ncomp"], geo["hsamp"], geo["vsamp"]
    tabs = [qtab[0]] + ([qtab[1]] if nc == 3 else [])
    dc, ac = [_codes(DC_LUMA), _codes(DC_CHROMA)], [_codes(AC_LUMA), _codes(AC_CHROMA)]
    bw, pred = _BitWriter(), [0] * nc
    for my in range(geo["mcu_rows"]):
        for mx in range(geo["mcu_cols"]):
            for c in range(nc):
                ch, cv = (hs, vs) if c == 0 else (1, 1)
                for by in range(cv):
                    for bx in range(ch):
                        blk = coef[c][my * cv + by, mx * ch + bx]
                        _block(bw, blk, pred[c], dc[min(c, 1)], ac[min(c, 1)])
                        pred[c] = int(blk[0])
    bw.flush()
    return header(geo, tabs) + bytes(bw.out) + b"\xff\xd9"


def encode(img, quality=75, subsampling="4:2:0") -> bytes:
    coef, qtab, geo = image_coefficients(img, quality, subsampling)
    return entropy_encode(coef, geo, qtab)


def flat_coef(coef) -> np.ndarray:
    return np.concatenate([c.reshape(-1) for c in coef])


def split_coef(flat, geo):
    out, at = [], 0
    for bh, bw in geo["blocks"]:
        out.append(np.asarray(flat[at:at + bh * bw * 64]).reshape(bh, bw, 64))
        at += bh * bw * 64
    return out


# ---- the fixture's cases (tests/golden/make_golden_jpeg_encode.py writes them; Pillow is needed only there)
SIZES = [(1, 1), (8, 8), (16, 16), (17, 23), (24, 8), (8, 24), (250, 1), (1, 250), (37, 45), (64, 64)]
CONTENTS = ("noise", "ramp", "sat")
QUALITIES = (30, 75, 95, 100)
GRAY = [("gray_17x23_noise_q75", (17, 23), "noise", 75), ("gray_37x45_ramp_q95", (37, 45), "ramp", 95)]


def content(kind: str, h: int, w: int, g) -> np.ndarray:
    if kind == "noise":
        return g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    if kind == "sat":                                    # 0 or 255 per pixel and channel
        return (g.integers(0, 2, size=(h, w, 3)) * 255).astype(np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    return np.stack([(xx * 255) // max(w - 1, 1), (yy * 255) // max(h - 1, 1), ((xx + yy) * 255) // max(h + w - 2, 1)],
                    axis=2).astype(np.uint8)


def case_list():
    """[(name, image key, quality, subsampling or None for gray)], the order of the fixture."""
    out = []
    for h, w in SIZES:
        for kind in CONTENTS:
            for q in QUALITIES:
                for s in SAMPLING:
                    out.append((f"{h}x{w}_{kind}_q{q}_s{s.replace(':', '')}", f"{h}x{w}_{kind}", q, s))
    return out + [(name, f"{h}x{w}_{kind}", q, None) for name, (h, w), kind, q in GRAY]


def load_fixture():
    """tests/golden/g24_jpeg_encode.npz as {name: dict(img uint8 [H, W, 3] or [H, W] (gray), quality, subsampling ("4:4:4" for gray),
    data Pillow's bytes, coef int16 [ncoef] in the library's layout, qtab uint16 [ncomp, 64])}."""
    z = np.load(FIXTURE)
    data, coef, d_off, c_off = z["data"], z["coef"], z["data_off"], z["coef_off"]
    quals = {int(q): z["qtabs"][i] for i, q in enumerate(z["qualities"])}
    cases = {}
    for i, (name, key, q, s) in enumerate(case_list()):
        img = z["img_" + key]
        if s is None:
            img = z["gray_" + key]
        nc = 1 if s is None else 3
        cases[name] = dict(img=img, quality=q, subsampling=s or "4:4:4", data=data[d_off[i]:d_off[i + 1]].tobytes(),
                           coef=coef[c_off[i]:c_off[i + 1]], qtab=quals[q][[0, 1, 1][:nc]])
    return cases
