"""NumPy / pure-Python restatement of the baseline JPEG decoder (csrc/jpeg_entropy.h, csrc/jpeg.hip, include/vunet_jpeg.h): the
marker parse, the Huffman walk, libjpeg's integer "islow" inverse DCT, its "fancy" chroma up-sampling and its YCbCr -> RGB
conversion, operation by operation.  Shared by the CPU tests (tests/test_jpeg_ref.py, tests/test_jpeg_host.py), the fixture's writer
(tests/golden/make_golden_jpeg.py, which does NOT use it to make the expected bytes -- those are Pillow's) and the kernels' tests
(tests/test_hip_jpeg.py).  Slow by design: one bit at a time, one block at a time where that is the plainest statement."""
from __future__ import annotations

import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g23_jpeg.npz")

# zigzag position -> natural (row-major) position of an 8 x 8 block
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63], dtype=np.int64)


class Unsupported(ValueError):
    """A well-formed stream outside the supported subset (progressive, 16-bit tables, CMYK, other samplings, several scans)."""


class Corrupt(ValueError):
    """A truncated or malformed stream."""


def _u16(d, p):
    if p + 2 > len(d):
        raise Corrupt("truncated")
    return (d[p] << 8) | d[p + 1]


def parse(data) -> dict:
    """The header up to and including SOS -> dict(height, width, ncomp, hsamp, vsamp (of component 0 against 1 x 1 chroma; 1, 1 for
    one component), mcu_cols, mcu_rows, blocks [(bh, bw) per component, MCU-padded], ncoef, restart, qtab [ncomp, 64] uint16 in
    natural order, dc / ac [(counts, symbols) per component], scan (offset of the entropy-coded data))."""
    d = bytes(data)
    if len(d) < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise Corrupt("no SOI")
    p, qt, huff, frame, restart, jfif, adobe = 2, {}, {}, None, 0, False, None
    while True:
        if p >= len(d):
            raise Corrupt("truncated")
        if d[p] != 0xFF:
            raise Corrupt("marker expected")
        while p < len(d) and d[p] == 0xFF:
            p += 1
        if p >= len(d):
            raise Corrupt("truncated")
        m = d[p]
        p += 1
        if m == 0xD9 or m == 0xD8 or m == 0 or 0xD0 <= m <= 0xD7:
            raise Corrupt("marker out of place")
        if m == 0x01:
            continue
        n = _u16(d, p)
        if n < 2 or p + n > len(d):
            raise Corrupt("segment length")
        seg, p = d[p + 2:p + n], p + n
        if m == 0xDB:
            q = 0
            while q < len(seg):
                pq, tq = seg[q] >> 4, seg[q] & 15
                if pq != 0:
                    raise Unsupported("16-bit quantisation table")
                if tq > 3 or q + 65 > len(seg):
                    raise Corrupt("DQT")
                t = np.zeros(64, dtype=np.uint16)
                t[ZIGZAG] = np.frombuffer(seg[q + 1:q + 65], dtype=np.uint8)
                qt[tq], q = t, q + 65
        elif m == 0xC0:
            if len(seg) < 6:
                raise Corrupt("SOF0")
            if seg[0] != 8:
                raise Unsupported("sample precision")
            h, w, nc = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if nc == 4:
                raise Unsupported("4 components")
            if nc not in (1, 3):
                raise Unsupported("component count")
            if len(seg) != 6 + 3 * nc or h < 1 or w < 1 or frame is not None:
                raise Corrupt("SOF0")
            frame = dict(height=h, width=w, comps=[(seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i])
                                                   for i in range(nc)])
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            raise Unsupported("progressive / extended / lossless / arithmetic frame")
        elif m == 0xC4:
            q = 0
            while q < len(seg):
                tc, th = seg[q] >> 4, seg[q] & 15
                if tc > 1 or th > 3 or q + 17 > len(seg):
                    raise Corrupt("DHT")
                counts = list(seg[q + 1:q + 17])
                total = sum(counts)
                if total > 256 or q + 17 + total > len(seg):
                    raise Corrupt("DHT")
                code = 0
                for length, c in enumerate(counts, 1):   # the canonical codes must fit their lengths
                    code += c
                    if code > (1 << length):
                        raise Corrupt("DHT")
                    code <<= 1
                huff[(tc, th)] = (counts, list(seg[q + 17:q + 17 + total]))
                q += 17 + total
        elif m == 0xDD:
            if len(seg) != 2:
                raise Corrupt("DRI")
            restart = (seg[0] << 8) | seg[1]
        elif m == 0xE0 and seg[:5] == b"JFIF\0":
            jfif = True
        elif m == 0xEE and seg[:5] == b"Adobe" and len(seg) >= 12:
            adobe = seg[11]
        elif m == 0xDA:
            if frame is None:
                raise Corrupt("SOS before SOF")
            nc = len(frame["comps"])
            if len(seg) < 1:
                raise Corrupt("SOS")
            ns = seg[0]
            if ns != nc:
                if 1 <= ns < nc:
                    raise Unsupported("several scans")
                raise Corrupt("SOS")
            if len(seg) != 4 + 2 * ns:
                raise Corrupt("SOS")
            sel = []
            for i in range(ns):
                if seg[1 + 2 * i] != frame["comps"][i][0]:
                    raise Corrupt("SOS component")
                sel.append((seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15))
            if seg[1 + 2 * ns] != 0 or seg[2 + 2 * ns] != 63 or seg[3 + 2 * ns] != 0:
                raise Corrupt("SOS spectral selection")
            break
        # every other segment (APPn, COM, ...) is skipped
    comps = frame["comps"]
    nc = len(comps)
    if nc == 3:
        if adobe is not None and adobe != 1:
            raise Unsupported("Adobe transform")
        if adobe is None and not jfif and [c[0] for c in comps] == [82, 71, 66]:
            raise Unsupported("RGB components")
        hs, vs = comps[0][1], comps[0][2]
        if (hs, vs) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
            raise Unsupported("sampling")
    else:
        if comps[0][1] < 1 or comps[0][2] < 1:
            raise Corrupt("sampling")
        hs, vs = 1, 1                                   # a one-component scan is not interleaved: one block per MCU
    H, W = frame["height"], frame["width"]
    mcu_cols, mcu_rows = -(-W // (8 * hs)), -(-H // (8 * vs))
    blocks = [(mcu_rows * vs, mcu_cols * hs)] + [(mcu_rows, mcu_cols)] * (nc - 1)
    qtab = np.zeros((nc, 64), dtype=np.uint16)
    dc, ac = [], []
    for i, (_, _, _, tq) in enumerate(comps):
        if tq not in qt or (0, sel[i][0]) not in huff or (1, sel[i][1]) not in huff:
            raise Corrupt("missing table")
        qtab[i] = qt[tq]
        dc.append(huff[(0, sel[i][0])])
        ac.append(huff[(1, sel[i][1])])
    return dict(height=H, width=W, ncomp=nc, hsamp=hs, vsamp=vs, mcu_cols=mcu_cols, mcu_rows=mcu_rows, blocks=blocks,
                ncoef=64 * sum(a * b for a, b in blocks), restart=restart, qtab=qtab, dc=dc, ac=ac, scan=p)


class _Bits:
    def __init__(self, d, p):
        self.d, self.p, self.acc, self.n = d, p, 0, 0

    def bit(self) -> int:
        if self.n == 0:
            d, p = self.d, self.p
            if p >= len(d):
                raise Corrupt("truncated scan")
            b = d[p]
            if b == 0xFF:
                if p + 1 >= len(d):
                    raise Corrupt("truncated scan")
                if d[p + 1] != 0:
                    raise Corrupt("marker inside the scan")
                p += 1
            self.p, self.acc, self.n = p + 1, b, 8
        self.n -= 1
        return (self.acc >> self.n) & 1

    def bits(self, s: int) -> int:
        v = 0
        for _ in range(s):
            v = (v << 1) | self.bit()
        return v

    def restart(self, k: int):
        self.n, d, p = 0, self.d, self.p
        if p >= len(d) or d[p] != 0xFF:
            raise Corrupt("truncated scan" if p >= len(d) else "restart marker expected")
        while p < len(d) and d[p] == 0xFF:
            p += 1
        if p >= len(d):
            raise Corrupt("truncated scan")
        if d[p] != 0xD0 + (k & 7):
            raise Corrupt("restart marker expected")
        self.p = p + 1


def _codebook(table):
    counts, symbols = table
    book, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            book[(length, code)] = symbols[k]
            code, k = code + 1, k + 1
        code <<= 1
    return book


def _symbol(br, book) -> int:
    code = 0
    for length in range(1, 17):
        code = (code << 1) | br.bit()
        s = book.get((length, code))
        if s is not None:
            return s
    raise Corrupt("bad Huffman code")


def _extend(v: int, s: int) -> int:
    return v if s == 0 or v >= (1 << (s - 1)) else v - (1 << s) + 1


def entropy_decode(data, hdr=None):
    """-> (coefficients: one int16 array [bh, bw, 64] per component -- natural order, unquantised, DC prediction undone --,
    qtab [ncomp, 64] uint16 in natural order)."""
    d = bytes(data)
    hdr = parse(d) if hdr is None else hdr
    nc, hs, vs = hdr["ncomp"], hdr["hsamp"], hdr["vsamp"]
    coef = [np.zeros((bh, bw, 64), dtype=np.int16) for bh, bw in hdr["blocks"]]
    dcb, acb = [_codebook(t) for t in hdr["dc"]], [_codebook(t) for t in hdr["ac"]]
    br, pred, ri, nrst = _Bits(d, hdr["scan"]), [0] * nc, hdr["restart"], 0
    for mcu in range(hdr["mcu_cols"] * hdr["mcu_rows"]):
        if ri and mcu and mcu % ri == 0:
            br.restart(nrst)
            nrst, pred = nrst + 1, [0] * nc
        my, mx = divmod(mcu, hdr["mcu_cols"])
        for c in range(nc):
            ch, cv = (hs, vs) if c == 0 else (1, 1)
            for by in range(cv):
                for bx in range(ch):
                    blk = coef[c][my * cv + by, mx * ch + bx]
                    s = _symbol(br, dcb[c])
                    if s > 15:
                        raise Corrupt("bad DC category")
                    pred[c] += _extend(br.bits(s), s)
                    blk[0] = np.int64(pred[c]).astype(np.int16)
                    k = 1
                    while k < 64:
                        rs = _symbol(br, acb[c])
                        r, s = rs >> 4, rs & 15
                        if s == 0:
                            if r != 15:
                                break
                            k += 16
                            continue
                        k += r
                        if k > 63:
                            raise Corrupt("coefficient index past 63")
                        blk[ZIGZAG[k]] = _extend(br.bits(s), s)
                        k += 1
    return coef, hdr["qtab"].copy()


# ---- libjpeg's jidctint.c (jpeg_idct_islow): CONST_BITS 13, PASS1_BITS 2, 64-bit integers
_F = dict(f0_298=2446, f0_390=3196, f0_541=4433, f0_765=6270, f0_899=7373, f1_175=9633, f1_501=12299, f1_847=15137, f1_961=16069,
          f2_053=16819, f2_562=20995, f3_072=25172)


def _idct_1d(v, shift_even, descale):
    """One pass over the LAST axis of ``v`` [..., 8] int64: the even part is shifted up by ``shift_even`` = CONST_BITS, the result
    descaled (rounded arithmetic shift) by ``descale``."""
    F = _F
    z2, z3 = v[..., 2], v[..., 6]
    z1 = (z2 + z3) * F["f0_541"]
    tmp2 = z1 + z3 * -F["f1_847"]
    tmp3 = z1 + z2 * F["f0_765"]
    z2, z3 = v[..., 0], v[..., 4]
    tmp0, tmp1 = (z2 + z3) << shift_even, (z2 - z3) << shift_even
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    tmp0, tmp1, tmp2, tmp3 = v[..., 7], v[..., 5], v[..., 3], v[..., 1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = (z3 + z4) * F["f1_175"]
    tmp0, tmp1, tmp2, tmp3 = tmp0 * F["f0_298"], tmp1 * F["f2_053"], tmp2 * F["f3_072"], tmp3 * F["f1_501"]
    z1, z2, z3, z4 = z1 * -F["f0_899"], z2 * -F["f2_562"], z3 * -F["f1_961"], z4 * -F["f0_390"]
    z3, z4 = z3 + z5, z4 + z5
    tmp0, tmp1, tmp2, tmp3 = tmp0 + z1 + z3, tmp1 + z2 + z4, tmp2 + z2 + z3, tmp3 + z1 + z4
    out = np.stack([tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3],
                   axis=-1)
    return (out + (1 << (descale - 1))) >> descale


def idct_islow(coef, q):
    """Coefficient blocks [..., 64] int16 and one table [64] -> samples [..., 8, 8] uint8: dequantise, the column pass (descale
    CONST_BITS - PASS1_BITS = 11), the row pass (descale CONST_BITS + PASS1_BITS + 3 = 18), + 128, clamp."""
    v = (coef.astype(np.int64) * q.astype(np.int64)).reshape(coef.shape[:-1] + (8, 8))
    ws = np.swapaxes(_idct_1d(np.swapaxes(v, -1, -2), 13, 11), -1, -2)     # columns
    return np.clip(_idct_1d(ws, 13, 18) + 128, 0, 255).astype(np.uint8)    # rows


def planes(coef, qtab):
    """-> one uint8 plane [bh * 8, bw * 8] per component (block-padded)."""
    out = []
    for c, q in zip(coef, qtab):
        s = idct_islow(c, q)                                                # [bh, bw, 8, 8]
        out.append(np.ascontiguousarray(s.transpose(0, 2, 1, 3)).reshape(c.shape[0] * 8, c.shape[1] * 8))
    return out


def upsample(plane, hs: int, vs: int, H: int, W: int):
    """libjpeg's up-sampling of one chroma plane (block-padded) to [H, W] int64, on the real down-sampled extent ``ceil(W / hs)`` x
    ``ceil(H / vs)`` with the edges replicated.  "Fancy" (triangle) filters where the down-sampled width is more than 2 -- libjpeg's
    own condition --, plain replication below that."""
    cw, ch = -(-W // hs), -(-H // vs)
    p = plane[:ch, :cw].astype(np.int64)
    if hs == 1 and vs == 1:
        return p[:H, :W]
    if cw <= 2:
        return np.repeat(np.repeat(p, vs, axis=0), hs, axis=1)[:H, :W]
    out = np.zeros((H, W), dtype=np.int64)
    for y in range(H):
        if vs == 2:
            j = y >> 1
            far = max(j - 1, 0) if y % 2 == 0 else min(j + 1, ch - 1)
            s = 3 * p[j] + p[far]                                           # [cw]
        else:
            s = p[y]
        for x in range(W):
            i = x >> 1
            if vs == 2:
                if x % 2 == 0:
                    out[y, x] = (4 * s[i] + 8) >> 4 if i == 0 else (3 * s[i] + s[i - 1] + 8) >> 4
                else:
                    out[y, x] = (4 * s[i] + 7) >> 4 if i == cw - 1 else (3 * s[i] + s[i + 1] + 7) >> 4
            else:
                if x % 2 == 0:
                    out[y, x] = s[i] if i == 0 else (3 * s[i] + s[i - 1] + 1) >> 2
                else:
                    out[y, x] = s[i] if i == cw - 1 else (3 * s[i] + s[i + 1] + 2) >> 2
    return out


def to_rgb(pl, hdr):
    """Component planes -> RGB [H, W, 3] uint8 (grayscale: R = G = B = Y)."""
    H, W = hdr["height"], hdr["width"]
    y = pl[0][:H, :W].astype(np.int64)
    if hdr["ncomp"] == 1:
        return np.repeat(y[:, :, None], 3, axis=2).astype(np.uint8)
    cb = upsample(pl[1], hdr["hsamp"], hdr["vsamp"], H, W) - 128
    cr = upsample(pl[2], hdr["hsamp"], hdr["vsamp"], H, W) - 128
    r = y + ((91881 * cr + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], axis=2), 0, 255).astype(np.uint8)


def decode(data) -> np.ndarray:
    hdr = parse(data)
    coef, qtab = entropy_decode(data, hdr)
    return to_rgb(planes(coef, qtab), hdr)


def flat_coef(coef) -> np.ndarray:
    """The library's layout: [component][block row][block column][64], one int16 vector."""
    return np.concatenate([c.reshape(-1) for c in coef])


def load_fixture():
    """tests/golden/g23_jpeg.npz (tests/golden/make_golden_jpeg.py) as ``dict(cases = {name: dict(data bytes, rgb [H, W, 3] Pillow's,
    coef int16 [ncoef], qtab uint16 [ncomp, 64])}, refused = {name: bytes}, truncated = (name of the case, [offsets]))``."""
    z = np.load(FIXTURE)
    cases = {}
    for name in (str(s) for s in z["case_names"]):
        cases[name] = dict(data=z[name + "_data"].tobytes(), rgb=z[name + "_rgb"], coef=z[name + "_coef"], qtab=z[name + "_qtab"])
    refused = {str(s): z["refused_" + str(s)].tobytes() for s in z["refused_names"]}
    return dict(cases=cases, refused=refused, truncated=(str(z["truncated_case"]), [int(v) for v in z["truncated_offsets"]]))
