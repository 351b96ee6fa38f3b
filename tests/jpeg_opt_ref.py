"""NumPy / pure-Python restatement of the optimised Huffman tables of the JPEG encoder (csrc/jpeg_huff_enc.h: symbol_histogram,
optimal_table, entropy_encode_tables): the symbols the coder emits, counted; libjpeg's jpeg_gen_optimal_table; and the stream with
the tables it gives -- what Pillow's ``Image.save(.., "JPEG", optimize=True)`` writes.  Builds on tests/jpeg_enc_ref.py (layout, bit
writer, segments).  Shared by tests/test_jpeg_opt_host.py, tests/test_hip_jpeg_entropy.py and the fixture's writer
(tests/golden/make_golden_jpeg_optimize.py, whose expected bytes are Pillow's, not this file's)."""
from __future__ import annotations

import os

import numpy as np

import jpeg_enc_ref as E
from jpeg_ref import ZIGZAG

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g25_jpeg_optimize.npz")
LIMIT_SIDE, LIMIT_QUALITY = 2048, 50
LIMIT_AC_COUNTS = [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 3]


def scan_blocks(coef, geo):
    """(component, block [64]) in scan order: MCUs left to right, top to bottom; per MCU component by component, row-major."""
    nc, hs, vs = geo["ncomp"], geo["hsamp"], geo["vsamp"]
    for my in range(geo["mcu_rows"]):
        for mx in range(geo["mcu_cols"]):
            for c in range(nc):
                ch, cv = (hs, vs) if c == 0 else (1, 1)
                for by in range(cv):
                    for bx in range(ch):
                        yield c, coef[c][my * cv + by, mx * ch + bx]


def block_symbols(blk, pred):
    """-> (DC symbol, [AC symbols]) of one block: the DC difference's bit length; one 0xF0 per 16 zeros of a run, (run << 4) | size
    per non-zero term, 0x00 where the block does not end at position 63."""
    n = abs(int(blk[0]) - pred).bit_length()
    if n > 11:
        raise E.OutOfRange("DC difference")
    zz, last, out = blk[ZIGZAG], 0, []
    for k in (np.flatnonzero(zz[1:]) + 1).tolist():
        run, size = k - last - 1, abs(int(zz[k])).bit_length()
        if size > 10:
            raise E.OutOfRange("AC term")
        out += [0xF0] * (run // 16) + [((run % 16) << 4) | size]
        last = k
    if last < 63:
        out.append(0x00)
    return n, out


def histogram(coef, geo) -> np.ndarray:
    """uint32 [4, 256] in DHT order DC0, AC0, DC1, AC1 (gray: the last two stay zero)."""
    hist, pred = np.zeros((4, 256), dtype=np.uint32), [0] * geo["ncomp"]
    for c, blk in scan_blocks(coef, geo):
        dc, ac = block_symbols(blk, pred[c])
        pred[c] = int(blk[0])
        t = 2 * min(c, 1)
        hist[t, dc] += 1
        np.add.at(hist[t + 1], ac, 1)
    return hist


def optimal_table(freq_in):
    """jchuff.c's jpeg_gen_optimal_table: 256 frequencies -> (counts per length 1 .. 16, symbols)."""
    freq = [int(f) for f in freq_in] + [1]                 # 256: a reserved code point, so that no code is all ones
    codesize, others = [0] * 257, [-1] * 257

    def smallest(skip):
        best, v = -1, None
        for i in range(257):                               # ties go to the larger index
            if freq[i] and i != skip and (v is None or freq[i] <= v):
                best, v = i, freq[i]
        return best
    while True:
        c1 = smallest(-1)
        c2 = smallest(c1)
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        codesize[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            codesize[c1] += 1
        others[c1] = c2
        codesize[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            codesize[c2] += 1
    bits = [0] * 33
    for s in codesize:
        if s:
            assert s <= 32, "a code longer than 32 bits"
            bits[s] += 1
    for i in range(32, 16, -1):
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while i > 0 and bits[i] == 0:
        i -= 1
    if i:
        bits[i] -= 1                                       # the reserved code leaves
    symbols = [j for length in range(1, 33) for j in range(256) if codesize[j] == length]
    return bits[1:17], symbols


def optimal_tables(coef, geo):
    """The image's four (two for gray) tables (counts, symbols) in DHT order."""
    hist = histogram(coef, geo)
    return [optimal_table(hist[t]) for t in range(4 if geo["ncomp"] == 3 else 2)]


def header(geo, qtab, tables) -> bytes:
    """tests/jpeg_enc_ref.py ``header`` with the DHT segments of ``tables``."""
    std = E.header(geo, qtab)
    first, sos = std.index(b"\xff\xc4"), std.index(b"\xff\xda")
    assert first > 0 and sos > first
    return std[:first] + b"".join(E._dht(i, t) for i, t in zip((0x00, 0x10, 0x01, 0x11), tables)) + std[sos:]


def entropy_encode(coef, geo, qtab, tables) -> bytes:
    """tests/jpeg_enc_ref.py ``entropy_encode`` under ``tables`` [(counts, symbols)] in DHT order."""
    books = [E._codes(t) for t in tables]
    bw, pred = E._BitWriter(), [0] * geo["ncomp"]
    for c, blk in scan_blocks(coef, geo):
        t = 2 * min(c, 1)
        E._block(bw, blk, pred[c], books[t], books[t + 1])
        pred[c] = int(blk[0])
    bw.flush()
    tabs = [qtab[0]] + ([qtab[1]] if geo["ncomp"] == 3 else [])
    return header(geo, tabs, tables) + bytes(bw.out) + b"\xff\xd9"


def encode_optimized(coef, geo, qtab) -> bytes:
    return entropy_encode(coef, geo, qtab, optimal_tables(coef, geo))


def dht_tables(data: bytes):
    """The (counts, symbols) of a stream's DHT segments, in the order they stand there."""
    out, at = [], 2
    while data[at + 1] != 0xDA:
        size = int.from_bytes(data[at + 2:at + 4], "big")
        if data[at + 1] == 0xC4:
            body, k = data[at + 4:at + 2 + size], 0
            while k < len(body):
                counts = list(body[k + 1:k + 17])
                out.append((counts, list(body[k + 17:k + 17 + sum(counts)])))
                k += 17 + sum(counts)
        at += 2 + size
    return out


def packed_tables(tables):
    """-> (counts uint8 [4, 16], symbols uint8 [4, 256]): the two plain arrays the C ABI takes."""
    counts, symbols = np.zeros((4, 16), dtype=np.uint8), np.zeros((4, 256), dtype=np.uint8)
    for t, (c, s) in enumerate(tables):
        counts[t], symbols[t, :len(s)] = c, s
    return counts, symbols


# ---- the length-limit case: 17 distinct gray blocks laid out over 2048 x 2048
def limit_blocks() -> np.ndarray:
    """uint8 [17, 8, 8]: block i < 16 has one AC term, at zigzag position i + 1, equal to that position's quantiser step at quality
    50 (a quantised 1); block 16 is flat.  Samples: the float inverse DCT of that one term around 128, rounded."""
    q = E.quant_tables(LIMIT_QUALITY)[0].astype(np.float64)
    n = np.arange(8)
    basis = np.cos((2 * n[:, None] + 1) * n[None, :] * np.pi / 16) * np.where(n == 0, np.sqrt(0.5), 1.0)[None, :] / 2   # [x, u]
    out = np.full((17, 8, 8), 128, dtype=np.uint8)
    for i in range(16):
        nat = int(ZIGZAG[i + 1])
        v, u = divmod(nat, 8)
        out[i] = np.clip(np.rint(128 + q[nat] * np.outer(basis[:, v], basis[:, u])), 0, 255).astype(np.uint8)
    return out


def limit_order() -> np.ndarray:
    """uint8 [256 * 256]: which block stands where (row-major over the block grid): the flat one, then block i 2^i times."""
    return np.concatenate([[16]] + [np.full(1 << i, i) for i in range(16)]).astype(np.uint8)


def limit_image(blocks, order) -> np.ndarray:
    side = LIMIT_SIDE // 8
    return np.ascontiguousarray(blocks[order].reshape(side, side, 8, 8).transpose(0, 2, 1, 3).reshape(LIMIT_SIDE, LIMIT_SIDE))


def limit_coefficients(order) -> np.ndarray:
    """int16 [65536 * 64], the library's layout: what the forward DCT and the quantiser give for ``limit_image`` (the fixture's
    writer asserts it)."""
    side = LIMIT_SIDE // 8
    coef = np.zeros((17, 64), dtype=np.int16)
    for i in range(16):
        coef[i, ZIGZAG[i + 1]] = 1
    return coef[order].reshape(side * side * 64)


def load_fixture():
    """tests/golden/g25_jpeg_optimize.npz -> ({case name of g24: Pillow's optimize=True bytes}, dict(blocks, order, data) of the
    length-limit case)."""
    z = np.load(FIXTURE)
    data, off = z["data"], z["data_off"]
    streams = {name: data[off[i]:off[i + 1]].tobytes() for i, (name, _, _, _) in enumerate(E.case_list())}
    return streams, dict(blocks=z["limit_blocks"], order=z["limit_order"], data=z["limit_data"].tobytes())
