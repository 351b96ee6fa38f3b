"""Pure-Python restatement of the device entropy decoder's rounds (csrc/jpeg_sync.h, csrc/jpeg_huff_dec.hip, include/
vunet_jpeg_huffdec.h): the marker scan into segments, the subsequences, the walk from a parser state (bit position in the STUFFED
bytes, block index within the MCU, zigzag index k) to the state at the first symbol boundary at or behind the subsequence's end,
Jacobi rounds until no exit state changes, the block ordinals, the write pass and the DC sums.  One "thread" per subsequence and
every thread its own workgroup, so the bound on the rounds is the subsequence count of the longest segment + 1.  Shared by
tests/test_jpeg_sync_ref.py, tests/test_jpeg_sync_host.py and tests/test_hip_jpeg_huff_dec.py, whose input streams are built here.
Slow by design; equal walks are remembered (a walk depends on the bytes it can see and on its entry state alone)."""
from __future__ import annotations

import ctypes
import os
import re

import numpy as np

import jpeg_enc_ref as E
import jpeg_ref as R

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "vunet_jpeg_huffdec.h")
SUBSEQ_BYTES = int(re.search(r"#define VUNET_JPEG_SUBSEQ_BYTES (\d+)", open(HEADER).read()).group(1))
NEVER_RGB = (200, 30, 90)
DONE, STOP, LOST, RANGE = 0, 1, 2, 3


def segments(data: bytes, hdr: dict):
    """[(byte begin, byte end, first MCU)] of the entropy-coded data, or None: irregular (a marker out of sequence, fill bytes, an FF
    at the end of the data, no EOI, a segment count that does not match the restart interval, an empty segment)."""
    d, p, ri = data, hdr["scan"], hdr["restart"]
    mcus = hdr["mcu_cols"] * hdr["mcu_rows"]
    expected = -(-mcus // ri) if ri else 1
    begin, segs = p, []
    while True:
        p = d.find(b"\xff", p)
        if p < 0 or p + 1 >= len(d):
            return None
        m = d[p + 1]
        if m == 0:
            p += 2
            continue
        rst = 0xD0 <= m <= 0xD7
        if (not rst and m != 0xD9) or p == begin or len(segs) >= expected:
            return None
        if rst and (ri == 0 or m != 0xD0 + (len(segs) & 7)):
            return None
        segs.append((begin, p, len(segs) * ri))
        if not rst:
            break
        begin = p = p + 2
    return segs if len(segs) == expected else None


def subsequences(segs, sub: int):
    """One row per subsequence: dict(seg (index), begin, end, first, last)."""
    rows = []
    for s, (b, e, _) in enumerate(segs):
        n = -(-(e - b) // sub)
        for i in range(n):
            rows.append(dict(seg=s, begin=b + i * sub, end=e if i + 1 == n else b + (i + 1) * sub, first=i == 0, last=i + 1 == n))
    return rows


class _Segment:
    """The unstuffed bits of one segment and the stuffed position of each (the 00 behind an FF belongs to the FF)."""

    def __init__(self, d: bytes, begin: int, end: int):
        raw = np.frombuffer(d, dtype=np.uint8, count=end - begin, offset=begin)
        keep = np.ones(raw.size, dtype=bool)
        keep[1:] = ~((raw[1:] == 0) & (raw[:-1] == 0xFF))
        idx = np.flatnonzero(keep)
        self.bits = np.unpackbits(raw[idx]).tolist()
        self.pos = ((begin + idx)[:, None] * 8 + np.arange(8)[None, :]).reshape(-1)
        self.begin, self.end = begin, end

    def index(self, pos: int) -> int:
        return int(np.searchsorted(self.pos, pos))                      # (a position on a stuffed byte moves behind it)

    def at(self, i: int) -> int:
        return int(self.pos[i]) if i < len(self.bits) else self.end * 8


class Decoder:
    def __init__(self, data: bytes, sub: int = SUBSEQ_BYTES):
        self.d, self.sub, self.hdr = bytes(data), sub, R.parse(data)
        h = self.hdr
        self.hv = h["hsamp"] * h["vsamp"] if h["ncomp"] == 3 else 1
        self.per_mcu = self.hv + 2 if h["ncomp"] == 3 else 1
        self.books = [(R._codebook(h["dc"][c]), R._codebook(h["ac"][c])) for c in range(h["ncomp"])]
        self.segs = segments(self.d, h)
        self.rows = subsequences(self.segs, sub) if self.segs else []
        self.bits = [_Segment(self.d, b, e) for b, e, _ in self.segs] if self.segs else []
        self.memo, self.rounds, self.walks = {}, 0, []

    def _symbol(self, bits, i, book):
        """-> (symbol, next index); symbol None: no such code, -1: the segment's bits ran out."""
        code = 0
        for length in range(1, 17):
            if i >= len(bits):
                return -1, i
            code = (code << 1) | bits[i]
            i += 1
            s = book.get((length, code))
            if s is not None:
                return s, i
        return None, i

    def walk(self, row, state, write=None, trace=None):
        """``state`` = (pos, blk, k) -> (exit state, blocks begun, status).  ``write``: (ordinal of the next block to begin, lo, hi,
        store(ordinal, k, value)): blocks with lo <= ordinal < hi are stored, the DC difference at k = 0; others end the walk.
        ``trace``: a list that takes the position of every block begun."""
        seg, end_bit = self.bits[row["seg"]], row["end"] * 8
        key = None
        if write is None and trace is None:
            lo = max(state[0] // 8 - 1, seg.begin)
            key = (self.d[lo:min(row["end"] + 8, seg.end)], state[0] - 8 * lo, end_bit - 8 * lo, state[1], state[2],
                   max(row["end"] + 8 - seg.end, 0))
            hit = self.memo.get(key)
            if hit is not None:
                (dp, blk, k), begun, status = hit
                return (dp + 8 * lo, blk, k), begun, status
        pos, blk, k = state
        bits, i, begun, status = seg.bits, seg.index(pos), 0, DONE
        ordinal = write[0] if write else 0
        if write and k != 0 and not write[1] <= ordinal - 1 < write[2]:
            return state, 0, RANGE
        while pos < end_bit:
            c = 0 if blk < self.hv else blk - self.hv + 1
            if k == 0:
                s, j = self._symbol(bits, i, self.books[c][0])
                if s is None or (s != -1 and s > 15):
                    status = LOST
                    break
                if s == -1 or j + s > len(bits):
                    status = STOP
                    break
                v = R._extend(int("".join(map(str, bits[j:j + s])) or "0", 2), s)
                if trace is not None:
                    trace.append(pos)
                if write:
                    if not write[1] <= ordinal < write[2]:
                        status = RANGE
                        break
                    write[3](ordinal, 0, v)
                ordinal, begun, k, i = ordinal + 1, begun + 1, 1, j + s
            else:
                rs, j = self._symbol(bits, i, self.books[c][1])
                if rs is None:
                    status = LOST
                    break
                if rs == -1:
                    status = STOP
                    break
                r, s = rs >> 4, rs & 15
                if s == 0:
                    k = k + 16 if r == 15 else 64
                else:
                    if j + s > len(bits):
                        status = STOP
                        break
                    if k + r > 63:
                        status = LOST
                        break
                    v = R._extend(int("".join(map(str, bits[j:j + s])), 2), s)
                    if write:
                        write[3](ordinal - 1, k + r, v)
                    k, j = k + r + 1, j + s
                i = j
                if k >= 64:
                    k, blk = 0, (blk + 1) % self.per_mcu
            pos = seg.at(i)
        out = ((end_bit, 0, 0) if status == LOST else (pos, blk, k)), begun, status
        if key is not None:
            lo = max(state[0] // 8 - 1, seg.begin)
            self.memo[key] = ((out[0][0] - 8 * lo, out[0][1], out[0][2]), begun, status)
        return out

    def entry(self, i, exits):
        row = self.rows[i]
        return (row["begin"] * 8, 0, 0) if row["first"] else exits[i - 1]

    def synchronise(self):
        """Jacobi rounds from the guess "every subsequence begins a block at its first bit" -> (exit states, blocks begun); sets
        ``rounds`` (the first round in which nothing changed included) and ``walks`` (subsequences walked per round)."""
        n = len(self.rows)
        exits, walked, begun = [(r["end"] * 8, 0, 0) for r in self.rows], [None] * n, [0] * n
        self.rounds, self.walks = 0, []
        bound = max(sum(1 for r in self.rows if r["seg"] == s) for s in range(len(self.segs))) + 1
        while True:
            self.rounds += 1
            new, moved, count = list(exits), 0, 0
            for i in range(n):
                e = self.entry(i, exits)
                if e == walked[i]:
                    continue
                new[i], begun[i], _ = self.walk(self.rows[i], e)
                walked[i], count = e, count + 1
                moved += new[i] != exits[i]
            exits = new
            self.walks.append(count)
            if moved == 0:
                return exits, begun
            assert self.rounds <= bound, (self.rounds, bound)

    def decode(self):
        """-> the coefficients in the library's layout (int16 [ncoef]), or None: irregular, or flagged (SHORT / ERROR)."""
        if not self.segs:
            return None
        h = self.hdr
        exits, begun = self.synchronise()
        nblocks = h["ncoef"] // 64
        mcus = h["mcu_cols"] * h["mcu_rows"]
        coef = [np.zeros((bh, bw, 64), dtype=np.int64) for bh, bw in h["blocks"]]

        def place(ordinal):
            m, r = divmod(ordinal, self.per_mcu)
            my, mx = divmod(m, h["mcu_cols"])
            if r < self.hv:
                return 0, my * h["vsamp"] + r // h["hsamp"], mx * h["hsamp"] + r % h["hsamp"]
            return r - self.hv + 1, my, mx

        def store(ordinal, k, v):
            c, y, x = place(ordinal)
            coef[c][y, x, R.ZIGZAG[k]] = v
        ok, in_seg = True, 0
        for i, row in enumerate(self.rows):
            b, e, mcu0 = self.segs[row["seg"]]
            tail = row["seg"] + 1 == len(self.segs)
            seg_blocks = (min(h["restart"], mcus - mcu0) if h["restart"] else mcus) * self.per_mcu
            lo = mcu0 * self.per_mcu
            if row["first"]:
                in_seg = 0
            state, _, status = self.walk(row, self.entry(i, exits), (lo + in_seg, lo, min(lo + seg_blocks, nblocks), store))
            in_seg += begun[i]
            if status == LOST or (status == STOP and state[2] != 0) or (status == RANGE and not tail):
                ok = False
            if row["last"]:
                left = len(self.bits[row["seg"]].bits) - self.bits[row["seg"]].index(state[0])
                if (in_seg < seg_blocks if tail else in_seg != seg_blocks) or (not tail and left >= 8):
                    ok = False
                if status != RANGE and state[2] != 0:
                    ok = False
        if not ok:
            return None
        pred = [0] * h["ncomp"]
        for o in range(nblocks):
            if h["restart"] and o % (h["restart"] * self.per_mcu) == 0:
                pred = [0] * h["ncomp"]
            c, y, x = place(o)
            pred[c] += int(coef[c][y, x, 0])
            coef[c][y, x, 0] = pred[c]
        return np.concatenate([c.reshape(-1) for c in coef]).astype(np.int16)

    def block_spans(self, longer_than: int = 0):
        """[(segment begin, first byte, last byte)] of every block of the true parse of the segments longer than ``longer_than``."""
        spans = []
        for s, (b, e, _) in enumerate(self.segs):
            if e - b <= longer_than:
                continue
            starts = []
            state, _, _ = self.walk(dict(seg=s, begin=b, end=e, first=True, last=True), (b * 8, 0, 0), trace=starts)
            spans += [(b, a // 8, max(a, z - 1) // 8) for a, z in zip(starts, starts[1:] + [state[0]])]
        return spans


# ---- the streams of the GPU tests
def noise_ramp(h, w, seed):
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([(xx * 255) // max(w - 1, 1), (yy * 255) // max(h - 1, 1), ((xx + yy) * 255) // max(h + w - 2, 1)], axis=2)
    return np.clip(img + g.integers(-24, 25, size=(h, w, 3)), 0, 255).astype(np.uint8)


def gpu_streams(encode):
    """The streams of the GPU file's test 3.  ``encode(frames uint8 [N, H, W, 3], quality=, subsampling=) -> list of bytes``."""
    square = np.stack([noise_ramp(256, 256, 256)] * 3)
    strip = np.random.default_rng(1100).integers(0, 256, size=(1, 9, 1100, 3), dtype=np.uint8)
    return (encode(square, quality=75, subsampling=list(E.SAMPLING)) + encode(strip, quality=95, subsampling="4:2:0") +
            encode(noise_ramp(1002, 1000, 1002)[None], quality=95, subsampling="4:2:0"))


def _lib():
    from behavior_driven_video_synthesis_amd import _lib as L
    return L


def host_encode(coef, h, w, qtab) -> bytes:
    """The library's host coder (no GPU): flat coefficients of an h x w frame at 4:2:0 and qtab [3, 64] -> the stream."""
    L = _lib()
    info = L.struct("vunet_jpeg_info")()
    assert L.lib().vunet_jpeg_encode_info(h, w, 3, 2, 2, ctypes.byref(info)) == 0 and info.ncoef == coef.size
    out, length = np.zeros(4096 + 8 * coef.size, dtype=np.uint8), ctypes.c_int64(0)   # (a term takes at most 26 bits, stuffed)
    coef, qtab = np.ascontiguousarray(coef, dtype=np.int16), np.ascontiguousarray(qtab, dtype=np.uint16)
    assert L.lib().vunet_jpeg_entropy_encode(coef.ctypes.data, ctypes.byref(info), qtab.ctypes.data, out.ctypes.data, out.size,
                                             ctypes.byref(length)) == 0
    return out[:length.value].tobytes()


def stuffed_stream() -> bytes:
    """24 x 24 at 4:2:0, 1023 in every AC position: the hand-made set 5 of tests/test_hip_jpeg_entropy.py's test 4."""
    coef = np.zeros((24, 64), dtype=np.int16)
    coef[:, 1:] = 1023
    return host_encode(coef.reshape(-1), 24, 24, E.quant_tables(75)[[0, 1, 1]])


def never_stream(side: int = 1536) -> bytes:
    """A constant NEVER_RGB frame at quality 75, 4:2:0: every MCU after the first is the same 32 bits."""
    img = np.empty((side, side, 3), dtype=np.uint8)
    img[:] = NEVER_RGB
    coef, qtab, _ = E.image_coefficients(img, 75, "4:2:0")
    return host_encode(E.flat_coef(coef), side, side, qtab)


def flipped(data: bytes, count: int, seed: int = 2024):
    """``count`` copies of ``data`` with one seeded bit inside the scan flipped each."""
    scan, g, out = R.parse(data)["scan"], np.random.default_rng(seed), []
    for _ in range(count):
        d = bytearray(data)
        d[int(g.integers(scan, len(data) - 2))] ^= 1 << int(g.integers(0, 8))
        out.append(bytes(d))
    return out


def three_tables(data: bytes) -> bytes:
    """A three-component stream rewritten to use THREE DC tables: the third component's table again under id 2, and that component
    pointed at it.  Baseline, and the same image -- but more than the device's two DC slots, so the marker scan calls it irregular."""
    hdr = R.parse(data)
    assert hdr["ncomp"] == 3
    sos = hdr["scan"] - 14                                             # FF DA, length 12, 3 x (id, tables), Ss, Se, Ah/Al
    assert data[sos:sos + 4] == b"\xff\xda\x00\x0c"
    counts, symbols = hdr["dc"][2]
    body = bytes([0x02]) + bytes(counts) + bytes(symbols)
    dht = b"\xff\xc4" + (len(body) + 2).to_bytes(2, "big") + body
    tail = bytearray(data[sos:])
    tail[10] = 0x20 | (tail[10] & 0x0F)                                # the third component: Td = 2, Ta as it was
    return data[:sos] + dht + bytes(tail)


def coverage(streams, sub: int = SUBSEQ_BYTES) -> dict:
    """What the streams make the walk meet at subsequence size ``sub``: a stuffed 00 that is the first byte of a subsequence, an FF
    that is the last byte of one, a block that straddles three subsequences, a segment shorter than one subsequence."""
    out = dict(stuffed_first=0, ff_last=0, three=0, short_segment=0)
    for data in streams:
        dec = Decoder(data, sub)
        if not dec.segs:
            continue
        d = dec.d
        for row in dec.rows:
            out["stuffed_first"] += not row["first"] and d[row["begin"]] == 0 and d[row["begin"] - 1] == 0xFF
            out["ff_last"] += not row["last"] and d[row["end"] - 1] == 0xFF
        out["short_segment"] += sum(e - b < sub for b, e, _ in dec.segs)
        out["three"] += sum((z - b) // sub - (a - b) // sub >= 2 for b, a, z in dec.block_spans(2 * sub))
    return out
