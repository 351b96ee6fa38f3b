"""Optimised Huffman tables without a GPU: the restatement (tests/jpeg_opt_ref.py) and the library's host functions
(csrc/jpeg_huff_enc.h through the C ABI: ``vunet_jpeg_symbol_histogram``, ``vunet_jpeg_optimal_table``,
``vunet_jpeg_entropy_encode_tables``, ``vunet_jpeg_write_header``, ``vunet_jpeg_code_words``) against Pillow's ``optimize=True``
bytes (tests/golden/g25_jpeg_optimize.npz), the length-limit case included; ``encode_batch(optimize=True)`` with the device step
replaced by the restatement as tests/test_jpeg_enc_host.py replaces it; and the stand-alone checker under the host sanitizers.
Everything is exact."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import jpeg_enc_ref as E
import jpeg_opt_ref as O

GUARD = 64
SENTINEL = 0xA5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from behavior_driven_video_synthesis_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def cases():
    """g24's cases with Pillow's optimised bytes as ``opt`` and the geometry as ``geo``; plus ``limit``, the length-limit case in
    the same form (its coefficients are what the fixture's writer asserted)."""
    plain, (streams, limit) = E.load_fixture(), O.load_fixture()
    assert list(plain) == list(streams)
    for name, c in plain.items():
        c["opt"] = streams[name]
        c["geo"] = E.geometry(*c["img"].shape[:2], 1 if c["img"].ndim == 2 else 3, *E.SAMPLING[c["subsampling"]])
    assert np.array_equal(limit["blocks"], O.limit_blocks()) and np.array_equal(limit["order"], O.limit_order())
    plain["limit"] = dict(img=O.limit_image(limit["blocks"], limit["order"]), quality=O.LIMIT_QUALITY, subsampling="4:4:4",
                          opt=limit["data"], coef=O.limit_coefficients(limit["order"]), qtab=E.quant_tables(O.LIMIT_QUALITY)[:1],
                          geo=E.geometry(O.LIMIT_SIDE, O.LIMIT_SIDE, 1, 1, 1))
    return plain


def _info(lib, c):
    from behavior_driven_video_synthesis_amd import _lib
    info, g = _lib.struct("vunet_jpeg_info")(), c["geo"]
    assert lib.vunet_jpeg_encode_info(g["height"], g["width"], g["ncomp"], g["hsamp"], g["vsamp"], ctypes.byref(info)) == 0
    return info


def _histogram(lib, c):
    coef, hist = np.ascontiguousarray(c["coef"], dtype=np.int16), np.full((4, 256), 77, dtype=np.uint32)
    assert lib.vunet_jpeg_symbol_histogram(coef.ctypes.data, ctypes.byref(_info(lib, c)), hist.ctypes.data) == 0
    return hist


def _tables(lib, hist, ntab):
    """-> (counts [4, 16], symbols [4, 256], [(counts, symbols)] as lists); sentinels behind both arrays of every call."""
    counts, symbols, out = np.zeros((4, 16), dtype=np.uint8), np.zeros((4, 256), dtype=np.uint8), []
    for t in range(ntab):
        c, s, n = np.full(16 + GUARD, SENTINEL, dtype=np.uint8), np.full(256 + GUARD, SENTINEL, dtype=np.uint8), ctypes.c_int32(-1)
        freq = np.ascontiguousarray(hist[t])
        assert lib.vunet_jpeg_optimal_table(freq.ctypes.data, c.ctypes.data, s.ctypes.data, ctypes.byref(n)) == 0
        assert (c[16:] == SENTINEL).all() and (s[n.value:] == SENTINEL).all() and n.value == int(c[:16].sum())
        counts[t], symbols[t, :n.value] = c[:16], s[:n.value]
        out.append((c[:16].tolist(), s[:n.value].tolist()))
    return counts, symbols, out


def _encode(lib, c, counts, symbols, cap, fn="vunet_jpeg_entropy_encode_tables"):
    """-> (return code, announced length, the ``cap`` bytes); asserts that the sentinel bytes behind ``cap`` are untouched."""
    coef, qtab = np.ascontiguousarray(c["coef"], dtype=np.int16), np.ascontiguousarray(c["qtab"], dtype=np.uint16)
    out, length = np.full(cap + GUARD, SENTINEL, dtype=np.uint8), ctypes.c_int64(-1)
    args = (None, None) if counts is None else (counts.ctypes.data, symbols.ctypes.data)
    lead = (coef.ctypes.data,) if fn == "vunet_jpeg_entropy_encode_tables" else ()
    rc = getattr(lib, fn)(*lead, ctypes.byref(_info(lib, c)), qtab.ctypes.data, *args, out.ctypes.data, cap, ctypes.byref(length))
    assert (out[cap:] == SENTINEL).all()
    return rc, length.value, out[:cap]


def _head(data: bytes) -> int:
    """The length of SOI .. SOS: the segments are walked, not searched for."""
    at = 2
    while True:
        assert data[at] == 0xFF
        size = int.from_bytes(data[at + 2:at + 4], "big")
        if data[at + 1] == 0xDA:
            return at + 2 + size
        at += 2 + size


def test_the_restatement_writes_pillows_optimised_bytes(cases):
    smaller = 0
    for name, c in cases.items():
        coef = E.split_coef(c["coef"], c["geo"])
        assert O.encode_optimized(coef, c["geo"], c["qtab"]) == c["opt"], name
        assert O.dht_tables(c["opt"]) == O.optimal_tables(coef, c["geo"]), name
        if "data" in c:
            assert len(c["opt"]) <= len(c["data"]), name
            smaller += len(c["opt"]) < len(c["data"])
    assert smaller > 300
    assert O.dht_tables(cases["limit"]["opt"])[1][0] == O.LIMIT_AC_COUNTS        # the 16-bit limiter has acted on this one


def test_the_librarys_histogram_is_the_restatements(lib, cases):
    for name, c in cases.items():
        want = O.histogram(E.split_coef(c["coef"], c["geo"]), c["geo"])
        assert np.array_equal(_histogram(lib, c), want), name
        assert int(want[0].sum() + want[2].sum()) == len(c["coef"]) // 64         # one DC symbol per block


def test_the_librarys_tables_are_pillows_dht_segments(lib, cases):
    for name, c in cases.items():
        ntab = 4 if c["geo"]["ncomp"] == 3 else 2
        assert _tables(lib, _histogram(lib, c), ntab)[2] == O.dht_tables(c["opt"]), name


def test_the_writer_with_those_tables_gives_pillows_bytes_and_null_tables_give_annex_ks(lib, cases):
    for name, c in cases.items():
        counts, symbols, _ = _tables(lib, _histogram(lib, c), 4 if c["geo"]["ncomp"] == 3 else 2)
        rc, n, out = _encode(lib, c, counts, symbols, len(c["opt"]))
        assert rc == 0 and n == len(c["opt"]) and out.tobytes() == c["opt"], (name, rc, n)
        head = _head(c["opt"])
        rc, n, out = _encode(lib, c, counts, symbols, head, fn="vunet_jpeg_write_header")
        assert rc == 0 and n == head and out.tobytes() == c["opt"][:head], name     # SOI .. SOS alone
        if "data" in c:
            rc, n, out = _encode(lib, c, None, None, len(c["data"]))
            assert rc == 0 and n == len(c["data"]) and out.tobytes() == c["data"], name
            rc, n, out = _encode(lib, c, None, None, head + 1000, fn="vunet_jpeg_write_header")
            assert rc == 0 and n == _head(c["data"]) and out[:n].tobytes() == c["data"][:n], name


def test_every_short_capacity_is_refused_and_nothing_is_written_behind_it(lib, cases):
    from behavior_driven_video_synthesis_amd import _lib
    code = _lib.const("VUNET_JPEG_ERR_CAPACITY")
    small = ("1x1_noise_q75_s420", "8x8_sat_q100_s420", "gray_17x23_noise_q75", "8x8_ramp_q30_s444")
    for name, c in cases.items():
        if name == "limit":
            continue
        counts, symbols, _ = _tables(lib, _histogram(lib, c), 4 if c["geo"]["ncomp"] == 3 else 2)
        n = len(c["opt"])
        for cap in (range(n) if name in small else (n - 1,)):
            rc, need, out = _encode(lib, c, counts, symbols, cap)
            assert rc == code and need == n and out.tobytes() == c["opt"][:cap], (name, cap, rc, need)
        if name in small:
            for cap in range(0, _head(c["opt"]), 7):
                rc, need, out = _encode(lib, c, counts, symbols, cap, fn="vunet_jpeg_write_header")
                assert rc == code and need == _head(c["opt"]) and out.tobytes() == c["opt"][:cap], (name, cap)


def test_tables_that_are_no_code_or_lack_a_symbol_are_refused(lib, cases):
    from behavior_driven_video_synthesis_amd import _lib
    arg, c = _lib.const("VUNET_ERR_ARG"), cases["16x16_noise_q75_s420"]
    counts, symbols, _ = _tables(lib, _histogram(lib, c), 4)
    cap = len(c["opt"])
    assert _encode(lib, c, counts, symbols, cap)[0] == 0
    for t in range(4):                                       # the longest code of each table leaves: a symbol the image needs
        bad = counts.copy()
        bad[t, np.flatnonzero(bad[t])[-1]] -= 1
        assert _encode(lib, c, bad, symbols, cap)[:2] == (arg, 0), t
    bad = counts.copy()
    bad[1, 0] = 3                                            # three codes of one bit
    assert _encode(lib, c, bad, symbols, cap)[0] == arg and _encode(lib, c, bad, symbols, cap, fn="vunet_jpeg_write_header")[0] == arg
    twice = symbols.copy()
    twice[3, 1] = twice[3, 0]
    assert _encode(lib, c, counts, twice, cap)[0] == arg
    coef, qtab, out, n = np.ascontiguousarray(c["coef"]), np.ascontiguousarray(c["qtab"]), np.zeros(cap, dtype=np.uint8), ctypes.c_int64(0)
    assert lib.vunet_jpeg_entropy_encode_tables(coef.ctypes.data, ctypes.byref(_info(lib, c)), qtab.ctypes.data, counts.ctypes.data, None,
                                                out.ctypes.data, cap, ctypes.byref(n)) == arg
    # the device coder's form of the tables: length << 16 | code per symbol, what the restatement's code book says
    codes = np.full((4, 256), 7, dtype=np.uint32)
    assert lib.vunet_jpeg_code_words(counts.ctypes.data, symbols.ctypes.data, codes.ctypes.data) == 0
    for t, table in enumerate(O.dht_tables(c["opt"])):
        book = E._codes(table)
        assert {s: (int(w) & 0xFFFF, int(w) >> 16) for s, w in enumerate(codes[t]) if w} == book, t
    assert lib.vunet_jpeg_code_words(None, None, codes.ctypes.data) == 0
    for t, table in enumerate((E.DC_LUMA, E.AC_LUMA, E.DC_CHROMA, E.AC_CHROMA)):
        assert {s: (int(w) & 0xFFFF, int(w) >> 16) for s, w in enumerate(codes[t]) if w} == E._codes(table), t
    assert lib.vunet_jpeg_code_words(bad.ctypes.data, symbols.ctypes.data, codes.ctypes.data) == arg
    # the batch form: three images' histograms at once, the gray one among them building two tables only when asked for two
    batch = [cases[n] for n in ("16x16_noise_q75_s420", "64x64_sat_q100_s444", "8x8_ramp_q30_s422")]
    hist = np.stack([_histogram(lib, b) for b in batch])
    c3, s3, w3, failed = np.full((3, 4, 16), 9, dtype=np.uint8), np.full((3, 4, 256), 9, dtype=np.uint8), np.zeros((3, 4, 256), dtype=np.uint32), \
        ctypes.c_int32(5)
    assert lib.vunet_jpeg_optimal_tables(hist.ctypes.data, 3, 4, c3.ctypes.data, s3.ctypes.data, w3.ctypes.data, ctypes.byref(failed)) == 0
    assert failed.value == -1
    for j, b in enumerate(batch):
        cj, sj, _ = _tables(lib, hist[j], 4)
        assert np.array_equal(c3[j], cj) and np.array_equal(s3[j], sj), j
        assert lib.vunet_jpeg_code_words(cj.ctypes.data, sj.ctypes.data, codes.ctypes.data) == 0 and np.array_equal(w3[j], codes), j
    hist[1, 1, :] = np.arange(256, dtype=np.uint64) ** 4 % (1 << 32)      # still fine: no code passes 32 bits
    hist[2, 1, :] = 0
    hist[2, 1, :2] = [1, 2]                                                 # 1, 2, 3, 5, 8, ..: a chain of 45 symbols, 45 bits
    for k in range(2, 45):
        hist[2, 1, k] = hist[2, 1, k - 1] + hist[2, 1, k - 2]
    assert lib.vunet_jpeg_optimal_tables(hist.ctypes.data, 3, 4, c3.ctypes.data, s3.ctypes.data, w3.ctypes.data, ctypes.byref(failed)) == arg
    assert failed.value == 2
    # a coefficient out of range is the histogram's to refuse, as it is the coder's
    wrong = dict(c, coef=c["coef"].copy())
    wrong["coef"][5] = 1024
    hist = np.zeros((4, 256), dtype=np.uint32)
    assert lib.vunet_jpeg_symbol_histogram(np.ascontiguousarray(wrong["coef"]).ctypes.data, ctypes.byref(_info(lib, c)),
                                           hist.ctypes.data) == _lib.const("VUNET_JPEG_ERR_RANGE")


# ---- jpeg_encode.encode_batch(optimize=True) and video_io with the device step replaced by the restatement
@pytest.fixture
def stubbed(monkeypatch):
    from behavior_driven_video_synthesis_amd import jpeg_encode as J
    calls = []

    def launch(buf, frames, m, channels, up_bytes, q_off, q_count, coef_count):
        stage = buf.stage.numpy()
        rows = (J.JpegImg * m).from_buffer_copy(stage[:m * ctypes.sizeof(J.JpegImg)].tobytes())
        qtab, dst = stage[q_off:up_bytes].view(np.uint16), buf.coef_host.numpy()
        for r in rows:
            planes, geo = E.from_rgb(frames[r.slot, :r.height, :r.width].numpy(), r.hsamp, r.vsamp)
            flat = E.flat_coef(E.coefficients(planes, geo, qtab[r.q_off:r.q_off + 128].reshape(2, 64)))
            dst[r.coef_off:r.coef_off + len(flat)] = flat
        calls.append(m)
    monkeypatch.setattr(J, "_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(J, "_launch", launch)
    J.clear_buffers()
    yield J, calls
    J.clear_buffers()


def test_encode_batch_optimize_returns_pillows_bytes(stubbed, cases, tmp_path):
    from behavior_driven_video_synthesis_amd import video_io as V
    J, calls = stubbed
    names = [n for n in cases if n.endswith("_s422") and "ramp" not in n]          # every size, two contents, four qualities
    stack, sizes = torch.full((len(names), 250, 250, 3), 7, dtype=torch.uint8), []
    for i, n in enumerate(names):
        img = cases[n]["img"]
        stack[i, :img.shape[0], :img.shape[1]] = torch.from_numpy(img)
        sizes.append(img.shape[:2])
    quality = [cases[n]["quality"] for n in names]
    for threads in (1, 3):
        got = J.encode_batch(stack, quality=quality, subsampling="4:2:2", sizes=sizes, threads=threads, optimize=True)
        assert [type(g) for g in got] == [bytes] * len(names)
        for n, g in zip(names, got):
            assert g == cases[n]["opt"], n
    got = J.encode_batch(stack, quality=quality, subsampling="4:2:2", sizes=sizes)       # the default is what it was
    assert all(g == cases[n]["data"] for n, g in zip(names, got))
    c = cases["gray_37x45_ramp_q95"]
    assert J.encode_batch(torch.from_numpy(c["img"])[None], quality=95, optimize=True) == [c["opt"]]
    with pytest.raises(ValueError, match="entropy"):
        J.encode_batch(stack, entropy="gpu")
    # the keywords reach encode_batch through the file writers, and an optimised video reads back as it was written
    a, b = cases["16x16_noise_q75_s420"], cases["16x16_ramp_q75_s420"]
    clip = torch.stack([torch.from_numpy(a["img"]), torch.from_numpy(b["img"])])
    path = V.write_mjpeg(str(tmp_path / "clip.avi"), clip, optimize=True)
    assert V.read_mjpeg(path) == (12.0, [a["opt"], b["opt"]])
    paths = V.save_videos(str(tmp_path / "row_%d.avi"), torch.stack([clip, clip.flip(0)]), optimize=True)
    assert V.read_mjpeg(paths[1])[1] == [b["opt"], a["opt"]]
    imgs = J.save_images(str(tmp_path / "img_%02d.jpg"), clip, optimize=True)
    assert open(imgs[1], "rb").read() == b["opt"]


def test_a_range_error_names_the_lowest_frame_with_optimize_too(stubbed, cases, monkeypatch):
    J, calls = stubbed
    real = J._launch

    def launch(buf, *a):
        real(buf, *a)
        dst = buf.coef_host.numpy()
        dst[3 * 64 * 6 + 5] = dst[64 * 6 + 5] = 1024         # frames 1 and 3 of four 16 x 16 frames at 4:2:0 (6 blocks each)
    monkeypatch.setattr(J, "_launch", launch)
    img = torch.from_numpy(cases["16x16_noise_q75_s420"]["img"])
    with pytest.raises(J.JpegEncodeError) as e:
        J.encode_batch(torch.stack([img] * 4), optimize=True)
    assert (e.value.code, e.value.index) == (J.ERR_RANGE, 1)


def test_the_checker_runs_clean_under_the_host_sanitizers(tmp_path):
    """tools/jpeg_opt_host_check.cpp (its own ``main``; the library is not involved) built with -fsanitize=address,undefined."""
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "jpeg_opt_host_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "jpeg_opt_host_check.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "72 coefficient sets" in r.stdout
