"""The host half of the JPEG encoder without a GPU: ``vunet_jpeg_entropy_encode`` and its helpers (csrc/jpeg_huff_enc.h through the
library's C ABI) against the fixture's bytes (tests/golden/g24_jpeg_encode.npz, Pillow's) and the restatement
(tests/jpeg_enc_ref.py); the capacity limit and the range check; and ``video_io``'s AVI writer and reader, with the device step of
``jpeg_encode.encode_batch`` replaced by the restatement as tests/test_jpeg_host.py does for the decoder."""
import ctypes
import os
import struct

import numpy as np
import pytest
import torch

import jpeg_enc_ref as E

GUARD = 64
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def lib():
    from behavior_driven_video_synthesis_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def cases():
    return E.load_fixture()


def _info(lib, c):
    from behavior_driven_video_synthesis_amd import _lib
    info = _lib.struct("vunet_jpeg_info")()
    h, w = c["img"].shape[:2]
    hs, vs = E.SAMPLING[c["subsampling"]]
    assert lib.vunet_jpeg_encode_info(h, w, 1 if c["img"].ndim == 2 else 3, hs, vs, ctypes.byref(info)) == 0
    return info


def _encode(lib, coef, info, qtab, cap):
    """-> (return code, announced length, the ``cap`` bytes); asserts that the sentinel bytes behind ``cap`` are untouched."""
    coef, qtab = np.ascontiguousarray(coef, dtype=np.int16), np.ascontiguousarray(qtab, dtype=np.uint16)
    out = np.full(cap + GUARD, SENTINEL, dtype=np.uint8)
    length = ctypes.c_int64(-1)
    rc = lib.vunet_jpeg_entropy_encode(coef.ctypes.data, ctypes.byref(info), qtab.ctypes.data, out.ctypes.data, cap, ctypes.byref(length))
    assert (out[cap:] == SENTINEL).all()
    return rc, length.value, out[:cap]


def test_encode_info_equals_the_restatements_geometry(lib, cases):
    from behavior_driven_video_synthesis_amd import _lib
    for name, c in cases.items():
        info = _info(lib, c)
        g = E.geometry(*c["img"].shape[:2], info.ncomp, *E.SAMPLING[c["subsampling"]])
        assert (info.mcu_cols, info.mcu_rows, info.restart, info.ncoef) == (g["mcu_cols"], g["mcu_rows"], 0, g["ncoef"]), name
        assert (info.bh0, info.bw0) == g["blocks"][0] and (info.bh1, info.bw1) == (g["blocks"][1] if info.ncomp == 3 else (0, 0))
        assert info.ncoef == len(c["coef"]) and info.nblocks * 64 == info.ncoef
    info = _lib.struct("vunet_jpeg_info")()
    for bad in ((0, 8, 3, 1, 1), (8, 65536, 3, 1, 1), (8, 8, 2, 1, 1), (8, 8, 3, 1, 2), (8, 8, 1, 2, 2), (8, 8, 3, 4, 1)):
        assert lib.vunet_jpeg_encode_info(*bad, ctypes.byref(info)) == _lib.const("VUNET_ERR_ARG"), bad


def test_quant_tables_equal_the_fixtures_and_the_restatements(lib, cases):
    q = np.zeros((2, 64), dtype=np.uint16)
    for quality in (-3, 1, 10, 30, 49, 50, 51, 75, 95, 100, 400):
        assert lib.vunet_jpeg_quant_tables(quality, q.ctypes.data) == 0
        assert np.array_equal(q, E.quant_tables(quality)), quality
    for name in ("64x64_noise_q30_s420", "64x64_noise_q75_s420", "64x64_noise_q95_s420", "64x64_noise_q100_s420"):
        lib.vunet_jpeg_quant_tables(cases[name]["quality"], q.ctypes.data)
        assert np.array_equal(q[[0, 1, 1]], cases[name]["qtab"]), name


def test_entropy_encode_equals_pillows_bytes_and_decodes_back(lib, cases):
    from behavior_driven_video_synthesis_amd import _lib
    for name, c in cases.items():
        info = _info(lib, c)
        bound = ctypes.c_int64(0)
        assert lib.vunet_jpeg_encode_bound(ctypes.byref(info), ctypes.byref(bound)) == 0 and bound.value >= len(c["data"]), name
        rc, n, out = _encode(lib, c["coef"], info, c["qtab"], len(c["data"]))
        assert rc == 0 and n == len(c["data"]), (name, rc, n)
        assert out.tobytes() == c["data"], name
        # ... and the library's own decoder gives the coefficients and the tables back
        back = _lib.struct("vunet_jpeg_info")()
        assert lib.vunet_jpeg_parse(c["data"], n, ctypes.byref(back)) == 0
        assert all(getattr(back, f) == getattr(info, f) for f, _ in back._fields_), name
        coef, qtab = np.zeros(info.ncoef, dtype=np.int16), np.zeros(info.ncomp * 64, dtype=np.uint16)
        assert lib.vunet_jpeg_entropy_decode(out.tobytes(), n, ctypes.byref(back), coef.ctypes.data, qtab.ctypes.data) == 0
        assert np.array_equal(coef, c["coef"]) and np.array_equal(qtab.reshape(-1, 64), c["qtab"]), name


def test_every_short_capacity_is_refused_and_nothing_is_written_behind_it(lib, cases):
    """Every ``cap`` from 0 to len - 1 on the smallest cases, len - 1 on the rest: the capacity code, the length the stream needs,
    the stream's own bytes below ``cap`` and the sentinel behind it (``_encode`` checks)."""
    from behavior_driven_video_synthesis_amd import _lib
    code = _lib.const("VUNET_JPEG_ERR_CAPACITY")
    assert code < 0 and code not in range(-119, -99)
    small = ("1x1_noise_q75_s420", "8x8_sat_q100_s420", "gray_17x23_noise_q75", "8x8_ramp_q30_s444")
    for name, c in cases.items():
        info, n = _info(lib, c), len(c["data"])
        for cap in (range(n) if name in small else (n - 1,)):
            rc, need, out = _encode(lib, c["coef"], info, c["qtab"], cap)
            assert rc == code and need == n, (name, cap, rc, need)
            assert out.tobytes() == c["data"][:cap], (name, cap)


def test_out_of_range_coefficients_and_bad_arguments_are_refused(lib, cases):
    from behavior_driven_video_synthesis_amd import _lib
    arg, rng = _lib.const("VUNET_ERR_ARG"), _lib.const("VUNET_JPEG_ERR_RANGE")
    c = cases["16x16_noise_q75_s420"]
    info, n = _info(lib, c), len(c["data"])
    for at, v, want in ((5, 1024, rng), (5, -1024, rng), (5, 1023, 0), (5, -1023, 0), (64 * 3 + 1, 1024, rng), (0, 2047, 0), (0, 2048, rng),
                        (64, -2048, rng)):
        coef = c["coef"].copy()
        if at % 64 == 0:
            coef[0::64][:4] = 0                     # (the DC difference is what counts: against zero neighbours)
        coef[at] = v
        rc, need, _ = _encode(lib, coef, info, c["qtab"], 4 * n)
        assert rc == want and (need > 0) == (want == 0), (at, v, rc)
    q = c["qtab"].copy()
    q[0, 3] = 256
    assert _encode(lib, c["coef"], info, q, n)[0] == arg
    q = c["qtab"].copy()
    q[2, 7] += 1
    assert _encode(lib, c["coef"], info, q, n)[0] == arg       # the two chroma components share table 1
    info.bw0 += 1
    assert _encode(lib, c["coef"], info, c["qtab"], n)[0] == arg
    bound = ctypes.c_int64(0)
    assert lib.vunet_jpeg_encode_bound(ctypes.byref(info), ctypes.byref(bound)) == arg


# ---- jpeg_encode.encode_batch and video_io with the device step replaced by the restatement
@pytest.fixture
def stubbed(monkeypatch):
    from behavior_driven_video_synthesis_amd import jpeg_encode as J
    calls = []

    def launch(buf, frames, m, channels, up_bytes, q_off, q_count, coef_count):
        stage = buf.stage.numpy()
        rows = (J.JpegImg * m).from_buffer_copy(stage[:m * ctypes.sizeof(J.JpegImg)].tobytes())
        assert q_off == m * 64 and up_bytes == q_off + 2 * q_count and q_count % 192 == 0
        qtab = stage[q_off:up_bytes].view(np.uint16)
        dst, blocks = buf.coef_host.numpy(), 0
        for r in rows:
            assert r.block0 == blocks and r.coef_off % 64 == 0 and r.plane_off % 16 == 0 and r.q_off % 192 == 0 and r.ncomp == channels
            img = frames[r.slot, :r.height, :r.width].numpy()
            planes, geo = E.from_rgb(img, r.hsamp, r.vsamp)
            assert geo["blocks"][0] == (r.bh0, r.bw0) and (r.ncomp == 1 or geo["blocks"][1] == (r.bh1, r.bw1))
            flat = E.flat_coef(E.coefficients(planes, geo, qtab[r.q_off:r.q_off + 128].reshape(2, 64)))
            dst[r.coef_off:r.coef_off + len(flat)] = flat
            blocks += len(flat) // 64
        assert blocks * 64 == coef_count
        calls.append(m)
    monkeypatch.setattr(J, "_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(J, "_launch", launch)
    J.clear_buffers()
    yield J, calls
    J.clear_buffers()


def test_encode_batch_stages_what_the_kernels_need(stubbed, cases):
    J, calls = stubbed
    names = [n for n in cases if n.endswith("_q95_s422") and "noise" in n]
    stack = torch.full((len(names), 250, 250, 3), 7, dtype=torch.uint8)
    sizes = []
    for i, n in enumerate(names):
        img = cases[n]["img"]
        stack[i, :img.shape[0], :img.shape[1]] = torch.from_numpy(img)
        sizes.append(img.shape[:2])
    got = J.encode_batch(stack, quality=95, subsampling="4:2:2", sizes=sizes, threads=3)
    assert calls == [len(names)] and [type(g) for g in got] == [bytes] * len(names)
    for n, g in zip(names, got):
        assert g == cases[n]["data"], n
    c = cases["gray_37x45_ramp_q95"]
    assert J.encode_batch(torch.from_numpy(c["img"])[None], quality=95) == [c["data"]]
    for kw in (dict(quality=0), dict(quality=101), dict(subsampling="4:1:1"), dict(threads=0), dict(threads=17), dict(sizes=[(1, 1)]),
               dict(sizes=[(251, 1)] * len(names))):
        with pytest.raises(ValueError):
            J.encode_batch(stack, **kw)
    for bad in (stack.float(), stack[0, 0], stack[..., :2], stack.numpy()):
        with pytest.raises(ValueError):
            J.encode_batch(bad)
    assert len(calls) == 2


def test_a_stream_longer_than_its_share_of_the_buffer_is_coded_again(stubbed, cases, monkeypatch):
    """``encode_batch`` gives every image two bytes per coefficient; the capacity code sends a longer stream through a second call
    with the length the first one asked for.  Forced here by coefficients at their longest codes."""
    J, calls = stubbed
    real = J._launch

    def launch(buf, *a):
        real(buf, *a)
        dst = buf.coef_host.numpy()
        dst[:] = np.where(np.arange(dst.size) % 2, 1023, -1023).astype(np.int16)
        dst[0::64] = 0
    monkeypatch.setattr(J, "_launch", launch)
    img = torch.zeros(1, 16, 16, 3, dtype=torch.uint8)
    (data,) = J.encode_batch(img, quality=100, subsampling="4:4:4")
    assert len(data) > 1024 + 2 * 3 * 4 * 64 and data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
    import jpeg_ref as R
    coef, _ = R.entropy_decode(data)
    assert all((abs(c[..., 1:]) == 1023).all() and (c[..., 0] == 0).all() for c in coef)


def _walk(data, at, end):
    out = []
    while at < end:
        tag, size = data[at:at + 4], struct.unpack_from("<I", data, at + 4)[0]
        out.append((tag, at + 8, size))
        at += 8 + size + (size & 1)
    assert at == end, "the chunks do not fill their parent exactly"
    return out


def test_mjpeg_file_is_consistent_and_round_trips(stubbed, cases, tmp_path):
    """``write_mjpeg`` (frames through the stubbed ``encode_batch``) and ``write_mjpeg_streams`` (the fixture's bytes): every chunk
    size, the RIFF size and every idx1 offset agree with the file, odd-length frames are padded, and ``read_mjpeg`` returns the
    streams unchanged."""
    from behavior_driven_video_synthesis_amd import video_io as V
    J, calls = stubbed
    names = [f"64x64_{k}_q{q}_s420" for k in E.CONTENTS for q in (30, 75, 95)]
    streams = [cases[n]["data"] for n in names]
    assert any(len(s) & 1 for s in streams) and any(not len(s) & 1 for s in streams)
    path = str(tmp_path / "fixture.avi")
    assert V.write_mjpeg_streams(path, streams, 64, 64, fps=12) == path
    frames = torch.stack([torch.from_numpy(cases[n]["img"]) for n in ("64x64_noise_q75_s420", "64x64_ramp_q75_s420", "64x64_sat_q75_s420")])
    path2 = str(tmp_path / "frames.avi")
    V.write_mjpeg(path2, frames, fps=12.5, quality=75, subsampling="4:2:0")
    want2 = [cases[n]["data"] for n in ("64x64_noise_q75_s420", "64x64_ramp_q75_s420", "64x64_sat_q75_s420")]
    for p, want, rate, scale in ((path, streams, 12, 1), (path2, want2, 25, 2)):
        data = open(p, "rb").read()
        assert data[:4] == b"RIFF" and struct.unpack_from("<I", data, 4)[0] == len(data) - 8 and data[8:12] == b"AVI "
        top = _walk(data, 12, len(data))
        assert [(t, data[a:a + 4] if t == b"LIST" else None) for t, a, _ in top] == [(b"LIST", b"hdrl"), (b"LIST", b"movi"), (b"idx1", None)]
        (_, ha, hsz), (_, ma, msz), (_, ia, isz) = top
        hdrl = _walk(data, ha + 4, ha + hsz)
        assert [t for t, _, _ in hdrl] == [b"avih", b"LIST"] and hdrl[0][2] == 56 and data[hdrl[1][1]:hdrl[1][1] + 4] == b"strl"
        avih = struct.unpack_from("<14I", data, hdrl[0][1])
        assert avih[0] == round(1e6 * scale / rate) and avih[3] & 0x10 and avih[4] == len(want) and avih[6] == 1 and avih[8:10] == (64, 64)
        assert avih[7] == max(len(s) for s in want)
        strl = _walk(data, hdrl[1][1] + 4, hdrl[1][1] + hdrl[1][2])
        assert [(t, s) for t, _, s in strl] == [(b"strh", 56), (b"strf", 40)]
        strh = struct.unpack_from("<4s4sIHHIIIIIIIIHHHH", data, strl[0][1])
        assert strh[:2] == (b"vids", b"MJPG") and strh[6:8] == (scale, rate) and strh[9] == len(want) and strh[-2:] == (64, 64)
        strf = struct.unpack_from("<IiiHH4sIiiII", data, strl[1][1])
        assert strf[:7] == (40, 64, 64, 1, 24, b"MJPG", 64 * 64 * 3)
        movi = _walk(data, ma + 4, ma + msz)
        assert [t for t, _, _ in movi] == [b"00dc"] * len(want) and [data[a:a + s] for _, a, s in movi] == want
        for _, a, s in movi:
            if s & 1:
                assert data[a + s] == 0 and (a + s + 1 == ma + msz or data[a + s + 1:a + s + 5] == b"00dc")
        assert isz == 16 * len(want)
        for i, (_, a, s) in enumerate(movi):
            ckid, flags, off, size = struct.unpack_from("<4sIII", data, ia + 16 * i)
            assert (ckid, flags, size) == (b"00dc", 0x10, s) and ma + off == a - 8, i     # from the 'movi' tag to the chunk header
        fps, back = V.read_mjpeg(p)
        assert fps == rate / scale and back == want
    # a damaged file is refused, not half read
    data = open(path, "rb").read()
    m, i = data.index(b"movi"), data.index(b"idx1")
    for bad in (data[:len(data) // 2], b"RIFX" + data[4:], data[:m - 4] + struct.pack("<I", 1 << 30) + data[m:],
                data[:m + 8] + struct.pack("<I", len(streams[0]) + 2) + data[m + 12:], data[:i + 16] + b"\x06" + data[i + 17:]):
        q = str(tmp_path / "bad.avi")
        open(q, "wb").write(bad)
        with pytest.raises(ValueError):
            V.read_mjpeg(q)
    with pytest.raises(ValueError):
        V.write_mjpeg_streams(path, [], 64, 64)
    with pytest.raises(ValueError):
        V.write_mjpeg_streams(path, [b"nope"], 64, 64)


def test_save_videos_and_save_images_name_one_file_per_row(stubbed, cases, tmp_path):
    from behavior_driven_video_synthesis_amd import video_io as V
    J, calls = stubbed
    a, b = cases["16x16_noise_q75_s420"], cases["16x16_ramp_q75_s420"]
    clip = torch.stack([torch.from_numpy(a["img"]), torch.from_numpy(b["img"])])
    rows = torch.stack([clip, clip.flip(0), clip])
    paths = V.save_videos(str(tmp_path / "row_%02d.avi"), rows, start=4)
    assert [os.path.basename(p) for p in paths] == ["row_04.avi", "row_05.avi", "row_06.avi"] and calls == [6]
    assert V.read_mjpeg(paths[0]) == (12.0, [a["data"], b["data"]]) and V.read_mjpeg(paths[1])[1] == [b["data"], a["data"]]
    imgs = J.save_images(str(tmp_path / "img_{:06d}.jpg"), clip)
    assert [os.path.basename(p) for p in imgs] == ["img_000000.jpg", "img_000001.jpg"]
    assert open(imgs[1], "rb").read() == b["data"]
    with pytest.raises(ValueError):
        J.save_images(str(tmp_path / "same.jpg"), clip)
