"""The host half of the JPEG decoder without a GPU: ``vunet_jpeg_parse`` / ``vunet_jpeg_entropy_decode`` (csrc/jpeg_entropy.h through
the library's C ABI) against the restatement (tests/jpeg_ref.py) and the fixture's arrays (tests/golden/g23_jpeg.npz); the refused
and damaged streams; and the host side of behavior_driven_video_synthesis_amd/jpeg_decode.py and of the trainers' hook with the
upload-and-launch step replaced by the restatement."""
import ctypes
import os

import numpy as np
import pytest
import torch

import jpeg_ref as R

GUARD = 4096          # int16 words after the announced coefficient count
SENTINEL = 0x5A5A


@pytest.fixture(scope="module")
def lib():
    from behavior_driven_video_synthesis_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def fixture():
    return R.load_fixture()


def _parse(lib, data):
    from behavior_driven_video_synthesis_amd import _lib
    info = _lib.struct("vunet_jpeg_info")()
    return lib.vunet_jpeg_parse(data, len(data), ctypes.byref(info)), info


def _decode(lib, data, info):
    """-> (return code, coef [ncoef], qtab [ncomp, 64]); asserts that the guard words behind both buffers are untouched."""
    coef = np.full(info.ncoef + GUARD, SENTINEL, dtype=np.int16)
    qtab = np.full(info.ncomp * 64 + GUARD, SENTINEL, dtype=np.uint16)
    rc = lib.vunet_jpeg_entropy_decode(data, len(data), ctypes.byref(info), coef.ctypes.data, qtab.ctypes.data)
    assert (coef[info.ncoef:] == SENTINEL).all() and (qtab[info.ncomp * 64:] == SENTINEL).all()
    return rc, coef[:info.ncoef], qtab[:info.ncomp * 64].reshape(info.ncomp, 64)


def test_parse_geometry_equals_the_restatement(lib, fixture):
    for name, c in fixture["cases"].items():
        rc, info = _parse(lib, c["data"])
        h = R.parse(c["data"])
        assert rc == 0, (name, rc)
        assert (info.height, info.width, info.ncomp, info.hsamp, info.vsamp) == (h["height"], h["width"], h["ncomp"], h["hsamp"], h["vsamp"])
        assert (info.mcu_cols, info.mcu_rows, info.restart, info.ncoef) == (h["mcu_cols"], h["mcu_rows"], h["restart"], h["ncoef"]), name
        assert (info.bh0, info.bw0) == h["blocks"][0] and info.nblocks * 64 == info.ncoef
        assert (info.bh1, info.bw1) == (h["blocks"][1] if h["ncomp"] == 3 else (0, 0)), name
        assert c["rgb"].shape == (info.height, info.width, 3)


def test_entropy_decode_equals_the_fixture(lib, fixture):
    for name, c in fixture["cases"].items():
        rc, info = _parse(lib, c["data"])
        rc, coef, qtab = _decode(lib, c["data"], info)
        assert rc == 0, (name, rc)
        assert np.array_equal(coef, c["coef"]), (name, int((coef != c["coef"]).sum()))
        assert np.array_equal(qtab, c["qtab"]), name


def test_entropy_decode_refuses_another_streams_info(lib, fixture):
    from behavior_driven_video_synthesis_amd import _lib
    a, b = fixture["cases"]["s420_16x16_smooth"]["data"], fixture["cases"]["s420_17x23_smooth"]["data"]
    _, info = _parse(lib, a)
    assert _decode(lib, b, info)[0] == _lib.const("VUNET_ERR_ARG")


def test_refused_streams_return_their_unsupported_code(lib, fixture):
    from behavior_driven_video_synthesis_amd import _lib, jpeg_decode as J
    want = {"progressive": "VUNET_JPEG_ERR_SOF", "cmyk": "VUNET_JPEG_ERR_COMPONENTS"}
    for name, data in fixture["refused"].items():
        rc, _ = _parse(lib, data)
        assert rc == _lib.const(want[name]), (name, rc)
        with pytest.raises(J.JpegUnsupported) as e:
            J.parse(data)
        assert e.value.code == rc and e.value.reason == J.REASONS[rc]
    # hand-made: a 16-bit quantisation table, a 4:1:1 frame, a second scan
    data = fixture["cases"]["s420_16x16_smooth"]["data"]
    dqt = data.index(b"\xff\xdb")
    assert _parse(lib, data[:dqt + 4] + bytes([data[dqt + 4] | 0x10]) + data[dqt + 5:])[0] == _lib.const("VUNET_JPEG_ERR_PRECISION")
    sof = data.index(b"\xff\xc0")
    assert data[sof + 11] == 0x22
    assert _parse(lib, data[:sof + 11] + b"\x41" + data[sof + 12:])[0] == _lib.const("VUNET_JPEG_ERR_SAMPLING")
    sos = data.index(b"\xff\xda")
    one = data[:sos] + b"\xff\xda\x00\x08\x01" + data[sos + 5:sos + 7] + data[sos + 11:]
    assert _parse(lib, one)[0] == _lib.const("VUNET_JPEG_ERR_SCANS")


def test_damaged_streams_return_a_code_or_decode_and_stay_inside_their_buffers(lib, fixture):
    """Every prefix of one 4:2:0 stream (the fixture's offsets among them) and of one with restart markers, and single flipped bits
    in the scan: an error code or a decode, never a write past the announced counts (``_decode`` checks the guard words)."""
    from behavior_driven_video_synthesis_amd import _lib
    name, offs = fixture["truncated"]
    corrupt = set(range(-109, -99))
    for case in (name, "s420_41x39_rstrow_noise", "s444_40x56_rst4_smooth"):
        data = fixture["cases"][case]["data"]
        scan, codes = R.parse(data)["scan"], {}
        for n in range(len(data)):
            cut = data[:n]
            rc, info = _parse(lib, cut)
            if rc == 0:
                assert n >= scan
                rc = _decode(lib, cut, info)[0]
            assert rc in corrupt, (case, n, rc)       # a prefix is never a whole stream: at least the EOI is missing
            codes[n] = rc
        assert codes[len(data) - 2] == _lib.const("VUNET_JPEG_ERR_TRUNCATED")
        if case == name:
            assert all(codes[o] in corrupt for o in offs)
    data = fixture["cases"][name]["data"]
    scan, n_ok, g = R.parse(data)["scan"], 0, np.random.default_rng(5)
    _, info = _parse(lib, data)
    for pos in sorted({scan, scan + 1, len(data) - 3} | {int(v) for v in g.integers(scan, len(data) - 2, size=48)}):
        for bit in (0, 3, 7):
            bad = bytearray(data)
            bad[pos] ^= 1 << bit
            rc, coef, _ = _decode(lib, bytes(bad), info)
            assert rc == 0 or rc in corrupt, (pos, bit, rc)
            n_ok += rc == 0
    print(f"flipped bits: {n_ok} of {51 * 3} streams still decode")
    rst = fixture["cases"]["s420_41x39_rstrow_noise"]["data"]       # a restart marker out of sequence
    k = rst.index(b"\xff\xd1", R.parse(rst)["scan"])
    _, info = _parse(lib, rst)
    assert _decode(lib, rst[:k + 1] + b"\xd3" + rst[k + 2:], info)[0] == _lib.const("VUNET_JPEG_ERR_RESTART")


# ---- jpeg_decode.decode_batch and the trainers' hook with the device step replaced by the restatement
@pytest.fixture
def stubbed(monkeypatch):
    from behavior_driven_video_synthesis_amd import jpeg_decode as J
    calls = []

    def launch(buf, m, nbytes, q_off, c_off, coef_count, plane_bytes, out):
        stage = buf.stage.numpy()
        rows = (J.JpegImg * m).from_buffer_copy(stage[:m * ctypes.sizeof(J.JpegImg)].tobytes())
        assert c_off % 128 == 0 and nbytes == c_off + 2 * coef_count and q_off == m * 64
        coef = stage[c_off:nbytes].view(np.int16)
        qtab = stage[q_off:q_off + 384 * m].view(np.uint16)
        blocks = 0
        for r in rows:
            assert r.block0 == blocks and r.coef_off % 64 == 0 and r.plane_off % 16 == 0 and r.q_off % 8 == 0
            grids = [(r.bh0, r.bw0)] + [(r.bh1, r.bw1)] * (r.ncomp - 1)
            cs, at = [], r.coef_off
            for bh, bw in grids:
                cs.append(coef[at:at + bh * bw * 64].reshape(bh, bw, 64))
                at += bh * bw * 64
            blocks += sum(bh * bw for bh, bw in grids)
            hdr = dict(height=r.height, width=r.width, ncomp=r.ncomp, hsamp=r.hsamp, vsamp=r.vsamp)
            rgb = R.to_rgb(R.planes(cs, qtab[r.q_off:r.q_off + 64 * r.ncomp].reshape(r.ncomp, 64)), hdr)
            out[r.slot, :r.height, :r.width] = torch.from_numpy(rgb)
        calls.append(m)
    monkeypatch.setattr(J, "_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(J, "_launch", launch)
    J.clear_buffers()
    yield J, calls
    J.clear_buffers()


def test_decode_batch_stages_what_the_kernels_need(stubbed, fixture):
    J, calls = stubbed
    names = list(fixture["cases"])
    data = [fixture["cases"][n]["data"] for n in names]
    out = torch.full((len(data), 52, 71, 3), 0xAB, dtype=torch.uint8)
    frames, hw = J.decode_batch(data, hmax=52, wmax=71, out=out, threads=3)
    assert frames is out and calls == [len(data)] and hw.dtype == torch.int32 and not hw.is_cuda
    for i, n in enumerate(names):
        rgb = fixture["cases"][n]["rgb"]
        h, w = rgb.shape[:2]
        assert hw[i].tolist() == [h, w] and np.array_equal(out[i, :h, :w].numpy(), rgb), n
        assert (out[i, h:] == 0xAB).all() and (out[i, :, w:] == 0xAB).all(), n
    again, _ = J.decode_batch(data[:3], tag="a")
    assert again.shape == (3, 16, 16, 3) and J.decode_batch(data[:3], tag="a")[0] is again and J.decode_batch(data[:3], tag="b")[0] is not again


def test_decode_batch_checks_its_arguments(stubbed, fixture):
    J, calls = stubbed
    c = fixture["cases"]
    ok, big = c["s444_8x8_smooth"]["data"], c["s420_50x70_q100_smooth"]["data"]
    for bad, exc in ((ok, TypeError), ([], ValueError), (["text"], TypeError), ([ok, None], TypeError)):
        with pytest.raises(exc):
            J.decode_batch(bad)
    for kw in (dict(threads=0), dict(threads=17), dict(hmax=49), dict(wmax=8), dict(out=torch.zeros(2, 50, 70, 3)),
               dict(out=torch.zeros(1, 50, 70, 3, dtype=torch.uint8)), dict(out=torch.zeros(2, 50, 70, 3, dtype=torch.uint8)[:, :, ::1].transpose(1, 2))):
        with pytest.raises(ValueError):
            J.decode_batch([ok, big], **kw)
    assert calls == []
    with pytest.raises(J.JpegUnsupported) as e:
        J.decode_batch([ok, fixture["refused"]["progressive"]])
    assert e.value.index == 1 and e.value.code == J._lib.const("VUNET_JPEG_ERR_SOF")
    with pytest.raises(J.JpegCorrupt) as e:
        J.decode_batch([ok, big[:len(big) // 2]], fallback=True)          # corrupt streams raise with the fallback too
    assert e.value.index == 1 and e.value.code == J._lib.const("VUNET_JPEG_ERR_TRUNCATED")
    with pytest.raises(J.JpegCorrupt):
        J.decode_batch([b"not a jpeg"])
    assert calls == []
    assert J.parse(bytearray(ok)).ncoef == 3 * 64 and J.parse(ok)._fields[0] == "height"


def test_fallback_hands_unsupported_streams_to_pillow(stubbed, fixture):
    Image = pytest.importorskip("PIL.Image")
    import io
    J, calls = stubbed
    prog, ok = fixture["refused"]["progressive"], fixture["cases"]["s420_17x23_noise"]
    frames, hw = J.decode_batch([prog, ok["data"]], fallback=True)
    want = np.asarray(Image.open(io.BytesIO(prog)).convert("RGB"))
    assert calls == [1] and hw.tolist() == [[24, 24], [17, 23]]
    assert np.array_equal(frames[0, :24, :24].numpy(), want) and np.array_equal(frames[1, :17, :23].numpy(), ok["rgb"])


def test_batch_images_decodes_the_jpeg_keys(stubbed, fixture, monkeypatch):
    from behavior_driven_video_synthesis_amd import image_input as I
    J, calls = stubbed
    seen = []

    def frames_to_images(frames, geom=None, size=256, out_u8=False):
        seen.append((frames.clone(), None if geom is None else torch.as_tensor(geom).clone(), size))
        return torch.zeros(frames.shape[0], 3, size, size), torch.zeros(frames.shape[0], dtype=torch.int32)
    monkeypatch.setattr(I, "frames_to_images", frames_to_images)
    names = ["s420_17x23_smooth", "gray_24x31_noise", "s422_33x41_smooth"]
    data = [fixture["cases"][n]["data"] for n in names]
    made = I.batch_images({"pose_img_jpeg": data, "stickman": 0}, 32)
    assert sorted(made) == ["pose_img", "pose_img_status"] and calls == [3]
    frames, geom, size = seen.pop()
    assert size == 32 and frames.shape == (3, 33, 41, 3)
    assert geom.tolist() == [[17, 23, 0, 0, 23, 17], [24, 31, 0, 0, 31, 24], [33, 41, 0, 0, 41, 33]]
    for i, n in enumerate(names):
        rgb = fixture["cases"][n]["rgb"]
        assert np.array_equal(frames[i, :rgb.shape[0], :rgb.shape[1]].numpy(), rgb), n
    # a geometry of the batch's own is kept; both inputs decode into stacks of their own; ready images are left alone
    g = np.asarray([[17, 23, 1, 2, 8, 8]], dtype=np.int32)
    batch = {"pose_img_jpeg": data[:1], "pose_img_geom": g, "app_img_jpeg": data[:1]}
    staged = I.decode_jpeg(batch)
    assert "pose_img_jpeg" not in staged and "app_img_jpeg" not in staged and staged["pose_img_geom"] is g
    assert staged["pose_img_u8"] is not staged["app_img_u8"] and torch.equal(staged["pose_img_u8"], staged["app_img_u8"])
    assert staged["app_img_geom"].tolist() == [[17, 23, 0, 0, 23, 17]] and "pose_img_jpeg" in batch
    plain = {"pose_img": torch.zeros(1, 3, 4, 4), "pose_img_jpeg": data[:1]}
    assert I.decode_jpeg(plain) is plain and I.batch_images(plain, 4) == {}
    none = {"pose_img_u8": torch.zeros(1, 4, 4, 3, dtype=torch.uint8)}
    assert I.decode_jpeg(none) is none
    aug = I.decode_jpeg({"pose_img_jpeg": data[:1], "pose_img_aug": np.zeros((1, 6))})
    assert "pose_img_geom" not in aug and aug["pose_img_hw"].tolist() == [[17, 23]]
