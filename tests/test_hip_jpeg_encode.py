"""The JPEG encode on the GPU (csrc/jpeg_enc.hip, behavior_driven_video_synthesis_amd/jpeg_encode.py, video_io.py) against Pillow's
bytes and the coefficients they hold (tests/golden/g24_jpeg_encode.npz) and the restatement (tests/jpeg_enc_ref.py, itself held to
Pillow in tests/test_jpeg_enc_ref.py): every case one image at a time -- coefficients, dummy blocks included, and bytes (A); the
whole fixture of mixed sizes, samplings and qualities in one padded stack in one call (B); one 1000 x 1002 frame (C); the round trip
through the decoder (D); no allocation on a second call (E); descriptors that point outside their buffers (F); Motion-JPEG files
(G, H).

Everything is exact: the encoder is integer arithmetic throughout, so there is no tolerance."""
import ctypes

import numpy as np
import pytest
import torch

import jpeg_enc_ref as E
import jpeg_ref as R

pytestmark = pytest.mark.gpu

FIX = E.load_fixture()
COLOUR = [n for n, c in FIX.items() if c["img"].ndim == 3]
GRAY = [n for n, c in FIX.items() if c["img"].ndim == 2]
GROUPS = [f"{h}x{w}_" for h, w in E.SIZES] + ["gray_"]


def _coef_of_last_call(J, count):
    (buf,) = J._buffers.values()
    return buf.coef_host[:count].numpy().copy()


@pytest.mark.parametrize("group", GROUPS)
def test_one_image_at_a_time_coefficients_and_bytes_equal_pillows(group):
    """A: every case of one size (3 contents x 4 qualities x 3 samplings; the two gray cases) from a batch of one: the coefficients the
    two launches leave -- every dummy block among them -- equal those of Pillow's stream, and ``encode_batch``'s bytes are Pillow's."""
    from behavior_driven_video_synthesis_amd import jpeg_encode as J
    J.clear_buffers()
    names = [n for n in FIX if n.startswith(group)]
    assert len(names) == (2 if group == "gray_" else 36)
    for name in names:
        c = FIX[name]
        (data,) = J.encode_batch(torch.from_numpy(c["img"]).cuda()[None], quality=c["quality"], subsampling=c["subsampling"], threads=1)
        coef = _coef_of_last_call(J, len(c["coef"]))
        assert np.array_equal(coef, c["coef"]), (name, int((coef != c["coef"]).sum()), np.flatnonzero(coef != c["coef"])[:8].tolist())
        assert data == c["data"], (name, len(data), len(c["data"]))
    J.clear_buffers()


def _stack(names, hmax, wmax, fill=0x5B):
    shape = (len(names), hmax, wmax, 3) if FIX[names[0]]["img"].ndim == 3 else (len(names), hmax, wmax)
    stack = np.full(shape, fill, dtype=np.uint8)
    for i, n in enumerate(names):
        img = FIX[n]["img"]
        stack[i, :img.shape[0], :img.shape[1]] = img
    return torch.from_numpy(stack).cuda(), [FIX[n]["img"].shape[:2] for n in names]


def test_whole_fixture_in_one_padded_stack_in_one_call_equals_pillow():
    """B: all 360 colour cases -- mixed sizes, samplings and qualities -- in ONE stack larger than any of them with ``sizes``: one
    upload, two launches, one download; then the two gray cases in a stack of their own.  Bytes outside an image never reach it."""
    from behavior_driven_video_synthesis_amd import jpeg_encode as J
    J.clear_buffers()
    for names in (COLOUR, GRAY):
        stack, sizes = _stack(names, 251, 253)
        got = J.encode_batch(stack, quality=[FIX[n]["quality"] for n in names], subsampling=[FIX[n]["subsampling"] for n in names],
                             sizes=sizes)
        coef = _coef_of_last_call(J, sum(len(FIX[n]["coef"]) for n in names))
        want = np.concatenate([FIX[n]["coef"] for n in names])
        assert np.array_equal(coef, want), int((coef != want).sum())
        bad = [n for n, g in zip(names, got) if g != FIX[n]["data"]]
        assert not bad, bad[:10]
    J.clear_buffers()


@pytest.fixture(scope="module")
def big():
    """One 1002 x 1000 (H x W) noise-plus-ramp frame and the restatement's coefficients and bytes of it, made once."""
    g = np.random.default_rng(1002)
    yy, xx = np.mgrid[0:1002, 0:1000]
    img = np.stack([(xx * 255) // 999, (yy * 255) // 1001, ((xx + yy) * 255) // 2000], axis=2) + g.integers(-24, 25, size=(1002, 1000, 3))
    img = np.clip(img, 0, 255).astype(np.uint8)
    coef, qtab, geo = E.image_coefficients(img, 75, "4:2:0")
    return img, E.flat_coef(coef), E.entropy_encode(coef, geo, qtab)


def test_a_1000_by_1002_frame_equals_the_restatement(big):
    """C: the wide-image index arithmetic -- more than one block of lanes per row is not needed at 4 pixels a thread, but 63 x 63
    MCUs, a dummy block column (1000 = 125 blocks, 126 with padding) and 23 814 blocks in 745 groups are."""
    from behavior_driven_video_synthesis_amd import jpeg_encode as J
    img, coef, data = big
    J.clear_buffers()
    (got,) = J.encode_batch(torch.from_numpy(img).cuda()[None], quality=75, subsampling="4:2:0")
    dev = _coef_of_last_call(J, len(coef))
    assert np.array_equal(dev, coef), int((dev != coef).sum())
    assert got == data
    J.clear_buffers()


def test_rows_wider_than_one_block_of_lanes_equal_the_restatement():
    """C: 9 x 1100 -- 276 threads of four pixels per row, so two blocks of lanes, the second one partly idle -- at every sampling in
    one call, against the restatement's coefficients and bytes."""
    from behavior_driven_video_synthesis_amd import jpeg_encode as J
    J.clear_buffers()
    img = np.random.default_rng(1100).integers(0, 256, size=(9, 1100, 3), dtype=np.uint8)
    subs = list(E.SAMPLING)
    got = J.encode_batch(torch.from_numpy(np.stack([img] * 3)).cuda(), quality=95, subsampling=subs)
    want = [E.image_coefficients(img, 95, s) for s in subs]
    flat = np.concatenate([E.flat_coef(c) for c, _, _ in want])
    dev = _coef_of_last_call(J, len(flat))
    assert np.array_equal(dev, flat), int((dev != flat).sum())
    assert got == [E.entropy_encode(c, geo, q) for c, q, geo in want]
    J.clear_buffers()


def _pillow_rgb(data):
    """Pillow's decode where PIL imports (held equal to the decoder's restatement), the restatement alone otherwise."""
    want = R.decode(data)
    try:
        import io
        from PIL import Image
    except ImportError:
        return want
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")), want)
    return want


def test_decode_of_encode_equals_pillows_decode_of_pillows_encode():
    """D: ``decode_batch(encode_batch(x))`` against Pillow's decode of the fixture's (Pillow's) streams, mixed cases in one batch."""
    from behavior_driven_video_synthesis_amd import jpeg_decode as D, jpeg_encode as J
    names = ["17x23_noise_q75_s420", "37x45_ramp_q95_s422", "24x8_sat_q100_s420", "8x24_noise_q30_s444", "1x250_ramp_q75_s420",
             "250x1_noise_q95_s420", "1x1_sat_q75_s420"]
    stack, sizes = _stack(names, 250, 250)
    streams = J.encode_batch(stack, quality=[FIX[n]["quality"] for n in names], subsampling=[FIX[n]["subsampling"] for n in names], sizes=sizes)
    frames, hw = D.decode_batch(streams)
    assert hw.tolist() == [list(s) for s in sizes]
    got = frames.cpu().numpy()
    for i, n in enumerate(names):
        h, w = sizes[i]
        assert np.array_equal(got[i, :h, :w], _pillow_rgb(FIX[n]["data"])), n
    J.clear_buffers()


def test_second_call_at_a_shape_allocates_nothing():
    """E: the descriptor block, its device mirror, the planes, the coefficients and their pinned copy are reused -- same addresses, and
    the allocator's count of live bytes does not move."""
    from behavior_driven_video_synthesis_amd import jpeg_encode as J
    J.clear_buffers()
    a, sizes = _stack([n for n in COLOUR if n.endswith("_noise_q75_s420")], 250, 250)
    b, _ = _stack([n for n in COLOUR if n.endswith("_sat_q75_s420")], 250, 250)
    first = J.encode_batch(a, sizes=sizes)
    (buf,) = J._buffers.values()
    ptrs = (buf.stage.data_ptr(), buf.dev.data_ptr(), buf.planes.data_ptr(), buf.coef.data_ptr(), buf.coef_host.data_ptr())
    torch.cuda.synchronize()
    live = torch.cuda.memory_allocated()
    again = J.encode_batch(b, sizes=sizes)                 # other frames, the same sizes
    assert (buf.stage.data_ptr(), buf.dev.data_ptr(), buf.planes.data_ptr(), buf.coef.data_ptr(), buf.coef_host.data_ptr()) == ptrs
    assert torch.cuda.memory_allocated() == live and buf.stage.is_pinned() and buf.coef_host.is_pinned()
    assert first == [FIX[n]["data"] for n in COLOUR if n.endswith("_noise_q75_s420")]
    assert again == [FIX[n]["data"] for n in COLOUR if n.endswith("_sat_q75_s420")]
    J.clear_buffers()


def test_descriptors_that_point_outside_their_buffers_are_refused_before_any_launch():
    """F: the two entry points by hand on two images; then rows whose offsets, grids or sizes do not fit are VUNET_ERR_ARG."""
    from behavior_driven_video_synthesis_amd import jpeg_encode as J
    from behavior_driven_video_synthesis_amd.ops import _call, _p, _stream
    names = ["37x45_noise_q75_s420", "17x23_noise_q75_s422"]
    stack, sizes = _stack(names, 40, 48)
    rows, at, blocks = (J.JpegImg * 2)(), 0, 0
    for j, n in enumerate(names):
        g = E.geometry(*sizes[j], 3, *E.SAMPLING[FIX[n]["subsampling"]])
        r = rows[j]
        r.coef_off, r.plane_off, r.q_off, r.block0, r.slot = at, at, 0, blocks, j
        r.height, r.width, r.ncomp, r.hsamp, r.vsamp = g["height"], g["width"], 3, g["hsamp"], g["vsamp"]
        (r.bh0, r.bw0), (r.bh1, r.bw1) = g["blocks"][0], g["blocks"][1]
        at, blocks = at + g["ncoef"], blocks + g["ncoef"] // 64
    qtab = torch.from_numpy(E.quant_tables(75)[[0, 1, 1]].astype(np.int16)).cuda()
    imgs = torch.frombuffer(bytearray(bytes(rows)), dtype=torch.uint8).cuda()
    planes, coef = torch.empty(at, dtype=torch.uint8, device="cuda"), torch.zeros(at, dtype=torch.int16, device="cuda")
    host = ctypes.cast(rows, ctypes.c_void_p)

    def from_rgb():
        _call("vunet_jpeg_from_rgb", _p(stack), 2, 40, 48, 3, _p(imgs), host, 2, _p(planes), at, _stream())

    def fdct():
        _call("vunet_jpeg_fdct", _p(planes), at, _p(qtab), 192, _p(imgs), host, 2, _p(coef), at, _stream())
    from_rgb()
    fdct()
    assert np.array_equal(coef.cpu().numpy(), np.concatenate([FIX[n]["coef"] for n in names]))
    for field, delta, calls in (("coef_off", 64, [fdct]), ("plane_off", 16, [from_rgb, fdct]), ("q_off", 8, [fdct]), ("height", 24, [from_rgb]),
                                ("bw0", 2, [from_rgb, fdct]), ("bh1", 1, [from_rgb, fdct]), ("slot", 1, [from_rgb])):
        setattr(rows[1], field, getattr(rows[1], field) + delta)
        for call in calls:
            with pytest.raises(RuntimeError, match="vunet_jpeg_f"):
                call()
        setattr(rows[1], field, getattr(rows[1], field) - delta)
    from_rgb()
    fdct()
    torch.cuda.synchronize()


def test_mjpeg_clip_round_trips_through_the_decoder():
    """G: ``write_mjpeg`` of a 5-frame 32 x 48 clip, ``read_mjpeg``, ``decode_batch``: the frames of Pillow's round trip (the
    restatement's encode -- Pillow's bytes -- decoded as Pillow decodes them)."""
    import os
    import tempfile
    from behavior_driven_video_synthesis_amd import jpeg_decode as D, video_io as V
    g = np.random.default_rng(48)
    yy, xx = np.mgrid[0:32, 0:48]
    clip = np.stack([np.clip(np.stack([xx * 5 + 9 * t, yy * 7, (xx + yy) * 3 + 20 * t], axis=2) + g.integers(-9, 10, size=(32, 48, 3)), 0, 255)
                     for t in range(5)]).astype(np.uint8)
    with tempfile.TemporaryDirectory() as d:
        path = V.write_mjpeg(os.path.join(d, "clip.avi"), torch.from_numpy(clip).cuda(), fps=12, quality=75, subsampling="4:2:0")
        fps, streams = V.read_mjpeg(path)
    assert fps == 12.0 and streams == [E.encode(f, 75, "4:2:0") for f in clip]
    frames, hw = D.decode_batch(streams)
    assert hw.tolist() == [[32, 48]] * 5
    got = frames.cpu().numpy()
    for t in range(5):
        assert np.array_equal(got[t], _pillow_rgb(streams[t])), t


def test_skeleton_video_goes_through_save_videos_one_file_per_row():
    """H: what ``render.skeleton_video`` returns, [rows, T, H, W, 3] on the device, through ``save_videos``: one well-formed file per
    row whose frames are the restatement's streams of the rendered frames."""
    import os
    import tempfile
    from synth import seeded_randn
    from test_hip_skeleton import _net_and_camera
    from behavior_driven_video_synthesis_amd import video_io as V
    from behavior_driven_video_synthesis_amd.render import skeleton_video, transfer_video
    net, cam = _net_and_camera()
    beh, start = (0.5 * seeded_randn("enc.beh", (2, 3, 51), 24)).cuda(), (0.5 * seeded_randn("enc.start", (2, 5, 51), 24)).cuda()
    _, poses, _ = transfer_video(net, None, None, beh, start, cam, start_frame=1)
    video = skeleton_video(poses, cam, target_size=(64, 64))
    assert video.dtype == torch.uint8 and tuple(video.shape) == (2, 4, 64, 64, 3)
    host = video.cpu().numpy()
    assert (host != 255).any()
    with tempfile.TemporaryDirectory() as d:
        paths = V.save_videos(os.path.join(d, "skeleton_%d.avi"), video, fps=12, quality=95)
        assert [os.path.basename(p) for p in paths] == ["skeleton_0.avi", "skeleton_1.avi"]
        for row, path in enumerate(paths):
            data = open(path, "rb").read()
            assert data[:4] == b"RIFF" and int.from_bytes(data[4:8], "little") == len(data) - 8 and data[8:12] == b"AVI "
            fps, streams = V.read_mjpeg(path)            # (raises where chunk sizes or the index disagree with the file)
            assert fps == 12.0 and len(streams) == 4
            assert streams == [E.encode(host[row, t], 95, "4:2:0") for t in range(4)], row


def test_each_route_issues_its_library_calls_in_order(monkeypatch):
    """I: the library calls of a call, by name and in order, for two images of different size and sampling in one stack: one
    ``encode_info`` per image, one ``quant_tables`` per distinct quality and the two launches on every route; behind them nothing
    on the host route, the device coder's four calls on the other, with the histogram in place of the fixed code words under
    ``optimize``."""
    from behavior_driven_video_synthesis_amd import jpeg_encode as J
    J.clear_buffers()
    g = np.random.default_rng(11)
    frames = torch.from_numpy(g.integers(0, 256, size=(2, 17, 23, 3), dtype=np.uint8)).cuda()
    kw = dict(sizes=[(16, 16), (17, 23)], subsampling=["4:2:0", "4:4:4"])
    seen, real = [], J._call

    def recorded(name, *args):
        seen.append(name.replace("vunet_jpeg_", ""))
        real(name, *args)
    monkeypatch.setattr(J, "_call", recorded)
    head = ["encode_info", "encode_info", "quant_tables", "from_rgb", "fdct"]
    tails = {("host", False): [], ("host", True): [], ("device", False): ["code_words", "huff_lengths", "huff_pack", "huff_stuff"],
             ("device", True): ["huff_count", "huff_lengths", "huff_pack", "huff_stuff"]}
    got = {}
    for (entropy, optimize), tail in tails.items():
        del seen[:]
        got[entropy, optimize] = J.encode_batch(frames, entropy=entropy, optimize=optimize, **kw)
        assert seen == head + tail, (entropy, optimize)
    assert got["host", False] == got["device", False] and got["host", True] == got["device", True]
    J.clear_buffers()
