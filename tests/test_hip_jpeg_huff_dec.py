"""The JPEG entropy DEcoder on the GPU (csrc/jpeg_sync.h, csrc/jpeg_huff_dec.hip, ``jpeg_decode.decode_batch(.., entropy="device")``)
against the host route and ``vunet_jpeg_entropy_decode``: g23's streams one at a time (1); all of g24 and g25 in one call (2); scans
that span several workgroups and sync launches (3); the stream that never synchronises (4); a scan that is nearly all stuffing (5);
damaged input, on which both routes must agree (6), and streams with more tables than the device has slots (6b); rows, table rows, offsets and capacities that point outside their buffers (7);
no allocation on a second call, ``out=``, ``tag`` and ``fallback=True`` (8); the hooks (9).

Everything is exact: integers and bytes throughout, so there is no tolerance."""
import copy
import ctypes

import numpy as np
import pytest
import torch

import jpeg_enc_ref as E
import jpeg_opt_ref as O
import jpeg_ref as R
import jpeg_sync_ref as SR

pytestmark = pytest.mark.gpu

G23 = R.load_fixture()
FIX = E.load_fixture()
OPT, _LIMIT = O.load_fixture()


def _decode(streams, **kw):
    from behavior_driven_video_synthesis_amd import jpeg_decode as J
    frames, hw = J.decode_batch(streams, entropy="device", **kw)
    return frames, hw, J.last_stats()


def _host_coef(data):
    """``vunet_jpeg_entropy_decode`` of one stream -> (coef int16 [ncoef], qtab uint16 [ncomp * 64])."""
    from behavior_driven_video_synthesis_amd import _lib, jpeg_decode as J
    info = J._parse_c(data)
    coef, qtab = np.empty(info.ncoef, dtype=np.int16), np.empty(info.ncomp * 64, dtype=np.uint16)
    assert _lib.lib().vunet_jpeg_entropy_decode(data, len(data), ctypes.byref(info), coef.ctypes.data, qtab.ctypes.data) == 0
    return coef, qtab


def _device_coef(J, counts, tag=None):
    """The coefficient buffer the device route has just filled under ``tag``, cut into the images' slots."""
    (buf,) = [b for k, b in J._buffers.items() if k[2] == tag]
    flat = buf.entropy.coef[:sum(counts)].cpu().numpy()
    return np.split(flat, np.cumsum(counts)[:-1])


@pytest.mark.parametrize("name", list(G23["cases"]))
def test_g23_one_image_at_a_time_equals_pillow_and_the_fixtures_coefficients(name):
    """1: the frame is Pillow's, the coefficient buffer and the tables are the fixture's, and nothing went to the host walk."""
    from behavior_driven_video_synthesis_amd import jpeg_decode as J
    J.clear_buffers()
    c = G23["cases"][name]
    frames, hw, stats = _decode([c["data"]])
    h, w = c["rgb"].shape[:2]
    assert hw.tolist() == [[h, w]] and stats["host_fallbacks"] == 0 and stats["subsequences"] >= 1 and stats["rounds"] >= 1
    assert np.array_equal(frames[0].cpu().numpy(), c["rgb"])
    (coef,) = _device_coef(J, [c["coef"].size])
    assert np.array_equal(coef, c["coef"])
    (buf,) = J._buffers.values()
    q = buf.dev[ctypes.sizeof(J.JpegImg):ctypes.sizeof(J.JpegImg) + 2 * c["qtab"].size].cpu().numpy().view(np.uint16)
    assert np.array_equal(q, c["qtab"].reshape(-1))
    J.clear_buffers()


def test_all_of_g24_and_g25_in_one_call_equal_the_host_route():
    """2: 724 streams of mixed sizes, samplings and per-image tables (Annex K's and optimised ones) in ONE call."""
    from behavior_driven_video_synthesis_amd import jpeg_decode as J
    J.clear_buffers()
    streams = [c["data"] for c in FIX.values()] + [OPT[n] for n in FIX]
    assert len(streams) == 2 * len(FIX) >= 700
    want, want_hw = J.decode_batch(streams, tag="host")
    got, hw, stats = _decode(streams, tag="device")
    assert stats["host_fallbacks"] == 0 and torch.equal(hw, want_hw)
    assert torch.equal(got, want)
    J.clear_buffers()


def test_scans_over_several_workgroups_and_sync_launches_equal_the_host_walk():
    """3: the streams of tests/jpeg_sync_ref.py's ``gpu_streams`` -- the noise-ramp 256 x 256 frame at the three samplings, the
    9 x 1100 strip at quality 95, one 1002 x 1000 frame at quality 95 (a scan over 256 KiB: nine workgroups)."""
    from behavior_driven_video_synthesis_amd import jpeg_decode as J, jpeg_encode as JE
    J.clear_buffers()
    streams = SR.gpu_streams(lambda frames, **kw: JE.encode_batch(torch.from_numpy(frames).cuda(), **kw))
    JE.clear_buffers()
    big = streams[-1]
    assert len(big) - big.index(b"\xff\xda") > 256 * 1024
    for batch in (streams[:-1], [big]):
        want, want_hw = J.decode_batch(batch, tag="host")
        got, hw, stats = _decode(batch, tag="device")
        assert stats["host_fallbacks"] == 0 and torch.equal(hw, want_hw) and torch.equal(got, want)
        host = [_host_coef(d)[0] for d in batch]
        for d, a, b in zip(batch, _device_coef(J, [h.size for h in host], "device"), host):
            assert np.array_equal(a, b), len(d)
    assert stats["launches"] >= stats["rounds"] >= 2 and stats["subsequences"] > 8 * J.GROUP
    J.clear_buffers()


def test_the_never_synchronising_stream_stays_within_the_bound():
    """4: a constant (200, 30, 90) frame of 1536 x 1536 at quality 75, 4:2:0 -- every MCU after the first is the same 32 bits, and
    the first shifts the phase, so a guessed state never falls into step -- in one batch with a noise frame."""
    from behavior_driven_video_synthesis_amd import jpeg_decode as J, jpeg_encode as JE
    J.clear_buffers()
    flat = np.empty((1536, 1536, 3), dtype=np.uint8)
    flat[:] = SR.NEVER_RGB
    (never,) = JE.encode_batch(torch.from_numpy(flat).cuda()[None], quality=75, subsampling="4:2:0")
    (noise,) = JE.encode_batch(torch.from_numpy(SR.noise_ramp(256, 256, 256)).cuda()[None], quality=75, subsampling="4:2:0")
    JE.clear_buffers()
    scan = len(never) - never.index(b"\xff\xda") - 16
    groups = -(-(-(-scan // J.SUBSEQ_BYTES)) // J.GROUP)
    assert groups >= 2
    want, _ = J.decode_batch([never, noise], tag="host")
    got, _, stats = _decode([never, noise], tag="device")
    assert torch.equal(got, want) and stats["host_fallbacks"] == 0
    assert 2 <= stats["rounds"] <= groups + 1, stats
    J.clear_buffers()


def test_a_scan_that_is_nearly_all_stuffing_equals_the_host_route():
    """5: 24 x 24 at 4:2:0 with 1023 in every AC position (sixteen 1-bits of code, ten of value per term), written by the host coder."""
    from behavior_driven_video_synthesis_amd import jpeg_decode as J
    J.clear_buffers()
    data = SR.stuffed_stream()
    scan = data[data.index(b"\xff\xda") + 14:-2]
    assert 2 * scan.count(b"\xff\x00") > 0.6 * len(scan)              # (4984 of 7160 bytes are FF 00 pairs)
    want, _ = J.decode_batch([data, data], tag="host")
    got, _, stats = _decode([data, data], tag="device")
    assert torch.equal(got, want) and stats["host_fallbacks"] == 0
    (a, b) = _device_coef(J, [24 * 64] * 2, "device")
    assert np.array_equal(a, _host_coef(data)[0]) and np.array_equal(a, b)
    J.clear_buffers()


def _outcome(J, streams, entropy):
    try:
        frames, hw = J.decode_batch(streams, entropy=entropy, tag=entropy)
    except J.JpegError as e:
        return (type(e), e.code, e.index)
    return (frames.cpu().clone(), hw)


def _same(a, b):
    if isinstance(a[0], type) or isinstance(b[0], type):
        return a == b
    return torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_damaged_input_gives_what_the_host_route_gives():
    """6: same frames, or same exception class, code and index, on truncations, bit flips and a restart marker out of sequence."""
    from behavior_driven_video_synthesis_amd import jpeg_decode as J
    J.clear_buffers()
    name, offsets = G23["truncated"]
    whole = G23["cases"][name]["data"]
    cases = [("cut at %d" % o, whole[:o]) for o in offsets]
    cases += [("flip %d" % i, d) for i, d in enumerate(SR.flipped(FIX["64x64_noise_q75_s420"]["data"], 16))]
    rst = bytearray(G23["cases"]["s444_40x56_rst4_noise"]["data"])
    at = bytes(rst).index(b"\xff\xd2")
    rst[at + 1] = 0xD3
    cases.append(("RST2 -> RST3", bytes(rst)))
    kinds = set()
    for what, data in cases:
        a, b = _outcome(J, [data], "host"), _outcome(J, [data], "device")
        assert _same(a, b), (what, a if isinstance(a[0], type) else "frames", b if isinstance(b[0], type) else "frames")
        kinds.add(a[1] if isinstance(a[0], type) else 0)
    assert len(kinds) >= 3, kinds                             # several error codes, and accepted streams too (code 0)
    # the first bad stream of a batch of three names itself, and the next call is unaffected
    good, bad1, bad2 = FIX["64x64_ramp_q75_s420"]["data"], cases[len(offsets) - 4][1], cases[-1][1]
    for batch in ([good, bad2, bad1], [bad1, good, bad2], [good, good, bad2]):
        a, b = _outcome(J, batch, "host"), _outcome(J, batch, "device")
        assert isinstance(a[0], type) and a == b, (a, b)
    a, b = _outcome(J, [good, whole, good], "host"), _outcome(J, [good, whole, good], "device")
    assert not isinstance(a[0], type) and _same(a, b) and J.last_stats()["host_fallbacks"] == 0
    J.clear_buffers()


def test_a_stream_with_three_dc_tables_goes_to_the_host_walk_alone_and_among_clean_streams():
    """6b: baseline streams that use more Huffman tables than the device has slots (``jpeg_sync_ref.three_tables``): the marker scan
    calls them irregular, the host walk decodes them, and their table rows travel with the batch's through every entry point's
    check.  Alone (no device stage runs), first, last and between clean streams, and two of them: the frames are the host route's."""
    from behavior_driven_video_synthesis_amd import jpeg_decode as J
    J.clear_buffers()
    clean = [G23["cases"][n]["data"] for n in ("s420_50x70_q100_noise", "s444_40x56_rst4_noise", "gray_24x31_noise")]
    odd = [SR.three_tables(G23["cases"][n]["data"]) for n in ("s420_17x23_smooth", "s444_40x56_rst4_noise")]
    for batch, fallbacks in (([odd[0]], 1), ([odd[0], clean[0]], 1), ([clean[0], odd[1], clean[1]], 1), (clean + [odd[0]], 1),
                             ([odd[1], clean[2], odd[0], clean[0]], 2)):
        want, want_hw = J.decode_batch(batch, tag="host")
        got, hw, stats = _decode(batch, tag="device")
        assert torch.equal(got, want) and torch.equal(hw, want_hw), len(batch)
        assert stats["host_fallbacks"] == fallbacks and (stats["subsequences"] > 0) == (len(batch) > fallbacks), (len(batch), stats)
    h, w = G23["cases"]["s420_17x23_smooth"]["rgb"].shape[:2]
    assert np.array_equal(got[2, :h, :w].cpu().numpy(), G23["cases"]["s420_17x23_smooth"]["rgb"])   # (the same image as the fixture's)
    J.clear_buffers()


def test_rows_tables_offsets_and_capacities_outside_their_buffers_are_refused_before_any_launch():
    """7: the entry points by hand on two images, then every argument that would let a kernel index outside a buffer is
    VUNET_ERR_ARG: the outputs carry a sentinel first and are unchanged afterwards, and the good arguments still work."""
    from behavior_driven_video_synthesis_amd import _lib, jpeg_decode as J
    from behavior_driven_video_synthesis_amd.ops import _call, _p, _stream
    lib = _lib.lib()
    names = ["s420_50x70_q100_noise", "s444_40x56_rst4_noise"]
    data = [G23["cases"][n]["data"] for n in names]
    infos = [J._parse_c(d) for d in data]
    scans = [J._scan(lib, d, inf) for d, inf in zip(data, infos)]
    assert all(rc == 0 for rc, _, _ in scans)
    imgs, tabs, qtab = (J.JpegImg * 2)(), np.zeros((2, J.TAB_BYTES), dtype=np.uint8), np.zeros((2, 192), dtype=np.uint16)
    rows, spans, blob = (J.Subseq * (4 * J.GROUP))(), np.zeros((2, 2), dtype=np.int32), bytearray()
    coef_at = block_at = row_at = 0
    for j, (inf, (_, segs, t)) in enumerate(zip(infos, scans)):
        r = imgs[j]
        r.coef_off, r.plane_off, r.q_off, r.block0, r.slot = coef_at, coef_at, 192 * j, block_at, j
        r.height, r.width, r.ncomp, r.hsamp, r.vsamp = inf.height, inf.width, inf.ncomp, inf.hsamp, inf.vsamp
        r.bw0, r.bh0, r.bw1, r.bh1 = inf.bw0, inf.bh0, inf.bw1, inf.bh1
        qtab[j], tabs[j] = t[:384].view(np.uint16), t[384:]
        made = ctypes.c_int64(0)
        assert lib.vunet_jpeg_huffdec_rows(segs.ctypes.data, len(segs), ctypes.byref(inf), j, len(blob) - int(segs[0, 0]), row_at,
                                           ctypes.byref(rows, row_at * ctypes.sizeof(J.Subseq)), 4 * J.GROUP - row_at,
                                           ctypes.byref(made)) == 0
        spans[j] = (row_at, made.value)
        blob += data[j][int(segs[0, 0]):int(segs[-1, 1])]
        coef_at, block_at, row_at = coef_at + inf.ncoef, block_at + inf.nblocks, row_at + made.value
    nsub, nbytes = row_at, len(blob)
    assert nsub == 2 * J.GROUP                                 # (the second image has a row per restart interval: one workgroup each)
    up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()   # noqa: E731
    d_imgs, d_rows, d_tabs, d_spans, d_bytes = up(bytes(imgs)), up(bytes(rows)[:nsub * 40]), up(tabs.tobytes()), up(spans.tobytes()), up(bytes(blob))
    state = torch.full((nsub * J.STATE_WORDS,), -1, dtype=torch.int32, device="cuda")
    counters, flags = torch.full((8,), -1, dtype=torch.int32, device="cuda"), torch.full((2,), -1, dtype=torch.int32, device="cuda")
    coef = torch.full((coef_at,), 0x5A5A, dtype=torch.int16, device="cuda")
    host = lambda o: ctypes.cast(o, ctypes.c_void_p)          # noqa: E731
    a = dict(nbytes=nbytes, nsub=nsub, state=state.numel(), counters=8, first=0, launches=2, flags=2, coef=coef_at, tabs=tabs,
             spans=spans, final=2)

    def sync():
        _call("vunet_jpeg_huffdec_sync", _p(d_bytes), a["nbytes"], _p(d_rows), host(rows), a["nsub"], _p(d_tabs), a["tabs"].ctypes.data,
              host(imgs), 2, _p(state), a["state"], _p(counters), a["counters"], a["first"], a["launches"], _stream())

    def blocks():
        _call("vunet_jpeg_huffdec_blocks", _p(d_rows), host(rows), a["nsub"], _p(d_spans), a["spans"].ctypes.data, host(imgs), 2,
              _p(state), a["state"], _p(flags), a["flags"], _stream())

    def write():
        _call("vunet_jpeg_huffdec_write", _p(d_bytes), a["nbytes"], _p(d_rows), host(rows), a["nsub"], _p(d_tabs), a["tabs"].ctypes.data,
              _p(d_imgs), host(imgs), 2, _p(state), a["state"], a["final"], _p(coef), a["coef"], _p(flags), a["flags"], _stream())

    def dc():
        _call("vunet_jpeg_huffdec_dc", _p(d_imgs), host(imgs), _p(d_tabs), a["tabs"].ctypes.data, 2, _p(coef), a["coef"], _stream())

    def run():
        sync(), blocks(), write(), dc()
        return counters.cpu().numpy().copy(), flags.cpu().numpy().copy(), coef.cpu().numpy().copy()
    c, f, got = run()
    want = np.concatenate([G23["cases"][n]["coef"] for n in names])
    assert c[1] == 0 and (c[2:] == -1).all() and f.tolist() == [0, 0] and np.array_equal(got, want)
    # everything that must be refused; the outputs carry sentinels and are compared afterwards
    def refused(call, what):
        with pytest.raises(RuntimeError, match="vunet_jpeg_huffdec_"):
            call()
            pytest.fail(f"{what}: {call.__name__} was not refused")
    state.fill_(-1), counters.fill_(-1), flags.fill_(-1), coef.fill_(0x5A5A)
    every, walks = [sync, blocks, write], [sync, write]
    row_edits = [(0, "seg_end", nbytes + 1, every), (0, "begin", -1, every), (1, "end", rows[1].end + J.SUBSEQ_BYTES, every),
                 (1, "seg_row", 1, every), (J.GROUP, "img", 0, every), (J.GROUP + 1, "img", 2, every), (3, "flags", 9, every),
                 (J.GROUP, "first_block", infos[1].nblocks, every), (J.GROUP, "seg_blocks", 0, every), (2, "begin", rows[2].begin + 1, every)]
    for i, field, value, calls in row_edits:
        keep = getattr(rows[i], field)
        setattr(rows[i], field, value)
        for call in calls:
            refused(call, (i, field, value))
        setattr(rows[i], field, keep)
    bad_tabs = [tabs.copy() for _ in range(3)]
    tail = J.TAB_BYTES - 40                                    # dc[3], ac[3], per_mcu, hv, restart, reserved
    bad_tabs[0][0, tail:tail + 4] = np.frombuffer(np.int32(4).tobytes(), dtype=np.uint8)          # a table slot that does not exist
    bad_tabs[1][1, tail + 24:tail + 28] = np.frombuffer(np.int32(6).tobytes(), dtype=np.uint8)    # six blocks per MCU at 4:4:4
    bad_tabs[2][0, tail + 20:tail + 24] = np.frombuffer(np.int32(-1).tobytes(), dtype=np.uint8)
    edits = [("nbytes", nbytes - 1, walks), ("nsub", nsub - J.GROUP, [blocks]), ("nsub", nsub + J.GROUP, every), ("nsub", nsub - 1, every),
             ("state", nsub * J.STATE_WORDS - 1, every), ("counters", 1, [sync]), ("first", 7, [sync]), ("launches", 0, [sync]),
             ("flags", 1, [blocks, write]), ("coef", coef_at - 64, [write, dc]), ("final", 0, [write]),
             ("spans", spans + np.array([[0, 0], [J.GROUP, 0]], dtype=np.int32), [blocks]),
             ("spans", spans + np.array([[0, J.GROUP], [0, 0]], dtype=np.int32), [blocks]),
             ("spans", spans[::-1].copy(), [blocks])] + [("tabs", t, [sync, write, dc]) for t in bad_tabs]
    for key, value, calls in edits:
        keep, a[key] = a[key], value
        for call in calls:
            refused(call, (key, value if np.isscalar(value) else "array"))
        a[key] = keep
    imgs[1].coef_off += 64
    for call in (write, dc):                                   # (the stages that take the coefficient buffer)
        refused(call, "coef_off")
    imgs[1].block0 += 1
    for call in (sync, blocks, write, dc):
        refused(call, "block0")
    imgs[1].block0 -= 1
    imgs[1].coef_off -= 64
    torch.cuda.synchronize()
    assert (state == -1).all() and (counters == -1).all() and (flags == -1).all() and (coef == 0x5A5A).all()
    c2, f2, again = run()                                      # ... and the good arguments still work
    assert np.array_equal(c2, c) and f2.tolist() == [0, 0] and np.array_equal(again, want)


def test_second_call_allocates_nothing_and_out_tag_and_fallback_are_honoured():
    """8: every buffer of the device route is reused at a shape -- same addresses, the allocator's live bytes do not move."""
    from behavior_driven_video_synthesis_amd import jpeg_decode as J
    J.clear_buffers()
    first_names = [n for n in FIX if n.endswith("_noise_q75_s420")]
    again_names = [n for n in FIX if n.endswith("_sat_q75_s420")]
    a, b = [FIX[n]["data"] for n in first_names], [FIX[n]["data"] for n in again_names]
    want_a, want_b = (J.decode_batch(s, tag="host")[0].clone() for s in (a, b))
    got_a = _decode(a)[0].clone()
    got_b = _decode(b)[0].clone()
    buf = J._buffers[[k for k in J._buffers if k[2] is None][0]]
    ent = buf.entropy

    def ptrs():
        return [t.data_ptr() for t in (buf.stage, buf.dev, buf.planes, ent.coef, ent.state, ent.small, ent.small_host)]
    before = ptrs()
    torch.cuda.synchronize()
    live = torch.cuda.memory_allocated()
    again_a, _, stats = _decode(a)
    assert torch.equal(again_a, want_a) and torch.equal(got_a, want_a) and torch.equal(got_b, want_b)
    again_b = _decode(b)[0]
    assert torch.equal(again_b, want_b)
    assert ptrs() == before and torch.cuda.memory_allocated() == live and ent.scratch is None and stats["host_fallbacks"] == 0
    assert buf.stage.is_pinned() and ent.small_host.is_pinned()
    # out= is written in place and left alone outside the images; tags keep their own stacks
    out = torch.full((len(a), 260, 270, 3), 0xAB, dtype=torch.uint8, device="cuda")
    frames, hw, _ = _decode(a, hmax=260, wmax=270, out=out)
    assert frames is out
    for i, (h, w) in enumerate(hw.tolist()):
        assert torch.equal(out[i, :h, :w], want_a[i, :h, :w]) and (out[i, h:] == 0xAB).all() and (out[i, :, w:] == 0xAB).all()
    x, y = _decode(a[:3], tag="x")[0], _decode(a[:3], tag="y")[0]
    assert x is not y and x is _decode(a[:3], tag="x")[0] and torch.equal(x, y)
    # a progressive stream in the batch goes to Pillow, its neighbours to the device
    pytest.importorskip("PIL.Image")
    prog = G23["refused"]["progressive"]
    mixed = [a[0], prog, a[1]]
    want, want_hw = J.decode_batch(mixed, fallback=True, tag="host")
    got, hw, stats = _decode(mixed, fallback=True, tag="mixed")
    assert torch.equal(got, want) and torch.equal(hw, want_hw) and stats["host_fallbacks"] == 0 and stats["subsequences"] >= 2
    with pytest.raises(J.JpegUnsupported) as e:
        _decode(mixed)
    assert e.value.index == 1
    with pytest.raises(ValueError, match="entropy"):
        J.decode_batch(a, entropy="gpu")
    J.clear_buffers()


def test_the_hooks_pass_the_keyword_on(tmp_path, monkeypatch):
    """9: ``image_input.decode_jpeg(.., entropy="device")``, a trainer built with ``data.jpeg_entropy: "device"`` and a written
    Motion-JPEG file."""
    from behavior_driven_video_synthesis_amd import image_input as I, jpeg_decode as J, jpeg_encode as JE, video_io as V
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import DEFAULT_CONFIG, ShapePoseNet, synthetic_batch
    J.clear_buffers()
    pair = [G23["cases"][n]["data"] for n in ("s420_17x23_smooth", "s444_40x56_rst4_noise")]
    seen = []
    real = J.decode_batch
    monkeypatch.setattr(J, "decode_batch", lambda *a, **kw: (seen.append(kw.get("entropy")), real(*a, **kw))[1])
    default = I.decode_jpeg({"pose_img_jpeg": pair})
    device = I.decode_jpeg({"pose_img_jpeg": pair}, entropy="device")
    assert seen == ["host", "device"] and J.last_stats()["subsequences"] >= 2 and J.last_stats()["host_fallbacks"] == 0
    want = default["pose_img_u8"].clone()
    assert torch.equal(device["pose_img_u8"], want) and torch.equal(device["pose_img_geom"], default["pose_img_geom"])
    assert torch.equal(I.batch_images({"pose_img_jpeg": pair}, 32, entropy="device")["pose_img"],
                       I.batch_images({"pose_img_u8": want, "pose_img_geom": default["pose_img_geom"]}, 32)["pose_img"])
    staged = {}
    for mode in ("host", "device"):
        cfg = copy.deepcopy(DEFAULT_CONFIG)
        cfg["data"]["spatial_size"] = 32
        cfg["architecture"].update(nf_start=8, nf_max=16)
        if mode == "device":
            cfg["data"]["jpeg_entropy"] = "device"
        tr = ShapePoseNet(cfg, device="cuda:0", vgg_width_div=8, total_steps=50, vgg_synthetic=True, hip_graph=False)
        monkeypatch.setattr(tr, "_train_fn", lambda batch, it, eps, reg_eps, mode=mode: staged.update({mode: batch["pose_img_u8"].clone()}) or {})
        batch = synthetic_batch(2, 32, "cuda:0", seed=5)
        del batch["pose_img"]
        batch["pose_img_jpeg"] = pair
        del seen[:]
        tr.train_fn(batch)
        assert seen == [mode]
    assert torch.equal(staged["host"], staged["device"]) and torch.equal(staged["device"], want)
    monkeypatch.setattr(J, "decode_batch", real)
    names = [f"64x64_{kind}_q75_s420" for kind in E.CONTENTS]
    clip = torch.from_numpy(np.stack([FIX[n]["img"] for n in names])).cuda()
    path = V.write_mjpeg(str(tmp_path / "clip.avi"), clip, fps=12)
    frames, hw, stats = _decode(V.read_mjpeg(path)[1])
    assert hw.tolist() == [[64, 64]] * len(names) and stats["host_fallbacks"] == 0
    assert torch.equal(frames, J.decode_batch([FIX[n]["data"] for n in names], tag="host")[0])
    J.clear_buffers()
    JE.clear_buffers()
