"""The raw-frame input route on the GPU (csrc/image_input.hip, behavior_driven_video_synthesis_amd/image_input.py) against Pillow's
bytes (tests/golden/g19_image_input.npz) and the integer-exact restatement (tests/image_input_ref.py, itself checked against
Pillow in tests/test_image_input_ref.py): the tables (A), the resized bytes (B), the fp32 images (C), contract-breaking rows (D),
the trainer's wiring, eagerly and from a replayed hipGraph (E), and the SSIM driver (F).

Everything is exact -- Pillow's 8-bit resampler is integer arithmetic on fixed-point coefficients, so there is no tolerance.
Inputs: the fixture's cases (no source larger than 64 x 64: non-integer down- and upscales, a skipped axis, a 1-pixel-high source,
crop windows over every edge, a mixed batch in one stack padded with 0xAB) and one frame of 1000 x 1002 -> 256 (the size the
trainers use: 256 lanes per block, 17 taps, several blocks), compared with the restatement."""
import copy
import functools

import numpy as np
import pytest
import torch

import image_input_ref as R

pytestmark = pytest.mark.gpu

FIX = R.load_fixture()


def _u8(c, **kw):
    from behavior_driven_video_synthesis_amd import image_input as I
    return I.frames_to_images(torch.from_numpy(c["frames"]).cuda(), c["geom"], c["size"], **kw)


@pytest.mark.parametrize("name", list(FIX))
def test_device_tables_equal_the_restatement(name):
    """A: coefficients and bounds of both axes, every image, every output index."""
    from behavior_driven_video_synthesis_amd import image_input as I
    c = FIX[name]
    hmax, wmax, s = c["frames"].shape[1], c["frames"].shape[2], c["size"]
    coef, bounds, status = I.resample_tables(c["geom"], (hmax, wmax), s)
    kmax = R.ksize_max(hmax, wmax, s)
    assert tuple(coef.shape) == (2, len(c["geom"]), s, kmax) and tuple(bounds.shape) == (2, len(c["geom"]), s, 2)
    assert coef.dtype == torch.int32 and bounds.dtype == torch.int32 and not status.cpu().numpy().any()
    coef, bounds = coef.cpu().numpy(), bounds.cpu().numpy()
    for i, row in enumerate(c["geom"]):
        for axis, in_size in ((0, int(row[4])), (1, int(row[5]))):
            b, k = R.tables(in_size, s, kmax)
            assert np.array_equal(bounds[axis, i], b), (name, i, axis)
            assert np.array_equal(coef[axis, i], k), (name, i, axis, int(np.abs(coef[axis, i] - k).max()))


@pytest.mark.parametrize("name", list(FIX))
def test_uint8_output_equals_pillow(name):
    """B: the resized bytes, single images and the mixed batch (whose 0xAB padding must not show)."""
    out, status = _u8(FIX[name], out_u8=True)
    assert out.dtype == torch.uint8 and not status.cpu().numpy().any()
    got = out.cpu().numpy()
    assert np.array_equal(got, FIX[name]["expect"]), int(np.abs(got.astype(int) - FIX[name]["expect"]).max())


@pytest.mark.parametrize("name", list(FIX))
def test_fp32_output_is_the_torch_expression_of_the_bytes(name):
    """C: fp32 NCHW == ToTensor and ``x * 2 - 1`` of (B)'s bytes, bit for bit."""
    out, _ = _u8(FIX[name])
    want = torch.from_numpy(FIX[name]["expect"]).permute(0, 3, 1, 2).float().div(255).mul(2.0).sub(1.0)
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(want.shape)
    assert torch.equal(out.cpu(), want)


def test_whole_frames_device_geometry_and_host_frames():
    """``geom=None`` is the whole stack slot; geometry already on the device and frames still on the host give the same bytes."""
    from behavior_driven_video_synthesis_amd import image_input as I
    c = FIX["down_37x53"]
    a, _ = I.frames_to_images(c["frames"], None, 16, out_u8=True)                              # NumPy frames, uploaded
    b, _ = I.frames_to_images(torch.from_numpy(c["frames"]).cuda(), torch.from_numpy(c["geom"]).cuda(), 16, out_u8=True)
    assert np.array_equal(a.cpu().numpy(), c["expect"]) and torch.equal(a, b)
    with pytest.raises(ValueError):
        I.frames_to_images(c["frames"], torch.zeros(1, 6, dtype=torch.int64).cuda(), 16)


def test_full_size_frame_equals_the_restatement():
    """1000 x 1002 -> 256, the trainers' size, with a window over the top-left corner: the 256-lane blocks and 17-tap rows."""
    from behavior_driven_video_synthesis_amd import image_input as I
    g = np.random.default_rng(11)
    frames = g.integers(0, 256, size=(2, 1000, 1002, 3), dtype=np.uint8)
    geom = np.array([[1000, 1002, 0, 0, 1002, 1000], [1000, 1000, -31, -17, 900, 903]], dtype=np.int32)
    want, _ = R.frames_to_u8(frames, geom, 256)
    out, status = I.frames_to_images(frames, geom, 256, out_u8=True)
    assert not status.cpu().numpy().any()
    assert np.array_equal(out.cpu().numpy(), want)


def test_contract_breaking_rows_are_flagged_and_never_indexed_with():
    """D: ``cw = 0`` and ``ch > Hmax`` (device geometry: the host check is not in the way) give status 1 and all -1.0 (0 as
    bytes); their batch neighbours are Pillow's bytes as before.  Wild offsets on a valid row are reflected, not a fault."""
    from behavior_driven_video_synthesis_amd import image_input as I
    c = FIX["batch"]
    geom = c["geom"].copy()
    geom[2, 4] = 0
    geom[5, 5] = c["frames"].shape[1] + 1
    geom[5, 2:4] = (2 ** 31 - 1, -2 ** 31)
    bad = [2, 5]
    good = [i for i in range(len(geom)) if i not in bad]
    frames, g = torch.from_numpy(c["frames"]).cuda(), torch.from_numpy(geom).cuda()
    u8, status = I.frames_to_images(frames, g, 16, out_u8=True)
    f32, status2 = I.frames_to_images(frames, g, 16)
    assert status.cpu().tolist() == status2.cpu().tolist() == [1 if i in bad else 0 for i in range(len(geom))]
    assert not u8[bad].cpu().numpy().any() and bool((f32[bad] == -1.0).all())
    assert np.array_equal(u8[good].cpu().numpy(), c["expect"][good])
    want = torch.from_numpy(c["expect"][good]).permute(0, 3, 1, 2).float().div(255).mul(2.0).sub(1.0)
    assert torch.equal(f32[good].cpu(), want)
    with pytest.raises(ValueError):
        I.frames_to_images(frames, geom, 16)                        # the same rows as host geometry: refused before any launch
    # offsets at the ends of int32 on a VALID row: reflected (the restatement does the same in 64-bit integers)
    far = c["geom"].copy()
    far[0, 2:4] = (2 ** 31 - 40, -2 ** 31)
    want_far, _ = R.frames_to_u8(c["frames"], far, 16)
    got_far, st = I.frames_to_images(frames, torch.from_numpy(far).cuda(), 16, out_u8=True)
    assert not st.cpu().numpy().any() and np.array_equal(got_far.cpu().numpy(), want_far)


# ---- E, F: wiring ------------------------------------------------------------------------------------------------------------
def _tiny(default, **training):
    """The smallest trainer config of tests/test_hip_training.py: 32^2, nf 8..16, 3-channel appearance input."""
    cfg = copy.deepcopy(default)
    cfg["data"]["spatial_size"] = 32
    cfg["architecture"].update(nf_start=8, nf_max=16)
    cfg["training"].update(training)
    return cfg


@functools.lru_cache(maxsize=None)
def _raw(seed):
    """Two raw frames (50 x 70 and 44 x 61 in one stack) and crop windows over their edges; computed once, never modified."""
    g = np.random.default_rng(seed)
    frames = R.stack([g.integers(0, 256, size=(50, 70, 3), dtype=np.uint8), g.integers(0, 256, size=(44, 61, 3), dtype=np.uint8)], 64, 72)
    geom = np.array([[50, 70, -5, 3, 60, 52], [44, 61, 10, -9, 49, 47]], dtype=np.int32)
    frames.setflags(write=False)
    geom.setflags(write=False)
    return frames, geom


def _batch(seed, raw):
    from behavior_driven_video_synthesis_amd import image_input as I
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import synthetic_batch
    batch = synthetic_batch(2, 32, "cuda:0", seed=seed)
    frames, geom = _raw(seed)
    if raw:
        del batch["pose_img"]
        batch["pose_img_u8"], batch["pose_img_geom"] = torch.from_numpy(frames.copy()), geom.copy()    # host inputs: staged by the trainer
    else:
        batch["pose_img"] = I.frames_to_images(frames.copy(), geom.copy(), 32)[0]
    return batch


def _run(raw, capture, steps):
    from behavior_driven_video_synthesis_amd import ops
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import DEFAULT_CONFIG, ShapePoseNet
    ops.set_dropout_seed(8642)
    cfg = _tiny(DEFAULT_CONFIG, lr=2e-3, n_init_batches=1, gamma_step=1e-3, information_max=5.0, train_regressor=False)
    tr = ShapePoseNet(cfg, device="cuda:0", vgg_width_div=8, total_steps=50, vgg_synthetic=True, hip_graph=False)
    if capture is not None:
        tr.enable_hip_graph(capture=capture)
    outs = []
    for i in range(steps):
        o = tr.train_fn(_batch(500 + i, raw))
        outs.append({k: float(o[k]) for k in ("loss", "likelihood_loss", "kl_loss", "gamma")})
    torch.cuda.synchronize()
    ops.set_dropout_step(None)
    return tr, outs


def _same_state(a, b):
    for (k, p), (_, q) in zip(a.vunet.state_dict().items(), b.vunet.state_dict().items()):
        assert torch.equal(p, q), k
    for x, y in zip(a.optimizer.buckets, b.optimizer.buckets):
        assert torch.equal(x.exp_avg, y.exp_avg) and torch.equal(x.exp_avg_sq, y.exp_avg_sq)


def test_shape_pose_net_trains_from_raw_frames_as_from_ready_images():
    """E: a ShapePoseNet given ``pose_img_u8`` + ``pose_img_geom`` + ``stickman`` takes, bit for bit, the steps of a twin fed the
    ``pose_img`` that ``frames_to_images`` returns."""
    a, oa = _run(True, None, 3)
    b, ob = _run(False, None, 3)
    assert oa == ob, (oa, ob)
    assert all(o["loss"] == o["loss"] for o in oa) and len({o["loss"] for o in oa}) == 3
    _same_state(a, b)


def test_hip_graph_replay_with_the_resize_inside_is_bit_identical_to_eager():
    """E: the step with the three image launches inside, replayed from ONE captured hipGraph (the uint8 stack and the geometry
    two more static inputs, fresh frames every step), against the same device-resident schedule launched eagerly: 7 steps, 4 of
    them replays -- and against the twin fed ready images."""
    a, oa = _run(True, True, 7)
    assert len(a._graphs) == 1
    b, ob = _run(True, False, 7)
    assert not b._graphs
    assert oa == ob, (oa, ob)
    assert len({o["loss"] for o in oa}) == len(oa)
    _same_state(a, b)


def test_compute_ssim_and_vunet_trainer_from_raw_frames():
    """F: ``lib.metrics.compute_ssim`` from ``pose_img_u8`` equals the call fed the fp32 images; so does ``compute_fid``, and
    ``experiments.vunet.Vunet.train_fn``."""
    from behavior_driven_video_synthesis_amd import ops
    from behavior_driven_video_synthesis_amd.experiments import vunet as V
    from behavior_driven_video_synthesis_amd.lib import metrics
    tr, _ = _run(False, None, 1)
    rb, fb = _batch(77, True), _batch(77, False)
    feats = lambda im: im.flatten(1)[:, :4]   # noqa: E731
    gt = np.random.default_rng(0).normal(size=(8, 4))
    torch.manual_seed(3)
    s_r = metrics.compute_ssim(tr.vunet, [rb])
    f_r = metrics.compute_fid(tr.vunet, [rb, rb, rb, rb], feats, gt_features=gt)
    torch.manual_seed(3)
    s_f = metrics.compute_ssim(tr.vunet, [fb])
    f_f = metrics.compute_fid(tr.vunet, [fb, fb, fb, fb], feats, gt_features=gt)
    assert s_r == s_f and f_r == f_f and s_r == s_r

    def run(raw):
        ops.set_dropout_seed(1357)
        cfg = _tiny(V.DEFAULT_CONFIG, dropout_prob=0.0)
        t = V.Vunet(cfg, device="cuda:0", n_channels_x=3, vgg_width_div=8, total_steps=8, vgg_synthetic=True)
        torch.manual_seed(5)
        return t, float(t.train_fn(_batch(41, raw))["loss"])
    (a, la), (b, lb) = run(True), run(False)
    assert la == lb and la == la
    for (k, p), (_, q) in zip(a.vunet.state_dict().items(), b.vunet.state_dict().items()):
        assert torch.equal(p, q), k
