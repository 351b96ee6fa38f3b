"""Behaviour transfer and latent interpolation on the GPU: ``vunet_seq_slerp`` (csrc/seq_interp.hip) against the float64
restatement (tests/behavior_interp_ref.py) and the reference's own column of tests/golden/g15_behavior_interp.npz, then
``seq.slerp_codes``, ``render.transfer_video`` and ``render.interpolation_video`` against the roll-outs the reference's
``ResidualBehaviorNet`` wrote into the same fixture.

The slerp bound.  The kernel keeps the sums, the angle and the coefficients in float64 and rounds an element once, at its
store: with U = 2^-24 that rounding is at most U |c_lo low + c_hi high| <= U (|c_lo low| + |c_hi high|), and the bound is twice
that, elementwise -- the second half for the float64 differences between the device's and the host's acos / sin and summation
order, which are orders of magnitude below it."""
import copy

import numpy as np
import pytest
import torch

import behavior_interp_ref as R
from conftest import load_golden
from synth import seeded_randn, synth_behavior_state, synth_image, synth_state_dict
from test_hip_seq import TOL        # what generate_seq is held to against the reference's g9 roll-outs

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BARE_H = [1, 3, 64, 130, 1024]


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


@pytest.fixture(scope="module")
def g15():
    return load_golden("g15_behavior_interp")


def _raw(b1, b2, ld, pairs, h, steps, out=None):
    """The C entry point itself (``seq.slerp_codes`` always hands it dense rows)."""
    from behavior_driven_video_synthesis_amd import ops
    st = torch.as_tensor(np.asarray(steps, dtype=np.float64)).cuda()
    if out is None:
        out = torch.full((2, pairs, len(steps), h), float("nan"), device="cuda")
    rc = getattr(ops._lib.lib(), "vunet_seq_slerp")(ops._p(b1), ops._p(b2), ld, pairs, h, ops._p(st), len(steps), ops._p(out),
                                                     ops._stream())
    torch.cuda.synchronize()
    return rc, out


def _held(got, b1, b2, steps, name, extra=0.0, ref=None):
    """|got - ref| <= 2 U (|c_lo low| + |c_hi high|) (+ ``extra``) for every element; prints the figure."""
    want, mag = R.slerp_codes(b1, b2, steps)
    ref = want if ref is None else np.asarray(ref, dtype=np.float64)
    got = got.detach().cpu().numpy().astype(np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    bound = 2 * U * mag + extra
    err = np.abs(got - ref)
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    print(f"{name}: max |got - ref| = {float(err.max()):.3e}, worst = {worst:.3f} of the bound")
    assert np.isfinite(got).all() and worst <= 1.0, (name, worst)


def _codes(tag, pairs, h, seed=15):
    return seeded_randn(f"{tag}.b1", (pairs, h), seed), seeded_randn(f"{tag}.b2", (pairs, h), seed)


# ---- 1. the kernel
@pytest.mark.parametrize("h", BARE_H)
def test_slerp_vs_the_restatement_and_the_reference_column(g15, h):
    """Every bare case of the fixture (Gaussian, near-parallel, identical pairs): against the float64 restatement within the
    bound, against the reference's float32-path column within twice the recorded gap between the two columns plus the bound."""
    from behavior_driven_video_synthesis_amd.seq import slerp_codes
    meta, arr = g15
    b1, b2, steps = arr[f"bare{h}.b1"], arr[f"bare{h}.b2"], np.asarray(meta["steps"])
    got = slerp_codes(torch.from_numpy(b1).cuda(), torch.from_numpy(b2).cuda(), steps)
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 3, 6, h)
    _held(got, b1, b2, steps, f"H = {h} vs float64")
    scale = max(float(np.abs(b1).max()), float(np.abs(b2).max()))
    _held(got, b1, b2, steps, f"H = {h} vs the reference column", extra=2 * meta["f64_gap"][str(h)] * scale, ref=arr[f"bare{h}.ref"])
    again = slerp_codes(torch.from_numpy(b1).cuda(), torch.from_numpy(b2).cuda())          # the default steps are these
    assert torch.equal(got, again)


@pytest.mark.parametrize("pairs,h,ld,steps", [
    (1, 64, 64, [0.3]), (3, 64, 68, [0.0, 1.0]), (3, 64, 65, np.linspace(0, 1, 6)), (65, 130, 131, [0.0, 0.1, 0.9, 1.0]),
    (3, 1024, 1024, np.linspace(0, 1, 64)), (65, 7, 7, np.linspace(-0.25, 1.25, 5)), (1, 1028, 1032, [0.0, 0.1, 0.3, 1.0]),
    (3, 1, 5, np.linspace(0, 1, 6))])
def test_slerp_shapes_pitches_and_step_counts(pairs, h, ld, steps):
    """Rows ``ld_in`` > h apart (aligned and unaligned pitches: vector and plain loads), 1 / 2 / 6 / 64 steps, [0, 0.1, 0.9, 1] and
    steps that are not symmetric about 1 / 2 (direction 1 is computed, not mirrored: the restatement it is held to evaluates
    slerp(v, b2, b1) itself), steps outside [0, 1], 1 / 3 / 65 pairs, widths on and off the 16-byte store path
    and beyond one pass of the workgroup; nothing is written outside the output; two launches give the same bits."""
    b1, b2 = _codes(f"shape{pairs}x{h}", pairs, h)
    if h == 1:
        b2 = b2.abs() * b1.sign()        # (two rows of width 1 are parallel or antiparallel; the latter is ill-conditioned)
    buf1, buf2 = torch.full((pairs, ld), 7.0), torch.full((pairs, ld), -7.0)
    buf1[:, :h], buf2[:, :h] = b1, b2
    guard = 64
    flat = torch.full((2 * pairs * len(steps) * h + 2 * guard,), 123.0, device="cuda")
    out = flat[guard:-guard].view(2, pairs, len(steps), h)
    rc, got = _raw(buf1.cuda(), buf2.cuda(), ld, pairs, h, steps, out=out)
    assert rc == 0
    assert bool((flat[:guard] == 123.0).all()) and bool((flat[-guard:] == 123.0).all())
    _held(got, b1.numpy(), b2.numpy(), steps, f"{pairs} pairs x {h} (pitch {ld}), {len(steps)} steps")
    rc2, got2 = _raw(buf1.cuda(), buf2.cuda(), ld, pairs, h, steps)
    assert rc2 == 0 and torch.equal(got, got2)


def test_slerp_end_points_return_the_codes_within_the_bound():
    """steps 0 and 1: low and high.  sin(omega) / sin(omega) is 1 and sin(0 omega) is 0, but the blend is still a float64 result
    rounded once: the bound is asserted, not bit equality."""
    from behavior_driven_video_synthesis_amd.seq import slerp_codes
    b1, b2 = _codes("ends", 5, 130)
    got = slerp_codes(b1.cuda(), b2.cuda(), [0.0, 1.0]).cpu().numpy().astype(np.float64)
    lo, hi = b1.numpy().astype(np.float64), b2.numpy().astype(np.float64)
    for name, g, want in (("0 -> low", got[0, :, 0], lo), ("0 -> high", got[0, :, 1], hi), ("1 -> low", got[1, :, 0], hi),
                          ("1 -> high", got[1, :, 1], lo)):
        worst = float(np.max(np.abs(g - want) / (2 * U * np.abs(want))))
        print(f"end point {name}: worst = {worst:.3f} of the bound")
        assert worst <= 1.0, name


def test_slerp_of_a_zero_row_is_nan_and_bad_arguments_are_refused():
    """A row of zeros has no direction: NaN rows as numpy gives, for that pair only, and no fault.  The library's argument
    code for what it cannot run."""
    from behavior_driven_video_synthesis_amd.seq import slerp_codes
    b1, b2 = _codes("zero", 3, 64)
    b1[1] = 0.0
    got = slerp_codes(b1.cuda(), b2.cuda(), [0.0, 0.5, 1.0])
    assert bool(torch.isnan(got[:, 1]).all()) and bool(torch.isfinite(got[:, 0]).all()) and bool(torch.isfinite(got[:, 2]).all())
    x, y = b1.cuda(), b2.cuda()
    assert _raw(x, y, 64, 3, 64, np.linspace(0, 1, 65))[0] == -1
    assert _raw(x, y, 63, 3, 64, [0.5])[0] == -1
    assert _raw(x, y, 64, 0, 64, [0.5])[0] == -1
    assert _raw(x, y, 64, 3, 0, [0.5])[0] == -1
    assert _raw(None, y, 64, 3, 64, [0.5])[0] == -1


def test_slerp_codes_refuses_what_it_cannot_run():
    from behavior_driven_video_synthesis_amd.seq import slerp_codes
    b1, b2 = _codes("refuse", 2, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        slerp_codes(b1, b2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        slerp_codes(b1.cuda(), b2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        slerp_codes(b1.cuda().double(), b2.cuda().double())
    with pytest.raises(ValueError, match="one shape"):
        slerp_codes(b1.cuda(), b2[:1].cuda())
    with pytest.raises(ValueError, match="one shape"):
        slerp_codes(b1.cuda(), b2[:, :32].cuda())
    with pytest.raises(ValueError, match="one shape"):
        slerp_codes(b1[0].cuda(), b2[0].cuda())
    with pytest.raises(ValueError, match="steps"):
        slerp_codes(b1.cuda(), b2.cuda(), np.linspace(0, 1, 65))
    with pytest.raises(ValueError, match="steps"):
        slerp_codes(b1.cuda(), b2.cuda(), [])
    assert tuple(slerp_codes(b1.cuda(), b2.cuda(), np.linspace(0, 1, 64)).shape) == (2, 2, 64, 64)


# ---- 2. the two calls on the fixture's net, poses only
def _g15_net(meta, arr):
    from behavior_driven_video_synthesis_amd.models.pose_behavior_rnn import ResidualBehaviorNet
    net = ResidualBehaviorNet(**meta["net_kw"])
    net.load_state_dict({k[len("net.sd."):]: torch.from_numpy(v) for k, v in arr.items() if k.startswith("net.sd.")})   # strict
    return net.cuda().eval()


def _camera(spatial=64, n=51):
    """A plausible standing figure: joints around the origin +- 600 mm, the camera 5 m away (tests/test_hip_seq.py)."""
    from behavior_driven_video_synthesis_amd.render import PoseCamera
    rng = np.random.RandomState(5)
    mean = (rng.randn(n) * 250.0).astype(np.float32)
    std = (40.0 + 40.0 * rng.rand(n)).astype(np.float32)
    ext = np.concatenate([np.eye(3), np.array([[0.0], [0.0], [5000.0]])], axis=1)
    return PoseCamera(mean, std, list(range(n)), ext, (1145.0, 500.0, 1145.0, 500.0), (1000, 1000), spatial)


def _close(a, b):
    np.testing.assert_allclose(a.detach().cpu().numpy(), np.asarray(b), **TOL)


def test_interpolation_video_poses_vs_the_reference_roll_outs(g15):
    from behavior_driven_video_synthesis_amd.render import interpolation_video
    meta, arr = g15
    net, cam = _g15_net(meta, arr), _camera()
    d1, d2 = torch.from_numpy(arr["pair.data1"]).cuda(), torch.from_numpy(arr["pair.data2"]).cuda()
    pairs, t, n, hid = meta["pairs"], meta["t"], meta["net_kw"]["n_kps"], meta["net_kw"]["dim_hidden_b"]
    frames, poses, kps, codes = interpolation_video(net, None, None, d1, d2, cam)
    assert frames is None
    assert tuple(poses.shape) == (2, pairs, 6, t + 1, n) and tuple(kps.shape) == (2, pairs, 6, t + 1, 17, 2)
    assert tuple(codes.shape) == (2, pairs, 6, hid) and poses.dtype == kps.dtype == codes.dtype == torch.float32
    _close(codes, arr["pair.slerp"])
    _close(poses[..., 1:, :], arr["pair.rollouts"])
    assert torch.equal(poses[0, :, :, 0], d1[:, :1].expand(-1, 6, -1)) and torch.equal(poses[1, :, :, 0], d2[:, :1].expand(-1, 6, -1))
    assert torch.equal(kps, cam.project(poses.reshape(-1, n)).reshape(kps.shape))
    # the end points of the walk are the two posterior means, in either direction
    mu = net.engine().infer_b(torch.cat([d1, d2]), None)[1]
    mu1, mu2 = mu[:pairs], mu[pairs:]
    _close(mu1, arr["pair.mu1"])
    _close(mu2, arr["pair.mu2"])
    _held(codes, mu1.cpu().numpy(), mu2.cpu().numpy(), np.asarray(meta["steps"]), "codes of the net's pairs")


@pytest.mark.parametrize("graph", [False, True])
def test_the_batched_roll_out_equals_row_by_row_calls(g15, graph, monkeypatch):
    """One roll-out over the 2 P S codes against one ``generate_seq`` call per code as the reference issues them (batch 1, the
    whole start sequence handed in), bit for bit, with the graph replay on and off (``VUNET_SEQ_GRAPH``)."""
    from behavior_driven_video_synthesis_amd.render import interpolation_video
    monkeypatch.setenv("VUNET_SEQ_GRAPH", "1" if graph else "0")
    meta, arr = g15
    net, cam = _g15_net(meta, arr), _camera()
    assert net.engine().graph.enabled == graph
    d1, d2 = torch.from_numpy(arr["pair.data1"]).cuda(), torch.from_numpy(arr["pair.data2"]).cuda()
    steps = [0.0, 0.1, 0.9, 1.0]
    for _ in range(2):                                           # second call: the replayed recording
        _, poses, _, codes = interpolation_video(net, None, None, d1, d2, cam, steps=steps)
    for d, data in enumerate((d1, d2)):
        for p in range(meta["pairs"]):
            for s in range(len(steps)):
                xs, *_ = net.generate_seq(codes[d, p, s].unsqueeze(0), data[p:p + 1], len=meta["t"], start_frame=0)
                assert torch.equal(xs[0], poses[d, p, s, 1:]), (d, p, s)


def test_transfer_video_poses_vs_the_reference_roll_outs(g15):
    from behavior_driven_video_synthesis_amd.render import transfer_video
    meta, arr = g15
    net, cam = _g15_net(meta, arr), _camera()
    d1, d2 = torch.from_numpy(arr["pair.data1"]).cuda(), torch.from_numpy(arr["pair.data2"]).cuda()
    pairs, t, n = meta["pairs"], meta["t"], meta["net_kw"]["n_kps"]
    for sf in meta["start_frames"]:
        for name, (beh, start) in {"x1_mu2": (d2, d1), "x2_mu1": (d1, d2)}.items():
            frames, poses, kps = transfer_video(net, None, None, beh, start, cam, start_frame=sf)
            assert frames is None and tuple(poses.shape) == (pairs, t + 1, n) and tuple(kps.shape) == (pairs, t + 1, 17, 2)
            _close(poses[:, 1:], arr[f"xfer.{name}.s{sf}"])
            assert torch.equal(poses[:, 0], start[:, sf])
            assert torch.equal(kps, cam.project(poses.reshape(-1, n)).reshape(kps.shape))
    # the posterior sample instead of the mean, with the noise the fixture recorded; a shorter roll-out; a negative start frame
    _, poses, _ = transfer_video(net, None, None, d2, d1, cam, sample=True, eps=torch.from_numpy(arr["pair.eps2"]).cuda())
    _close(poses[:, 1:], arr["xfer.x1_b2.s0"])
    _, short, _ = transfer_video(net, None, None, d2, d1, cam, start_frame=3, length=2)
    assert tuple(short.shape) == (pairs, 3, n)
    _close(short[:, 1:], arr["xfer.x1_mu2.s3"][:, :2])
    _, neg, _ = transfer_video(net, None, None, d2, d1, cam, start_frame=3 - t)
    _, pos, _ = transfer_video(net, None, None, d2, d1, cam, start_frame=3)
    assert torch.equal(neg, pos)
    drawn = transfer_video(net, None, None, d2, d1, cam, sample=True)[1]
    assert bool(torch.isfinite(drawn).all()) and not torch.equal(drawn, pos)
    with pytest.raises(ValueError, match="one"):
        transfer_video(net, None, None, d2[:1], d1, cam)


# ---- 3. with a synthesis model
def _small_vunet(seed):
    """The smallest model and spatial size tests/test_hip_render.py renders with."""
    from behavior_driven_video_synthesis_amd.models.vunets import VunetAlter
    cfg = dict(spatial_size=64, bottleneck_factor=2, box_factor=2, n_scales=0, n_latent_scales=2, conv_layer_type="l1", nf_start=8,
               nf_max=16, subpixel_upsampling=True, dropout_prob=0.0)
    vunet = VunetAlter(**cfg)
    vunet.load_state_dict(synth_state_dict({k: list(v.shape) for k, v in vunet.state_dict().items()}, seed))
    return vunet.cuda().eval()


def _small_net(n, seed):
    from behavior_driven_video_synthesis_amd.models.pose_behavior_rnn import ResidualBehaviorNet
    net = ResidualBehaviorNet(n, information_bottleneck=True, decoder_arch="lstm", linear_in_decoder=False, dim_hidden_b=64)
    sd = synth_behavior_state({k: list(v.shape) for k, v in net.state_dict().items()}, seed, {})
    sd["decoder.n_out.weight"] = sd["decoder.n_out.weight"] * 0.05      # small steps: the figure stays in the image
    net.load_state_dict(sd)
    return net.cuda().eval()


def _by_hand(vunet, app, cam, poses, **kw):
    """``camera.project`` + ``render_sequence`` on the returned poses, row after row, with the keyword tail the two calls default
    to (``render_sequence``'s own defaults are fp32 and one appearance encoding per frame)."""
    from behavior_driven_video_synthesis_amd.render import render_sequence
    kw = dict(dict(dtype="bf16", share_appearance=True), **kw)
    rows = poses.reshape(-1, poses.shape[-2], poses.shape[-1])
    out = [render_sequence(vunet, app, cam.project(r), spatial_size=cam.spatial_size, **kw)[0] for r in rows]
    return torch.stack(out).reshape(*poses.shape[:-2], *out[0].shape)


@pytest.mark.parametrize("kw", [dict(dtype="f32", share_appearance=False), dict()])
def test_frames_equal_projection_and_render_sequence_by_hand(kw):
    """Both calls with a small VUnet, in fp32 with one appearance encoding per frame and with the default keyword tail (bf16,
    one encoding per sequence): shapes and dtypes as documented, frames bit-identical to the pieces called by hand (the
    synthesis draws its latent noise from torch's generator, seeded the same before either)."""
    from behavior_driven_video_synthesis_amd.render import interpolation_video, transfer_video
    net, vunet, cam = _small_net(51, 23), _small_vunet(23), _camera()
    app = synth_image("interp.app", (1, 3, 64, 64), 23).cuda()
    s1, s2 = (0.5 * seeded_randn("interp.s1", (1, 3, 51), 23)).cuda(), (0.5 * seeded_randn("interp.s2", (1, 3, 51), 23)).cuda()
    torch.manual_seed(5)
    frames, poses, kps, codes = interpolation_video(net, vunet, app, s1, s2, cam, steps=[0.0, 0.6], **kw)
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (2, 1, 2, 4, 64, 64, 3)
    assert tuple(poses.shape) == (2, 1, 2, 4, 51) and tuple(kps.shape) == (2, 1, 2, 4, 17, 2) and tuple(codes.shape) == (2, 1, 2, 64)
    torch.manual_seed(5)
    assert torch.equal(frames, _by_hand(vunet, app, cam, poses, **kw))
    assert float(frames.float().std()) > 0 and float(kps.min()) > -64 and float(kps.max()) < 128
    beh, start = (0.5 * seeded_randn("xfer.beh", (2, 3, 51), 23)).cuda(), (0.5 * seeded_randn("xfer.start", (2, 5, 51), 23)).cuda()
    torch.manual_seed(6)
    frames, poses, kps = transfer_video(net, vunet, app, beh, start, cam, start_frame=4, length=2, **kw)
    assert frames.dtype == torch.uint8 and tuple(frames.shape) == (2, 3, 64, 64, 3)
    assert tuple(poses.shape) == (2, 3, 51) and tuple(kps.shape) == (2, 3, 17, 2)
    torch.manual_seed(6)
    assert torch.equal(frames, _by_hand(vunet, app, cam, poses, **kw))
    assert transfer_video(net, vunet, None, beh, start, cam)[0] is None          # no appearance image: poses only


def test_both_calls_with_an_angle_camera():
    """A model trained on ``angle_world_expmap`` poses (54 dimensions): ``AnglePoseCamera`` over the g12 tree takes the place of
    ``PoseCamera`` -- both expose ``project`` -- and the same path runs."""
    from behavior_driven_video_synthesis_amd.render import AnglePoseCamera, interpolation_video, transfer_video
    meta, arr = load_golden("g12_pose_angles")
    tree = {"parent": arr["tree.parent"], "offset": arr["tree.offset"], "expmapInd": list(arr["tree.expmapInd"]),
            "posInd": {"ids": arr["tree.posInd"]}}
    ang = 0.4
    rot = np.array([[np.cos(ang), 0.0, np.sin(ang)], [0.0, 1.0, 0.0], [-np.sin(ang), 0.0, np.cos(ang)]])
    ext = np.concatenate([rot, np.array([[50.0], [-120.0], [5200.0]])], axis=1)
    use = [d for d in range(99) if d not in set(meta["ignore"])]
    cam = AnglePoseCamera(arr["stats.mean"], arr["stats.std"], use, tree, ext, (1145.0, 512.5, 1143.8, 515.4), (1000, 1000), 64)
    net, vunet = _small_net(54, 29), _small_vunet(29)
    app = synth_image("angle.app", (1, 3, 64, 64), 29).cuda()
    s1, s2 = (0.5 * seeded_randn("angle.s1", (1, 3, 54), 29)).cuda(), (0.5 * seeded_randn("angle.s2", (1, 3, 54), 29)).cuda()
    kw = dict(dtype="f32", share_appearance=False)
    torch.manual_seed(7)
    frames, poses, kps, codes = interpolation_video(net, vunet, app, s1, s2, cam, steps=[0.25], **kw)
    assert tuple(frames.shape) == (2, 1, 1, 4, 64, 64, 3) and tuple(kps.shape) == (2, 1, 1, 4, 32, 2)
    assert torch.equal(kps, cam.project(poses.reshape(-1, 54)).reshape(kps.shape))
    torch.manual_seed(7)
    assert torch.equal(frames, _by_hand(vunet, app, cam, poses, **kw))
    frames, poses, kps = transfer_video(net, vunet, app, s2, s1, cam, **kw)
    assert tuple(frames.shape) == (1, 4, 64, 64, 3) and tuple(poses.shape) == (1, 4, 54) and tuple(kps.shape) == (1, 4, 32, 2)
    assert bool(torch.isfinite(kps).all()) and float(frames.float().std()) > 0


# ---- 4. eval -> train -> eval
def test_transfer_video_after_a_training_step_uses_the_updated_weights():
    """The inference engine caches its weight images; the fused optimiser writes the parameters through a kernel and moves
    their version counters itself (``ops.mark_written``).  After one ``BehaviorNet.train_fn`` step ``transfer_video`` must decode with the new weights: equal to a freshly
    built net holding them, different from before the step."""
    from behavior_driven_video_synthesis_amd.experiments.behavior_net import BehaviorNet, DEFAULT_CONFIG
    from behavior_driven_video_synthesis_amd.models.pose_behavior_rnn import ResidualBehaviorNet
    from behavior_driven_video_synthesis_amd.render import transfer_video
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["architecture"].update(dim_hidden_b=64, n_flows=2, flow_mid_channels_factor=2, flow_hidden_depth=1)
    cfg["training"].update(batch_size=6, lr_init=1e-2, gamma_init=0.05, gamma_step=1e-3, information_max=5, flow_lr=5e-5)
    with torch.enable_grad():
        tr = BehaviorNet(cfg, n_kps=51, device="cuda:0", hip_graph=False)
    tr.net.load_state_dict(synth_behavior_state({k: list(v.shape) for k, v in tr.net.state_dict().items()}, 3, {}))
    cam = _camera()
    beh, start = (0.5 * seeded_randn("ete.beh", (3, 5, 51), 3)).cuda(), (0.5 * seeded_randn("ete.start", (3, 5, 51), 3)).cuda()
    before = transfer_video(tr.net, None, None, beh, start, cam)[1]
    kps, eps = 0.5 * seeded_randn("ete.kps", (6, 6, 51), 3), seeded_randn("ete.eps", (6, 64), 3)
    with torch.enable_grad():
        tr.train_fn({"keypoints": kps.cuda()}, eps=eps.cuda())
    after = transfer_video(tr.net, None, None, beh, start, cam)[1]
    kw = {k: v for k, v in cfg["architecture"].items() if k in ("decoder_arch", "linear_in_decoder", "dim_hidden_b")}
    fresh = ResidualBehaviorNet(n_kps=51, information_bottleneck=True, **kw)
    fresh.load_state_dict({k: v.detach().clone() for k, v in tr.net.state_dict().items()})
    want = transfer_video(fresh.cuda(), None, None, beh, start, cam)[1]
    assert torch.equal(after, want)
    assert not torch.equal(after[:, 1:], before[:, 1:]) and torch.equal(after[:, 0], before[:, 0])
