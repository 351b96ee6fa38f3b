"""The random appearance augmentation on the GPU (csrc/appearance_aug.hip, behavior_driven_video_synthesis_amd/appearance_aug.py)
against Pillow's bytes (tests/golden/g22_appearance_aug.npz) and the restatement (tests/appearance_aug_ref.py, itself checked
against Pillow in tests/test_appearance_aug_ref.py): the bytes (A), the fp32 images (B), the chain into the bicubic resize (C),
non-finite matrices (D), device-resident inputs (E), a 256 x 256 frame (F) and the trainers' wiring, eagerly and from a replayed
hipGraph (G).

Everything is exact -- Pillow's bilinear transform is double arithmetic with a truncating store, so there is no tolerance.
Inputs: the fixture's cases (no source larger than 32 x 32: random affines on odd sizes, the identity, large filled regions, a
mixed batch in one stack padded with 0xAB, rotations of reflect-padded frames at 0, +-90, 45 and random angles, a pad larger than
the frame, a 1-pixel-wide frame) and 256 x 256 frames (the trainers' size: 256 lanes per block; the Market form with pad 128;
windows of 512 and 301 columns, more than one block per row), compared with the restatement."""
import copy
import functools

import numpy as np
import pytest
import torch

import appearance_aug_ref as R

pytestmark = pytest.mark.gpu

FIX = R.load_fixture()


def _run_case(c, **kw):
    from behavior_driven_video_synthesis_amd import appearance_aug as A
    return A.affine_images(torch.from_numpy(c["frames"]).cuda(), c["mats"], c["hw"], **{**c["kw"], **kw})


def _f32(u8):
    return torch.from_numpy(np.ascontiguousarray(u8)).permute(0, 3, 1, 2).float().div(255).mul(2.0).sub(1.0)


@pytest.mark.parametrize("name", list(FIX))
def test_uint8_output_equals_pillow(name):
    """A (and C, the chained case): the bytes, single images and batches -- the 0xAB padding of the mixed stack must not show."""
    out, status = _run_case(FIX[name], out_u8=True)
    assert out.dtype == torch.uint8 and status.dtype == torch.int32 and not status.cpu().numpy().any()
    got, want = out.cpu().numpy(), FIX[name]["expect"]
    assert got.shape == want.shape
    assert np.array_equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("name", list(FIX))
def test_fp32_output_is_the_torch_expression_of_the_bytes(name):
    """B (and C): fp32 NCHW == ToTensor and ``x * 2 - 1`` of (A)'s bytes, bit for bit -- written by the kernel itself where the
    window is the output size, by the bicubic route's vertical pass in the chained case."""
    out, _ = _run_case(FIX[name])
    want = _f32(FIX[name]["expect"])
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(want.shape)
    assert torch.equal(out.cpu(), want)


def test_size_equal_to_the_window_is_a_copy():
    """``Resize`` to the window's own size is Pillow's copy: the same bytes, no bicubic launch needed."""
    c = FIX["rotate_32x16"]
    out, _ = _run_case(c, size=16, out_u8=True)
    assert np.array_equal(out.cpu().numpy(), c["expect"])


def test_non_finite_matrices_give_fill_and_status_and_leave_their_neighbours_alone():
    """D: NaN / inf rows (device matrices: the host check is not in the way) are all fill with status 1; the other rows of the
    batch are Pillow's bytes as before."""
    from behavior_driven_video_synthesis_amd import appearance_aug as A
    c = FIX["rotate_24x24"]
    mats = c["mats"].copy()
    mats[1, 2], mats[3, 0], mats[4, 4] = np.nan, np.inf, -np.inf
    bad, good = [1, 3, 4], [0, 2]
    frames, m = torch.from_numpy(c["frames"]).cuda(), torch.from_numpy(mats).cuda()
    kw = {k: v for k, v in c["kw"].items() if k != "size"}
    u8, status = A.affine_images(frames, m, c["hw"], out_u8=True, **kw)
    f32, status2 = A.affine_images(frames, m, c["hw"], **kw)
    assert status.cpu().tolist() == status2.cpu().tolist() == [0, 1, 0, 1, 1]
    assert not u8[bad].cpu().numpy().any() and bool((f32[bad] == -1.0).all())       # fill black
    assert np.array_equal(u8[good].cpu().numpy(), c["expect"][good]) and torch.equal(f32[good].cpu(), _f32(c["expect"][good]))
    with pytest.raises(ValueError):
        A.affine_images(frames, mats, c["hw"], **kw)                                # the same rows as host matrices: refused
    w = FIX["affine_mixed"]                                                          # fill white, finite coefficients that overflow
    mats = w["mats"].copy()
    mats[0, 5], mats[2, :] = np.nan, [1e308, 1e308, -1e308, 1e308, -1e308, 1e308]   # (row 2: inf - inf = NaN inside the kernel)
    kw = {k: v for k, v in w["kw"].items() if k != "size"}
    u8, status = A.affine_images(torch.from_numpy(w["frames"]).cuda(), torch.from_numpy(mats).cuda(), w["hw"], out_u8=True, **kw)
    f32, _ = A.affine_images(torch.from_numpy(w["frames"]).cuda(), torch.from_numpy(mats).cuda(), w["hw"], **kw)
    assert status.cpu().tolist() == [1, 0, 0]
    assert bool((u8[[0, 2]] == 255).all()) and bool((f32[[0, 2]] == 1.0).all())
    assert np.array_equal(u8[1].cpu().numpy(), w["expect"][1])
    # an hw row outside the stack slot (device tensor) is never indexed with either
    hw = torch.tensor([[35, 31], [17, 29], [32, 0]], dtype=torch.int32).cuda()
    u8, status = A.affine_images(torch.from_numpy(w["frames"]).cuda(), w["mats"], hw, out_u8=True, **kw)
    assert status.cpu().tolist() == [1, 0, 1] and bool((u8[[0, 2]] == 255).all()) and np.array_equal(u8[1].cpu().numpy(), w["expect"][1])


def test_device_resident_matrices_and_sizes_give_the_same_bytes():
    """E: ``mats`` / ``hw`` already on the device, frames still on the host; ``hw=None`` is the whole stack slot."""
    from behavior_driven_video_synthesis_amd import appearance_aug as A
    c = FIX["affine_mixed"]
    kw = {k: v for k, v in c["kw"].items() if k != "size"}
    a, _ = A.affine_images(c["frames"], c["mats"], c["hw"], out_u8=True, **kw)      # NumPy everything, uploaded
    b, _ = A.affine_images(torch.from_numpy(c["frames"]).cuda(), torch.from_numpy(c["mats"]).cuda(), torch.from_numpy(c["hw"]).cuda(),
                           out_u8=True, **kw)
    assert np.array_equal(a.cpu().numpy(), c["expect"]) and torch.equal(a, b)
    s = FIX["affine_24x24"]
    d, _ = A.affine_images(s["frames"], s["mats"], None, fill=(255, 255, 255), out_u8=True)   # window and hw: the slot
    assert np.array_equal(d.cpu().numpy(), s["expect"])
    with pytest.raises(ValueError):
        A.affine_images(c["frames"], torch.from_numpy(c["mats"]).float().cuda(), c["hw"])
    with pytest.raises(ValueError):
        A.affine_images(c["frames"], c["mats"], torch.from_numpy(c["hw"]).long().cuda())


def test_full_size_frames_equal_the_restatement():
    """F: 256 x 256, the trainers' size (256-lane blocks, a block row per output row), in the DeepFashion form -- drawn by
    ``AppearanceAug`` -- and in the Market form (pad 128, centre crop 128); then windows wider than one block: the whole 512 x 512
    padded image (two blocks per row, the rotated corners reach over the reflected border into the fill) and a 37 x 301 one."""
    from behavior_driven_video_synthesis_amd import appearance_aug as A
    frames = np.random.default_rng(12).integers(0, 256, size=(2, 256, 256, 3), dtype=np.uint8)
    hw = np.array([[256, 256], [256, 256]], dtype=np.int32)
    aug = A.AppearanceAug("deepfashion", seed=3)
    mats, args = aug.draw(hw), aug.launch_args(256)
    want, _ = R.affine_stack(frames, hw, mats, **args)
    out, status = A.affine_images(frames, mats, hw, size=256, out_u8=True, **args)
    assert not status.cpu().numpy().any() and np.array_equal(out.cpu().numpy(), want)
    aug = A.AppearanceAug("market", seed=3, size=256)
    mats, args = aug.draw(hw), aug.launch_args(256, (256, 256))
    assert args["pad"] == 128 and args["origin"] == (192, 192)
    want, _ = R.affine_stack(frames, hw, mats, **args)
    out, status = A.affine_images(frames, mats, hw, out_u8=True, **args)
    assert not status.cpu().numpy().any() and np.array_equal(out.cpu().numpy(), want)
    # the whole rotated 512 x 512 padded image of one frame: two 256-lane blocks per output row
    want, _ = R.affine_stack(frames[:1], hw[:1], mats[:1], pad=128)
    out, status = A.affine_images(frames[:1], mats[:1], hw[:1], pad=128, out_u8=True)
    assert tuple(out.shape) == (1, 512, 512, 3) and not status.cpu().numpy().any() and np.array_equal(out.cpu().numpy(), want)
    # a 37 x 301 window of it at an odd origin: the second block of a row is partly outside the window
    kw = dict(pad=128, origin=(101, 229), out_hw=(37, 301), fill=(9, 8, 7))
    want, _ = R.affine_stack(frames, hw, mats, **kw)
    assert np.array_equal(want[0], out.cpu().numpy()[0, 229:266, 101:402])       # (fill does not show inside the padded image)
    out, _ = A.affine_images(frames, mats, hw, out_u8=True, **kw)
    assert np.array_equal(out.cpu().numpy(), want)


# ---- G: wiring ---------------------------------------------------------------------------------------------------------------
def _tiny(default, aug, **training):
    """The smallest trainer config of tests/test_hip_image_input.py: 32^2, nf 8..16, 3-channel appearance input."""
    cfg = copy.deepcopy(default)
    cfg["data"].update(spatial_size=32, appearance_aug=aug, appearance_aug_crop=16)
    cfg["architecture"].update(nf_start=8, nf_max=16)
    cfg["training"].update(training)
    return cfg


@functools.lru_cache(maxsize=None)
def _raw(kind, seed):
    """Two raw frames, this step's matrices and the host-made ``pose_img_inplane`` (the restatement's bytes through ToTensor and
    ``x * 2 - 1``); computed once per (kind, seed), never modified.  DeepFashion form: 32 x 32 frames, the window is the frame.
    Market form: 32 x 16 frames, pad 16, centre crop 16, Resize(32) -- the chain into the bicubic route."""
    from behavior_driven_video_synthesis_amd import appearance_aug as A
    h, w = (32, 32) if kind == "deepfashion" else (32, 16)
    frames = np.random.default_rng(seed).integers(0, 256, size=(2, h, w, 3), dtype=np.uint8)
    hw = np.array([[h, w]] * 2, dtype=np.int32)
    aug = A.AppearanceAug(kind, seed=seed, crop=16, size=32)
    mats = aug.draw(hw)
    want, _ = R.affine_stack(frames, hw, mats, size=32, **aug.launch_args(32, (h, w)))
    ready = torch.from_numpy(R.to_float(want))
    assert tuple(ready.shape) == (2, 3, 32, 32)
    for a in (frames, mats):
        a.setflags(write=False)
    return frames, mats, ready


def _batch(kind, seed, raw):
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import synthetic_batch
    batch = synthetic_batch(2, 32, "cuda:0", seed=seed)
    frames, mats, ready = _raw(kind, seed)
    if raw:
        batch["pose_img_u8"], batch["pose_img_aug"] = torch.from_numpy(frames.copy()), mats.copy()   # host inputs: staged by the trainer
    else:
        batch["pose_img_inplane"] = ready.clone().cuda()
    return batch


def _run(raw, capture, steps, kind="deepfashion"):
    from behavior_driven_video_synthesis_amd import ops
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import DEFAULT_CONFIG, ShapePoseNet
    ops.set_dropout_seed(8642)
    cfg = _tiny(DEFAULT_CONFIG, kind, lr=2e-3, n_init_batches=1, gamma_step=1e-3, information_max=5.0, train_regressor=False)
    tr = ShapePoseNet(cfg, device="cuda:0", vgg_width_div=8, total_steps=50, vgg_synthetic=True, hip_graph=False)
    if capture is not None:
        tr.enable_hip_graph(capture=capture)
    outs = []
    for i in range(steps):
        o = tr.train_fn(_batch(kind, 700 + i, raw))
        outs.append({k: float(o[k]) for k in ("loss", "likelihood_loss", "kl_loss", "gamma")})
    torch.cuda.synchronize()
    ops.set_dropout_step(None)
    return tr, outs


def _same_state(a, b):
    for (k, p), (_, q) in zip(a.vunet.state_dict().items(), b.vunet.state_dict().items()):
        assert torch.equal(p, q), k


def test_shape_pose_net_augments_on_the_gpu_as_from_host_made_images():
    """G: a ShapePoseNet given ``pose_img_u8`` + ``pose_img_aug`` takes, bit for bit, the steps of a twin fed the host-made
    ``pose_img_inplane``."""
    a, oa = _run(True, None, 3)
    b, ob = _run(False, None, 3)
    assert oa == ob, (oa, ob)
    assert all(o["loss"] == o["loss"] for o in oa) and len({o["loss"] for o in oa}) == 3
    _same_state(a, b)


@pytest.mark.parametrize("kind", ["deepfashion", "market"])
def test_hip_graph_replay_with_the_augmentation_inside_follows_new_matrices(kind):
    """G: the step with the augmentation launch inside -- and, in the Market form, the bicubic route's three launches after it --
    replayed from ONE captured hipGraph (the uint8 stack and the matrices two more static inputs; fresh frames and fresh matrices
    every step), against the twin fed each step's host-made image: 7 steps, several of them replays, every one bit-identical --
    so each replay followed its new matrices."""
    a, oa = _run(True, True, 7, kind)
    assert len(a._graphs) == 1
    b, ob = _run(False, True, 7, kind)
    assert oa == ob, (oa, ob)
    assert len({o["loss"] for o in oa}) == len(oa)
    _same_state(a, b)


def test_vunet_trainer_augments_through_the_resize_chain():
    """G: ``experiments.vunet.Vunet.train_fn`` in the Market form -- the bilinear bytes, then the bicubic route's launches --
    against the twin fed the host-made image."""
    from behavior_driven_video_synthesis_amd import ops
    from behavior_driven_video_synthesis_amd.experiments import vunet as V

    def run(raw):
        ops.set_dropout_seed(1357)
        cfg = _tiny(V.DEFAULT_CONFIG, "market", dropout_prob=0.0)
        t = V.Vunet(cfg, device="cuda:0", n_channels_x=3, vgg_width_div=8, total_steps=8, vgg_synthetic=True)
        torch.manual_seed(5)
        return t, float(t.train_fn(_batch("market", 41, raw))["loss"])
    (a, la), (b, lb) = run(True), run(False)
    assert la == lb and la == la
    _same_state(a, b)
