"""The NumPy restatement of the raw-frame input route (tests/image_input_ref.py) against Pillow -- through the stored fixture
(tests/golden/g19_image_input.npz, written with Pillow 12.2.0) and, where PIL imports, directly -- and the host side of
behavior_driven_video_synthesis_amd/image_input.py: ``bounding_box`` against hand-derived answers and against the reference's
pad-then-slice replayed in NumPy, ``stack_frames``, the host validation.  No GPU.  Everything here is exact."""
import numpy as np
import pytest
import torch

import image_input_ref as R

FIX = R.load_fixture()


@pytest.mark.parametrize("name", list(FIX))
def test_restatement_equals_the_pillow_fixture(name):
    c = FIX[name]
    out, status = R.frames_to_u8(c["frames"], c["geom"], c["size"])
    assert not status.any()
    assert out.dtype == np.uint8 and np.array_equal(out, c["expect"])


def test_fixture_covers_what_it_is_for():
    assert len(FIX["batch"]["geom"]) == 8 and (FIX["batch"]["frames"][0, 40:, :] == R.PAD_BYTE).all()
    up = FIX["up_8x5"]["expect"]
    assert up.min() == 0 and up.max() == 255
    g = FIX["skip_16x40"]["geom"][0]
    assert g[5] == FIX["skip_16x40"]["size"] and g[4] != g[5]                       # the vertical axis is skipped
    h, w, x0, y0, cw, ch = FIX["crop_wider_than_frame"]["geom"][0]
    assert w == 10 and x0 < -w and x0 + cw > 2 * w and ch > h                            # more than one reflection on both sides
    # the saturating taps: an upscaled 0 / 255 edge overshoots below 0 and above 255 before the clamp
    b, k = R.tables(5, 16)
    row = FIX["up_8x5"]["frames"][0, :, :, 0].astype(np.int64)
    acc = np.stack([(1 << 21) + row[:, b[x, 0]:b[x, 0] + b[x, 1]] @ k[x, :b[x, 1]].astype(np.int64) for x in range(16)], axis=1) >> 22
    assert acc.min() < 0 and acc.max() > 255


def test_restatement_equals_pillow_directly():
    Image = pytest.importorskip("PIL.Image")
    g = np.random.default_rng(5)
    for (h, w, s) in [(37, 53, 16), (8, 5, 16), (16, 40, 16), (1, 7, 4), (64, 64, 24), (19, 64, 33), (50, 3, 8), (33, 47, 47)]:
        for kind in ("random", "binary", "checker"):
            if kind == "random":
                img = g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
            elif kind == "binary":
                img = (g.integers(0, 2, size=(h, w, 3)) * 255).astype(np.uint8)
            else:
                img = np.broadcast_to((((np.add.outer(np.arange(h), np.arange(w))) % 2) * 255).astype(np.uint8)[..., None], (h, w, 3)).copy()
            want = np.asarray(Image.fromarray(img, "RGB").resize((s, s), Image.BICUBIC))
            assert np.array_equal(R.resize(img, s), want), (h, w, s, kind)


def test_reflect_is_the_stated_rule():
    for length in (1, 2, 3, 10):
        for p in range(-5 * length - 3, 5 * length + 3):
            assert int(R.reflect(p, length)) == R.reflect_loop(p, length), (p, length)
    assert [int(R.reflect(p, 4)) for p in range(-6, 10)] == [2, 3, 3, 2, 1, 0, 0, 1, 2, 3, 3, 2, 1, 0, 0, 1]


def test_identity_table_is_a_skipped_axis():
    img = np.random.default_rng(1).integers(0, 256, size=(9, 12, 3), dtype=np.uint8)
    b, k = R.tables(12, 12)
    assert np.array_equal(R._pass(img, b, k), img)
    assert R.ksize_of(1002, 256) == 17 and R.ksize_max(1000, 1002, 256) == 17 and R.ksize_of(5, 16) == 5


def test_to_float_is_the_torch_expression():
    u8 = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1).repeat(3, axis=3)
    want = torch.from_numpy(u8).permute(0, 3, 1, 2).float().div(255).mul(2.0).sub(1.0)
    assert torch.equal(torch.from_numpy(R.to_float(u8)), want)


# ---- the host side of the package --------------------------------------------------------------------------------------------
def test_bounding_box_hand_derived():
    from behavior_driven_video_synthesis_amd import image_input as I
    # a wide pose: x in [10.5, 49.2] -> x = 10, w = 49 - 10 + 1 = 40; y in [20.0, 30.9] -> y = 20, h = 11.  w >= h:
    # x_tl = int(10 - 4.0) = 6, x_br = int(10 + 1.1 * 40) = 54, D = 48; y_tl = int((40 + 11 - 48) / 2) = int(1.5) = 1,
    # y_br = int((51 + 48) / 2) = int(49.5) = 49
    wide = np.array([[10.5, 20.0], [49.2, 25.0], [30.0, 30.9]])
    assert I.bounding_box(wide, (64, 64)).tolist() == [[64, 64, 6, 1, 48, 48]]
    # a tall pose: x in [30.0, 35.5] -> x = 30, w = 6; y in [5.2, 44.9] -> y = 5, h = 40.  y_tl = int(5 - 4.0) = 1,
    # y_br = int(5 + 44.0...) = 49, D = 48; x_tl = int((60 + 6 - 48) / 2) = 9, x_br = int((66 + 48) / 2) = 57
    tall = np.array([[30.0, 5.2], [35.5, 44.9], [33.0, 17.0]])
    assert I.bounding_box(tall, (64, 72)).tolist() == [[64, 72, 9, 1, 48, 48]]
    # over the left, top and right edges of a 40 x 40 frame, ``int`` truncating toward zero: x in [2.0, 38.5] -> x = 2, w = 37;
    # y in [1.0, 20.5] -> y = 1, h = 20.  x_tl = int(2 - 3.7) = int(-1.7) = -1 (floor would give -2), x_br = int(2 + 40.7) = 42,
    # D = 43; y_tl = int((2 + 20 - 43) / 2) = int(-10.5) = -10, y_br = int((22 + 43) / 2) = int(32.5) = 32
    over = np.array([[2.0, 1.0], [38.5, 20.5], [20.0, 10.0]])
    assert I.bounding_box(over, (40, 40)).tolist() == [[40, 40, -1, -10, 43, 42]]
    # batched, a torch tensor, one size for all, extra columns ignored, another relax
    kps = torch.tensor(np.stack([np.c_[wide, np.ones(3)], np.c_[tall, np.ones(3)]]))
    assert I.bounding_box(kps, (64, 64)).tolist() == [[64, 64, 6, 1, 48, 48], [64, 64, 9, 1, 48, 48]]
    assert I.bounding_box(wide, (64, 64), relax=0.0).tolist() == [[64, 64, 10, 5, 40, 40]]
    assert R.bounding_rect(wide) == (10, 20, 40, 11)
    with pytest.raises(ValueError):
        I.bounding_box(np.zeros((2, 3, 2)), np.zeros((3, 2)))


def test_bounding_box_window_is_the_references_pad_then_slice():
    """The derivation of the docstring, replayed: pad the frame as ``get_bounding_box`` says (each pad on its own side, the border
    reflected), slice with the shifted box as ``_get_pose_img`` does -- the crop equals the reflected window of the geometry row."""
    from behavior_driven_video_synthesis_amd import image_input as I
    g = np.random.default_rng(3)
    frame = g.integers(0, 256, size=(40, 48, 3), dtype=np.uint8)
    poses = [np.array([[2.0, 1.0], [38.5, 20.5]]), np.array([[20.0, 15.0], [47.0, 39.5]]), np.array([[10.0, 12.0], [30.0, 22.0]]),
             np.array([[-6.0, 3.0], [60.0, 8.0]])]
    for pts in poses:
        row = I.bounding_box(pts, frame.shape[:2])[0]
        _, _, x_tl, y_tl, cw, ch = (int(v) for v in row)
        bbox = [x_tl, x_tl + cw, y_tl, y_tl + ch]
        pl, pr = abs(min(0, bbox[0])), abs(max(0, bbox[1] - frame.shape[1]))
        pt, pb = abs(min(0, bbox[2])), abs(max(0, bbox[3] - frame.shape[0]))
        bbox = [bbox[0] + pl, bbox[1] + pl + pr, bbox[2] + pt, bbox[3] + pt + pb]
        padded = np.pad(frame, ((pt, pb), (pl, pr), (0, 0)), mode="symmetric")
        crop = padded[bbox[2]:bbox[3], bbox[0]:bbox[1]]
        assert np.array_equal(crop, R.window(frame[None], 0, row)), pts.tolist()


def test_stack_frames():
    from behavior_driven_video_synthesis_amd import image_input as I
    g = np.random.default_rng(2)
    a, b = g.integers(0, 256, size=(5, 9, 3), dtype=np.uint8), g.integers(0, 256, size=(7, 4, 3), dtype=np.uint8)
    stack, hw = I.stack_frames([a, torch.from_numpy(b)])
    assert stack.dtype == torch.uint8 and tuple(stack.shape) == (2, 7, 9, 3) and hw.dtype == torch.int32
    assert hw.tolist() == [[5, 9], [7, 4]]
    s = stack.numpy()
    assert np.array_equal(s[0, :5, :9], a) and np.array_equal(s[1, :7, :4], b)
    assert not s[0, 5:].any() and not s[1, :, 4:].any()
    big, _ = I.stack_frames([a, b], hmax=12, wmax=3)
    assert tuple(big.shape) == (2, 12, 9, 3) and np.array_equal(big.numpy()[1, :7, :4], b)
    for bad in ([], [a.astype(np.float32)], [a[..., :2]], [a[0]]):
        with pytest.raises(ValueError):
            I.stack_frames(bad)


def test_host_validation():
    from behavior_driven_video_synthesis_amd import image_input as I
    ok = np.array([[40, 48, -7, -4, 33, 29], [10, 48, 100000, -100000, 48, 40]], dtype=np.int32)
    t = I.check_geom(ok, 2, 40, 48)
    assert t.dtype == torch.int32 and t.tolist() == ok.tolist()
    assert I.check_geom(torch.from_numpy(ok), 2, 40, 48).tolist() == ok.tolist()
    for col, val in [(4, 0), (5, 41), (4, 49), (5, 0), (0, 0), (0, 41), (1, 0), (1, 49)]:
        bad = ok.copy()
        bad[1, col] = val
        with pytest.raises(ValueError, match="row 1"):
            I.check_geom(bad, 2, 40, 48)
    for bad in (ok[:1], ok[:, :5], ok.astype(np.float32), ok.astype(np.int64) + (1 << 40) * np.eye(2, 6, 2, dtype=np.int64)):
        with pytest.raises(ValueError):
            I.check_geom(bad, 2, 40, 48)
    for frames in (np.zeros((2, 4, 4, 3), dtype=np.float32), np.zeros((2, 4, 4), dtype=np.uint8), np.zeros((2, 4, 4, 4), dtype=np.uint8)):
        with pytest.raises(ValueError):
            I.frames_to_images(frames)
    assert I.ksize_max(1000, 1002, 256) == R.ksize_max(1000, 1002, 256) == 17
    assert I.ksize_max(8, 5, 16) == 5 and I.ksize_max(61, 64, 32) == R.ksize_of(64, 32) == 9
    # a batch of ready images is left alone: nothing made, the same dict back
    batch = {"pose_img": torch.zeros(1, 3, 4, 4), "pose_img_u8": torch.zeros(1, 4, 4, 3, dtype=torch.uint8), "stickman": torch.zeros(1)}
    assert I.batch_images(batch, 4) == {} and I.batch_images({"stickman": batch["stickman"]}, 4) == {}
    assert I.to_device(batch, "cpu") is batch
