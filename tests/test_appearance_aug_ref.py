"""The NumPy restatement of the random appearance augmentation (tests/appearance_aug_ref.py) against Pillow -- through the stored
fixture (tests/golden/g22_appearance_aug.npz, written with Pillow 12.2.0) and, where PIL imports, directly -- and the host side of
behavior_driven_video_synthesis_amd/appearance_aug.py: ``rotation_matrix`` against the bytes of ``Image.rotate``,
``inverse_affine``, the draws of ``AppearanceAug``, the launch arguments, the host validation and the hook's refusals.  No GPU.
Everything here is exact."""
import math
import random

import numpy as np
import pytest
import torch

import appearance_aug_ref as R

FIX = R.load_fixture()


@pytest.mark.parametrize("name", list(FIX))
def test_restatement_equals_the_pillow_fixture(name):
    c = FIX[name]
    out, status = R.affine_stack(c["frames"], c["hw"], c["mats"], **c["kw"])
    assert not status.any()
    assert out.dtype == np.uint8 and out.shape == c["expect"].shape and np.array_equal(out, c["expect"])


def test_fixture_covers_what_it_is_for():
    assert set(FIX) >= {"affine_24x24", "affine_17x29", "affine_32x20", "affine_identity", "affine_far", "affine_mixed",
                        "rotate_32x16", "rotate_24x24", "rotate_20x6", "rotate_12x1", "chain_32x16"}
    c = FIX["affine_identity"]
    assert np.array_equal(c["expect"][0], c["frames"][0])                          # identity: the source itself
    assert (FIX["affine_far"]["expect"] == 255).all(axis=-1).mean() > 0.25          # large filled regions
    m = FIX["affine_mixed"]
    assert (m["frames"][1, 17:] == R.PAD_BYTE).all() and m["kw"]["out_hw"] == (34, 31) and len(set(map(tuple, m["hw"]))) == 3
    assert FIX["rotate_24x24"]["angles"][:4].tolist() == [90.0, -90.0, 0.0, 45.0]
    t = FIX["rotate_20x6"]
    assert t["kw"]["pad"] > t["hw"][0, 1] - 1                                       # the reflection repeats
    assert FIX["rotate_12x1"]["hw"][0, 1] == 1
    assert FIX["chain_32x16"]["kw"]["size"] == 12 and FIX["chain_32x16"]["expect"].shape == (1, 12, 12, 3)


def test_reflect_is_numpys():
    for n in (1, 2, 3, 6, 10):
        a = np.arange(n)
        for p in (0, 1, n - 1, n, 3 * n + 2):
            want = np.pad(a, p, mode="reflect")
            assert np.array_equal(R.refl(np.arange(-p, n + p), n), want), (n, p)
    assert R.refl(np.arange(-4, 8), 4).tolist() == [2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1]


def test_restatement_equals_pillow_directly():
    """Every case of the fixture made afresh, and a few dozen further seeded ones: affines on odd sizes with windows larger than
    the frame, rotations of padded frames at random and special angles."""
    pytest.importorskip("PIL.Image")
    import make_golden_appearance_aug as G
    from behavior_driven_video_synthesis_amd import appearance_aug as A
    frames, cases = G.build_cases()
    for name, c in cases.items():
        assert np.array_equal(c["expect"], FIX[name]["expect"]), name               # (this Pillow gives the stored bytes)
    g, rnd = np.random.default_rng(7), random.Random(7)
    for k in range(24):
        h, w = int(g.integers(1, 40)), int(g.integers(1, 40))
        f = g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        mat = A.inverse_affine((w * 0.5 + 0.5, h * 0.5 + 0.5), rnd.uniform(-180, 180), (rnd.uniform(-w, w), rnd.uniform(-h, h)),
                               rnd.uniform(0.3, 2.5))
        out_hw, fill = (h + k % 5, w + k % 3), (k * 10 % 256, 255 - k, 7)
        want = G.pillow_affine(f, mat, 0, (k % 4, k % 2), out_hw, fill)
        got, _ = R.affine_u8(f, mat, 0, (k % 4, k % 2), out_hw, fill)
        assert np.array_equal(got, want), ("affine", k, h, w)
    for k in range(24):
        h, w, p = int(g.integers(1, 33)), int(g.integers(1, 33)), int(g.integers(0, 12))
        f = g.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        angle = (0.0, 90.0, 180.0, 270.0, -45.0, 360.0)[k] if k < 6 else rnd.uniform(-400, 400)
        crop = min(h, w) + p
        origin = G.center_origin((h, w), p, crop)
        want = G.pillow_rotate(f, angle, p, origin, (crop, crop))
        got, _ = R.affine_u8(f, A.rotation_matrix(w + 2 * p, h + 2 * p, angle), p, origin, (crop, crop), (0, 0, 0))
        assert np.array_equal(got, want), ("rotate", k, h, w, p, angle)


def test_rotation_matrix_gives_the_bytes_of_image_rotate():
    """The fixture's rotate cases were made by ``Image.rotate`` itself: the package's matrix is the stored one, bit for bit, and
    the restatement with it gives Pillow's bytes."""
    from behavior_driven_video_synthesis_amd import appearance_aug as A
    n = 0
    for name, c in FIX.items():
        for i, ang in enumerate(c["angles"]):
            if math.isnan(ang):
                continue
            h, w = (int(v) + 2 * c["kw"]["pad"] for v in c["hw"][i])
            m = A.rotation_matrix(w, h, float(ang))
            assert np.array_equal(np.asarray(m), c["mats"][i]), (name, i)
            kw = dict(c["kw"])
            size = kw.pop("size")
            got, _ = R.affine_stack(c["frames"][i:i + 1], c["hw"][i:i + 1], [m], size=size, **kw)
            assert np.array_equal(got[0], c["expect"][i]), (name, i)
            n += 1
    assert n >= 10
    assert A.rotation_matrix(36, 36, 0.0) == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    assert A.rotation_matrix(36, 36, 90.0) == [0.0, -1.0, 36.0, 1.0, 0.0, 0.0]
    assert A.rotation_matrix(10, 20, 360.0 + 30.0)[:2] == [round(math.cos(-math.radians(30.0)), 15), round(math.sin(-math.radians(30.0)), 15)]


def test_inverse_affine_is_the_stated_formula():
    from behavior_driven_video_synthesis_amd import appearance_aug as A
    assert A.inverse_affine((12.5, 12.5), 0.0, (0, 0), 1.0) == [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]
    assert A.inverse_affine((3.0, 4.0), 0.0, (2, -1), 0.5) == [2.0, 0.0, -7.0, 0.0, 2.0, -2.0]
    c, s = math.cos(math.radians(90.0)), math.sin(math.radians(90.0))
    d = c * c + s * s
    m = A.inverse_affine((5.0, 7.0), 90.0, (1, 0), 1.0)
    want2 = 0.0 + ((1.0 / d * c) * (-5.0 - 1) + (1.0 / d * s) * (-7.0 - 0))
    assert m[:2] == [1.0 / d * c, 1.0 / d * s] and m[3] == 1.0 / d * -s and m[2] == want2 + 5.0
    # the fixture's matrices of the DeepFashion form are this function's (the writer keeps its own copy of the formula)
    f = FIX["affine_identity"]
    assert np.array_equal(np.asarray(A.inverse_affine((12.5, 12.5), 0.0, (0, 0), 1.0)), f["mats"][0])


def test_draws_are_reproducible_and_consume_the_stated_order():
    from behavior_driven_video_synthesis_amd import appearance_aug as A
    hw = np.array([[24, 24], [17, 29], [32, 20]], dtype=np.int32)
    a, b = A.AppearanceAug("deepfashion", seed=5).draw(hw), A.AppearanceAug("deepfashion", seed=5).draw(hw)
    assert a.dtype == np.float64 and a.shape == (3, 6) and np.array_equal(a, b)
    assert not np.array_equal(a, A.AppearanceAug("deepfashion", seed=6).draw(hw))
    rnd = random.Random(5)
    for (h, w), row in zip(hw.tolist(), a):
        angle = rnd.uniform(-30.0, 30.0)
        tx = round(rnd.uniform(-0.3 * w, 0.3 * w))
        rnd.uniform(0.0, 0.0)                                                       # ty: drawn although it is 0
        scale = rnd.uniform(0.7, 1.0)
        assert row.tolist() == A.inverse_affine((w * 0.5 + 0.5, h * 0.5 + 0.5), angle, (tx, 0), scale)
    aug = A.AppearanceAug("deepfashion", seed=5)
    first = aug.draw(hw[:1])
    assert np.array_equal(first, a[:1]) and np.array_equal(aug.draw(hw[1:]), a[1:])  # one generator, consumed in order
    assert aug.launch_args(256) == dict(pad=0, origin=(0, 0), out_hw=None, fill=(255, 255, 255))
    m = A.AppearanceAug("market", seed=9, size=64)
    rows, rnd = m.draw(np.array([[128, 64], [128, 64]])), random.Random(9)
    for row in rows:
        assert row.tolist() == A.rotation_matrix(64 + 64, 128 + 64, rnd.uniform(-90.0, 90.0))
    assert m.launch_args(64, (128, 64)) == dict(pad=32, origin=(0, 32), out_hw=(128, 128), fill=(0, 0, 0))
    assert A.AppearanceAug("market", crop=16).launch_args(16, (32, 16)) == dict(pad=8, origin=(8, 16), out_hw=(16, 16), fill=(0, 0, 0))
    with pytest.raises(ValueError):
        A.AppearanceAug("h36m")
    with pytest.raises(ValueError):
        A.AppearanceAug("market").draw(hw)                                          # the pad needs the size
    with pytest.raises(ValueError):
        A.AppearanceAug("market", size=64).launch_args()                            # the crop origin needs the frame size


def test_host_validation_refuses_bad_shapes_and_dtypes():
    from behavior_driven_video_synthesis_amd import appearance_aug as A
    ok = np.tile(np.array([1.0, 0, 0, 0, 1, 0]), (2, 1))
    assert A.check_mats(ok, 2).dtype == torch.float64 and tuple(A.check_mats(ok.astype(np.float32), 2).shape) == (2, 6)
    assert A.check_mats(torch.from_numpy(ok), 2).tolist() == ok.tolist()
    for bad in (ok[:1], ok[:, :5], ok.astype(np.int64), np.where(np.eye(2, 6) > 0, np.nan, ok), np.where(np.eye(2, 6) > 0, np.inf, ok)):
        with pytest.raises(ValueError):
            A.check_mats(bad, 2)
    assert A.check_hw([[3, 4], [1, 1]], 2, 3, 4).dtype == torch.int32
    for bad in ([[3, 4]], [[3.0, 4.0], [1.0, 1.0]], [[4, 4], [1, 1]], [[3, 5], [1, 1]], [[0, 1], [1, 1]], [[3, 4, 1], [1, 1, 1]]):
        with pytest.raises(ValueError):
            A.check_hw(np.asarray(bad), 2, 3, 4)
    frames = np.zeros((2, 3, 4, 3), dtype=np.uint8)
    with pytest.raises(ValueError):
        A.affine_images(frames.astype(np.float32), ok)                              # (all refused before any launch)
    with pytest.raises(ValueError):
        A.affine_images(frames[..., :2], ok)


def test_hook_leaves_other_batches_alone_and_refuses_the_crop_route():
    from behavior_driven_video_synthesis_amd import appearance_aug as A
    u8, mats = torch.zeros(1, 4, 4, 3, dtype=torch.uint8), np.array([[1.0, 0, 0, 0, 1, 0]])
    aug = A.AppearanceAug("deepfashion")
    assert A.batch_appearance({"pose_img": 0}, 4, aug) == {}
    assert A.batch_appearance({"pose_img_u8": u8}, 4, aug) == {}
    assert A.batch_appearance({"pose_img_aug": mats}, 4, aug) == {}
    assert A.batch_appearance({"pose_img_u8": u8, "pose_img_aug": mats, "pose_img_inplane": 0}, 4, aug) == {}
    with pytest.raises(ValueError):
        A.batch_appearance({"pose_img_u8": u8, "pose_img_aug": mats, "pose_img_geom": np.zeros((1, 6), dtype=np.int32)}, 4, aug)
    with pytest.raises(ValueError):
        A.batch_appearance({"pose_img_u8": u8, "pose_img_aug": mats}, 4, None)    # nothing configured
    b = {"pose_img": 0, "stickman": 1}
    assert A.to_device(b, "cpu") is b
