"""The float64 restatement of the part-normalised appearance input (tests/inplane_ref.py) against an independent sampler, against
answers derived by hand from the reference's rules (lib/utils.py:70-232, data/base_dataset.py:685-725), and through a round trip.
CPU only: this is the oracle the GPU tests (tests/test_hip_inplane.py) compare the kernels with."""
import numpy as np
import torch

import inplane_ref as R


def _image(n, hs, ws, seed):
    g = np.random.default_rng(seed)
    return g.uniform(-1.0, 1.0, size=(n, 3, hs, ws))


def _plausible_kps(n, hs, ws, seed):
    g = np.random.default_rng(seed)
    return g.uniform([2.0, 2.0], [ws - 2.0, hs - 2.0], size=(n, 18, 2)).astype(np.float32)


def test_sampler_matches_grid_sample_in_float64():
    """The warp against torch.nn.functional.grid_sample in float64 (bilinear, border padding, align_corners: pixel centres at
    integers) on the same homographies: <= 1e-12.  The homographies are those of both shipped part models on random keypoints, so
    rotated, sheared, perspective and partly outside the image."""
    hs, ws, s = 40, 56, 16
    img = _image(3, hs, ws, 1)
    worst, n_parts = 0.0, 0
    for parts, seed in ((R.MARKET, 2), (R.DEEPFASHION, 3)):
        kps = _plausible_kps(3, hs, ws, seed)
        minv, _, valid = R.part_transforms(kps, parts, s, hs)
        assert valid.all()
        got = R.warp(img, minv, valid, s)
        y, x = np.meshgrid(np.arange(s, dtype=np.float64), np.arange(s, dtype=np.float64), indexing="ij")
        for i in range(3):
            for q in range(len(parts)):
                m = minv[i, q]
                w = m[6] * x + m[7] * y + m[8]
                assert (w != 0.0).all()
                sx, sy = (m[0] * x + m[1] * y + m[2]) / w, (m[3] * x + m[4] * y + m[5]) / w
                grid = torch.from_numpy(np.stack([2.0 * sx / (ws - 1) - 1.0, 2.0 * sy / (hs - 1) - 1.0], axis=-1))[None]
                want = torch.nn.functional.grid_sample(torch.from_numpy(img[i:i + 1]), grid, mode="bilinear", padding_mode="border",
                                                       align_corners=True)[0].numpy()
                worst = max(worst, float(np.abs(got[i, 3 * q:3 * q + 3] - want).max()))
                n_parts += 1
    assert n_parts == 60 and worst <= 1e-12, worst


def test_t4p_on_an_axis_aligned_window_is_a_copy():
    """T4P sends the body joints, in order, to (0,0) (wh,0) (wh,wh) (0,wh).  Joints on the corners (x0, y0), (x0 + S, y0),
    (x0 + S, y0 + S), (x0, y0 + S) make the transform the translation by (x0, y0): the crop is img[y0 : y0 + S, x0 : x0 + S]."""
    s, x0, y0 = 16, 7, 5
    img = _image(1, 40, 56, 4)
    kps = np.zeros((1, 4, 2), dtype=np.float32)
    kps[0] = [[x0, y0], [x0 + s, y0], [x0 + s, y0 + s], [x0, y0 + s]]
    minv, src, valid = R.part_transforms(kps, [(R.T4P, (0, 1, 2, 3))], s, 40)
    assert valid[0, 0] == 1 and np.array_equal(src[0, 0], kps[0].astype(np.float64))
    np.testing.assert_allclose(minv[0, 0], [1, 0, x0, 0, 1, y0, 0, 0, 1], atol=1e-12)
    out = R.warp(img, minv, valid, s)
    assert np.abs(out[0] - img[0, :, y0:y0 + s, x0:x0 + s]).max() <= 1e-11


def test_t2p_on_a_vertical_limb():
    """T2P on k0 = (cx, y0), k1 = (cx, y0 + L): segment (0, L), normal (-L, 0), so a = (cx - L/4, y0), b = (cx + L/4, y0),
    c = (cx + L/4, y0 + L), d = (cx - L/4, y0 + L) go to (-1,-1), (-1, wh-1), (wh-1, wh-1), (wh-1, -1).  The crop's x axis therefore
    runs ALONG the limb and its y axis across it: source = (cx - L/4 + (Y + 1) L / (2 wh), y0 + (X + 1) L / wh).  With L = wh = 16
    that is (cx - 4 + (Y + 1) / 2, y0 + X + 1): a transposed copy on odd Y, the mean of two neighbours on even Y.  Corner pixels:
    (X, Y) = (wh-1, wh-1) is c itself, (0, wh-1) is (cx + 4, y0 + 1), (wh-1, 1) is (cx - 3, y0 + wh)."""
    s, cx, y0 = 16, 20, 6
    img = _image(1, 40, 56, 5)
    kps = np.array([[[cx, y0], [cx, y0 + s]]], dtype=np.float32)
    minv, src, valid = R.part_transforms(kps, [(R.T2P, (0, 1))], s, 40)
    assert valid[0, 0] == 1
    assert np.array_equal(src[0, 0], [[cx - 4, y0], [cx + 4, y0], [cx + 4, y0 + s], [cx - 4, y0 + s]])
    np.testing.assert_allclose(R.apply_h(minv[0, 0], R.dst_points(R.T2P, s)), src[0, 0], atol=1e-10)
    out = R.warp(img, minv, valid, s)[0]
    X = np.arange(s)
    for Y in range(s):
        if Y % 2:
            want = img[0, :, y0 + 1 + X, cx - 4 + (Y + 1) // 2].T
        else:
            want = 0.5 * (img[0, :, y0 + 1 + X, cx - 4 + Y // 2].T + img[0, :, y0 + 1 + X, cx - 4 + Y // 2 + 1].T)
        assert np.abs(out[:, Y, :] - want).max() <= 1e-10, Y
    assert np.abs(out[:, s - 1, s - 1] - img[0, :, y0 + s, cx + 4]).max() <= 1e-10          # c
    assert np.abs(out[:, s - 1, 0] - img[0, :, y0 + 1, cx + 4]).max() <= 1e-10
    assert np.abs(out[:, 1, s - 1] - img[0, :, y0 + s, cx - 3]).max() <= 1e-10


def test_t3p_normal_fallback_and_none():
    """T3P reads (right shoulder, left shoulder, head).  All >= 0: the box round neck + 2 (head - neck) -> neck, half its length to
    either side.  Head negative: the shoulder-only fallback -- seg = rs - ls, normal (-seg.y, seg.x) flipped to point up
    (normal.y <= 0), source = ls, rs, rs + n, ls + n to (0,0) (0,wh) (wh,wh) (wh,0); with ls = (lx, y), rs = (lx - wh, y) the
    crop is img[y - X, lx - Y].  A negative shoulder coordinate: None."""
    s = 16
    img = _image(1, 40, 56, 6)
    parts = [(R.T3P, (0, 1, 2))]
    # normal: rs = (10, 30), ls = (20, 30), head = (15, 24): neck (15, 30), top (15, 18), segment (0, 12), normal (-12, 0)
    src = R.src_points(np.array([[10, 30], [20, 30], [15, 24]], dtype=np.float32), R.T3P, (0, 1, 2), 40)
    assert np.array_equal(src, [[21, 18], [21, 30], [9, 30], [9, 18]])                     # b, c, d, a
    # fallback
    lx, y = 30, 25
    kps = np.array([[[lx - s, y], [lx, y], [-1.0, 12.0]]], dtype=np.float32)
    minv, src, valid = R.part_transforms(kps, parts, s, 40)
    assert valid[0, 0] == 1
    assert np.array_equal(src[0, 0], [[lx, y], [lx - s, y], [lx - s, y - s], [lx, y - s]])
    out = R.warp(img, minv, valid, s)[0]
    X = np.arange(s)
    for Y in range(s):
        assert np.abs(out[:, Y, :] - img[0, :, y - X, lx - Y].T).max() <= 1e-10, Y
    # the flip: shoulders swapped give normal (0, +16) before the flip, the same upward box after it
    src2 = R.src_points(np.array([[lx, y], [lx - s, y], [5.0, -0.5]], dtype=np.float32), R.T3P, (0, 1, 2), 40)
    assert np.array_equal(src2, [[lx - s, y], [lx, y], [lx, y - s], [lx - s, y - s]])
    # a negative shoulder: absent, all -1
    kps[0, 0, 1] = -0.25
    minv, src, valid = R.part_transforms(kps, parts, s, 40)
    assert valid[0, 0] == 0 and not src.any() and not minv.any()
    assert (R.warp(img, minv, valid, s) == -1.0).all()


def test_t2p_leg_fallback_and_none():
    """A joint with both coordinates <= 0: the box goes from the other joint t straight down to row oh - 1, a quarter of that
    length to either side.  t = (20, 15), oh = 40: segment (0, 24), normal (-24, 0): a = (14, 15), b = (26, 15), c = (26, 39),
    d = (14, 39).  Both joints at (0, 0) -- or the other joint not strictly positive in both coordinates: None."""
    s = 16
    for order in ((0, 1), (1, 0)):
        kps = np.zeros((2, 2), dtype=np.float32)
        kps[order[1]] = [20, 15]
        src = R.src_points(kps, R.T2P, (0, 1), 40)
        assert np.array_equal(src, [[14, 15], [26, 15], [26, 39], [14, 39]])
    assert R.src_points(np.zeros((2, 2), dtype=np.float32), R.T2P, (0, 1), 40) is None
    assert R.src_points(np.array([[0, 0], [-3, 15]], dtype=np.float32), R.T2P, (0, 1), 40) is None
    # (x <= 0 with y > 0 is no fallback case: the joint is used as it is)
    assert np.array_equal(R.src_points(np.array([[-4, 8], [4, 8]], dtype=np.float32), R.T2P, (0, 1), 40),
                          [[-4, 10], [-4, 6], [4, 6], [4, 10]])
    minv, _, valid = R.part_transforms(np.zeros((1, 2, 2), dtype=np.float32), [(R.T2P, (0, 1))], s, 40)
    assert valid[0, 0] == 0 and (R.warp(_image(1, 40, 56, 7), minv, valid, s) == -1.0).all()


def test_coincident_joints_make_the_part_absent():
    """Two limb joints on one point: the four source points coincide, the 8x8 system is singular, a pivot falls below the
    threshold: the part is absent and the crop all -1 (OpenCV would return whatever its decomposition yields)."""
    img = _image(1, 40, 56, 8)
    kps = np.array([[[12.5, 9.25], [12.5, 9.25], [30, 30], [30, 30], [30, 30], [30, 30]]], dtype=np.float32)
    parts = [(R.T2P, (0, 1)), (R.T4P, (2, 3, 4, 5))]
    minv, _, valid = R.part_transforms(kps, parts, 16, 40)
    assert not valid.any() and not minv.any()
    assert (R.warp(img, minv, valid, 16) == -1.0).all()
    # three collinear corners: also singular
    kps = np.array([[[5, 5], [15, 5], [25, 5], [5, 20]]], dtype=np.float32)
    assert R.part_transforms(kps, [(R.T4P, (0, 1, 2, 3))], 16, 40)[2][0, 0] == 0


def test_quad_outside_the_image_replicates_the_border():
    """A body window wholly to the right of the image: every source x clamps to Ws - 1, the rows stay: the crop repeats the last
    column.  Wholly above and to the left: the crop is the corner pixel."""
    s, hs, ws = 16, 40, 56
    img = _image(1, hs, ws, 9)
    kps = np.array([[[100, 4], [116, 4], [116, 20], [100, 20]]], dtype=np.float32)
    minv, _, valid = R.part_transforms(kps, [(R.T4P, (0, 1, 2, 3))], s, hs)
    out = R.warp(img, minv, valid, s)[0]
    assert valid[0, 0] == 1 and np.abs(out - img[0, :, 4:20, ws - 1:ws]).max() <= 1e-12
    minv, _, valid = R.part_transforms(kps - np.float32(200), [(R.T4P, (0, 1, 2, 3))], s, hs)
    out = R.warp(img, minv, valid, s)[0]
    assert valid[0, 0] == 1 and np.array_equal(out, np.broadcast_to(img[0, :, :1, :1], out.shape))


def test_w_zero_samples_the_origin():
    """A homography whose third row vanishes on a crop pixel: that pixel takes source (0, 0), as OpenCV's warpPerspective does."""
    img = _image(1, 40, 56, 10)
    minv = np.array([[[1.0, 0, 2, 0, 1, 3, 1, 0, -3]]])
    out = R.warp(img, minv, np.ones((1, 1), dtype=np.int32), 8)[0]
    assert np.array_equal(out[:, :, 3], np.broadcast_to(img[0, :, 0, 0][:, None], (3, 8)))
    sx, _ = R.source_coords(minv[0, 0], 8, 40, 56)
    assert sx[0, 4] == 6.0 and sx[0, 2] == 0.0        # (4 + 2) / 1;  (2 + 2) / -1 clamped


def test_round_trip_of_random_quads():
    """Minv applied to the four destination corners returns the source points, for random convex quads and both corner orders.
    Bound 1e-4 px: float64 epsilon x a condition number of up to 1e9 for pixel-scale systems x a 256 px range ~ 3e-5."""
    g = np.random.default_rng(11)
    worst, n = 0.0, 0
    while n < 200:
        c = g.uniform(20, 236, size=2)
        ang = np.sort(g.uniform(0, 2 * np.pi, size=4))
        q = c + g.uniform(8, 60, size=(4, 1)) * np.stack([np.cos(ang), np.sin(ang)], axis=1)
        e = np.roll(q, -1, axis=0) - q
        cross = e[:, 0] * np.roll(e, -1, axis=0)[:, 1] - e[:, 1] * np.roll(e, -1, axis=0)[:, 0]
        if not ((cross > 0).all() and R.quad_area(q) >= 16.0):
            continue
        kind = (R.T4P, R.T2P)[n % 2]
        dst = R.dst_points(kind, (16, 32, 64)[n % 3])
        m = R.solve_inverse(q, dst)
        assert m is not None
        worst = max(worst, float(np.abs(R.apply_h(m, dst) - q).max()))
        n += 1
    assert worst <= 1e-4, worst


def test_package_part_lists_match_the_restatement():
    """The shipped part models are the lists this restatement transcribes from data/market.py:45 and data/deepfashion.py:61-72."""
    from behavior_driven_video_synthesis_amd import inplane
    assert list(inplane.MARKET_PARTS.parts) == R.MARKET and list(inplane.DEEPFASHION_PARTS.parts) == R.DEEPFASHION
    assert inplane.MARKET_PARTS.n_parts == inplane.DEEPFASHION_PARTS.n_parts == 10
    assert inplane.part_model("market") is inplane.MARKET_PARTS and inplane.part_model([(R.T5P, (0, 14, 8, 11, 3))]).min_joints == 15
    assert inplane.configured_parts({"dataset": "Market", "inplane_normalize": True}) is inplane.MARKET_PARTS
    assert inplane.configured_parts({"dataset": "Market", "inplane_normalize": False}) is None
    assert inplane.configured_parts({"dataset": "Human3.6m", "inplane_normalize": True}) is None
