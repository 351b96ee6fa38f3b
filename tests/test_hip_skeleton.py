"""-m gpu: the skeleton-frame kernel (csrc/skeleton.hip) and its host surface, bit-exact against tests/skeleton_ref.py -- the
sequential canvas of oracle/stickman_oracle.c, then the reference's own numpy resize / crop / span / overlay expressions."""
import numpy as np
import pytest
import torch

import skeleton_ref as R
from test_hip_seq import TOL        # what generate_seq is held to between batch sizes

pytestmark = pytest.mark.gpu

LIMBS = [(0, 1), (1, 2), (3, 4), (4, 5), (3, 6), (0, 6), (6, 7), (7, 8), (8, 9), (9, 10), (8, 11), (8, 14), (11, 12),
         (12, 13), (14, 15), (15, 16)]


def _colors(seed, n=16):
    return np.random.default_rng(seed).integers(1, 255, size=(n, 3)).astype(np.uint8)


def _person(rng, f, hs, ws, cx=None):
    """``f`` person-sized figures on an hs x ws canvas, centred at column ``cx`` (default: somewhere inside)."""
    cx = rng.uniform(0.2 * ws, 0.8 * ws, size=f) if cx is None else np.broadcast_to(np.asarray(cx, dtype=np.float64), (f,))
    k = rng.normal(0.0, 1.0, size=(f, 17, 2)) * (0.06 * ws, 0.15 * hs)
    k[..., 0] += cx[:, None]
    k[..., 1] += 0.5 * hs
    return k.astype(np.float32)


def _frames(kps, *a, **kw):
    from behavior_driven_video_synthesis_amd.render import skeleton_frames
    return skeleton_frames(torch.from_numpy(np.ascontiguousarray(kps)).cuda(), *a, **kw)


# ---- 1. native size
@pytest.mark.parametrize("thickness", [1, 3, 6])
@pytest.mark.parametrize("background", [255, 0, 37])
def test_native_size_limbs_leave_the_canvas_on_every_side(background, thickness):
    rng = np.random.default_rng(10 * thickness + background)
    hs, ws = 37, 53
    kps = (rng.uniform(-0.4, 1.4, size=(4, 17, 2)) * (ws, hs)).astype(np.float32)
    assert (kps < 0).any() and (kps[..., 0] > ws).any() and (kps[..., 1] > hs).any()
    colors = _colors(1)
    want = R.canvas(kps, LIMBS, colors, hs, ws, thickness, background)
    got = _frames(kps, (hs, ws), LIMBS, colors.tolist(), target_size=None, background=background, thickness=thickness)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (4, hs, ws, 3)
    assert np.array_equal(got.cpu().numpy(), want)
    assert (want != background).any(axis=-1).mean() > 0.02


@pytest.mark.parametrize("thickness", [1, 3])
def test_end_points_far_outside_the_canvas(thickness):
    """Limbs that cross the canvas between end points hundreds of canvas sizes away: the clip intersections, and the edge chains
    of the quad walked down from tens of thousands of rows above the canvas, against the sequential walk; the kernel's distance
    pre-test must stay a superset there."""
    rng = np.random.default_rng(thickness)
    hs, ws = 37, 53
    kps = (rng.uniform(-600.0, 600.0, size=(8, 17, 2)) * (ws, hs)).astype(np.float32)
    kps[:, ::4] = (rng.uniform(0.0, 1.0, size=(8, 5, 2)) * (ws, hs)).astype(np.float32)      # some end points inside
    colors = _colors(9)
    want = R.canvas(kps, LIMBS, colors, hs, ws, thickness, 255)
    got = _frames(kps, (hs, ws), LIMBS, colors.tolist(), target_size=None, thickness=thickness)
    assert np.array_equal(got.cpu().numpy(), want)
    assert (want != 255).any(axis=(1, 2, 3)).sum() >= 6
    # beyond the documented limit of 2^20 pixels a limb is not drawn; the others are
    kps[0, 0] = (3.0e6, 5.0)
    got = _frames(kps[:1], (hs, ws), LIMBS, colors.tolist(), target_size=None, thickness=thickness)
    keep = [i for i, l in enumerate(LIMBS) if 0 not in l]
    assert np.array_equal(got.cpu().numpy(), R.canvas(kps[:1], [LIMBS[i] for i in keep], colors[keep], hs, ws, thickness, 255))


@pytest.mark.parametrize("thickness", [0, 1, 3])
def test_the_later_limb_wins_in_all_three_channels(thickness):
    kps = np.zeros((1, 4, 2), dtype=np.float32)
    kps[0] = [(1, 1), (7, 7), (1, 7), (7, 1)]
    limbs, colors = [(0, 1), (2, 3)], [(200, 0, 50), (0, 90, 0)]
    got = _frames(kps, (9, 9), limbs, colors, target_size=None, thickness=thickness).cpu().numpy()
    assert np.array_equal(got, R.canvas(kps, limbs, colors, 9, 9, thickness, 255))
    assert got[0, 4, 4].tolist() == [0, 90, 0] and got[0, 1, 1].tolist() == [200, 0, 50] and got[0, 0, 4].tolist() == [255] * 3
    swapped = _frames(kps, (9, 9), limbs[::-1], colors[::-1], target_size=None, thickness=thickness).cpu().numpy()
    assert swapped[0, 4, 4].tolist() == [200, 0, 50]


# ---- 2. sampling
@pytest.mark.parametrize("src,dst", [((1002, 1000), (256, 256)), ((37, 53), (16, 15)), ((20, 20), (64, 64))])
def test_nearest_sampling_equals_the_indexed_canvas(src, dst):
    """The expectation is the full canvas, indexed by the host tables.  16 x 15: the odd width takes the byte-store tail;
    20 -> 64: up-scaling repeats canvas pixels."""
    from behavior_driven_video_synthesis_amd.render import nearest_table
    rng = np.random.default_rng(src[0])
    (hs, ws), (ht, wt) = src, dst
    kps = _person(rng, 3, hs, ws)
    kps[2, :, 0] += 0.02 * ws - kps[2, :, 0].mean()              # one frame partly outside
    colors = _colors(2)
    full = R.canvas(kps, LIMBS, colors, hs, ws, 3, 255)
    want = full[:, nearest_table(hs, ht)][:, :, nearest_table(ws, wt)]
    assert np.array_equal(want, np.stack([R.resize_nearest(c, ht, wt) for c in full]))
    got = _frames(kps, src, LIMBS, colors.tolist(), target_size=dst)
    assert tuple(got.shape) == (3, ht, wt, 3)
    assert np.array_equal(got.cpu().numpy(), want)
    assert (want != 255).any() and (kps[2, :, 0] < 0).any()


def test_leading_dimensions_and_the_default_colours():
    from behavior_driven_video_synthesis_amd.lib.utils import H36M_LIMBS, skeleton_colors
    rng = np.random.default_rng(8)
    kps = _person(rng, 6, 100, 90).reshape(2, 3, 17, 2)
    got = _frames(kps, (100, 90), target_size=(32, 32), background=0)
    want = R.frames(kps.reshape(6, 17, 2), H36M_LIMBS, skeleton_colors(), (100, 90), (32, 32), background=0)["skel"]
    assert tuple(got.shape) == (2, 3, 32, 32, 3) and np.array_equal(got.cpu().numpy().reshape(6, 32, 32, 3), want)


# ---- 3. crop, 4. overlay
@pytest.mark.parametrize("src,size,tw,subset", [((1002, 1000), 256, 128, None), ((1002, 1000), 256, 128, [0, 3, 6, 8]),
                                                ((37, 53), 16, 8, None), ((37, 53), 16, 8, [16, 2])])
def test_crop_spans_strips_and_overlays(src, size, tw, subset):
    """The person at the left edge, the right edge and the centre (and two in between); both spans equal numpy's, the skeleton
    and rgb strips equal the sliced reference, and the overlay shows the rgb frame exactly where the skeleton VALUE is
    (255, 255, 255) -- one limb is drawn in that colour, and the random rgb frames contain 255s."""
    rng = np.random.default_rng(size + tw)
    hs, ws = src
    kps = _person(rng, 5, hs, ws, cx=[0.02 * ws, 0.98 * ws, 0.4 * ws, 0.3 * ws, 0.55 * ws])
    colors = _colors(3)
    colors[5] = 255
    rgb = rng.integers(0, 256, size=(5, size, size, 3)).astype(np.uint8)
    rgb[:, ::3, ::2] = 255
    want = R.frames(kps, LIMBS, colors, src, (size, size), crop=True, target_width=tw, crop_joints=subset, rgb=rgb, overlay=True)
    skel, span, strip, over = _frames(kps, src, LIMBS, colors.tolist(), target_size=(size, size), crop=True, target_width=tw,
                                      crop_joints=subset, rgb=torch.from_numpy(rgb).cuda(), overlay=True)
    assert span.dtype == torch.int32 and np.array_equal(span.cpu().numpy(), want["span"])
    assert want["span"][0, 0, 0] == 0 and want["span"][1, 0, 1] == size and 0 < want["span"][2, 0, 0] < size - tw
    for got, name in ((skel, "skel"), (strip, "rgb"), (over, "overlay")):
        assert tuple(got.shape) == (5, size, tw, 3) and np.array_equal(got.cpu().numpy(), want[name]), name
    white = (want["skel"] == 255).all(axis=-1)
    assert (want["overlay"][white] != 255).any() and (want["overlay"][~white] == want["skel"][~white]).all()
    # the skeleton strip alone: the same frames and skeleton span, no rgb span
    alone, span0 = _frames(kps, src, LIMBS, colors.tolist(), target_size=(size, size), crop=True, target_width=tw, crop_joints=subset)
    assert torch.equal(alone, skel) and torch.equal(span0[:, 0], span[:, 0]) and int(span0[:, 1].abs().max()) == 0


def test_overlay_without_a_crop():
    rng = np.random.default_rng(4)
    kps = _person(rng, 2, 120, 100)
    colors = _colors(5)
    colors[::2] = 255
    rgb = rng.integers(0, 256, size=(2, 31, 30, 3)).astype(np.uint8)
    rgb[:, :, ::4] = 255
    want = R.frames(kps, LIMBS, colors, (120, 100), (31, 30), rgb=rgb, overlay=True)
    skel, over = _frames(kps, (120, 100), LIMBS, colors.tolist(), target_size=(31, 30), rgb=torch.from_numpy(rgb).cuda(), overlay=True)
    assert np.array_equal(skel.cpu().numpy(), want["skel"]) and np.array_equal(over.cpu().numpy(), want["overlay"])
    assert (want["overlay"] != want["skel"]).any()


# ---- 5. strided output
@pytest.mark.parametrize("wt", [16, 15])
def test_drawing_into_one_tile_of_a_grid_leaves_the_rest_alone(wt):
    rng = np.random.default_rng(6)
    kps = _person(rng, 3, 37, 53)
    colors = _colors(7).tolist()
    plain = _frames(kps, (37, 53), LIMBS, colors, target_size=(16, wt))
    grid = torch.full((3, 3 * 16, 3 * wt, 3), 77, dtype=torch.uint8, device="cuda")
    view = grid[:, 16:32, 2 * wt:3 * wt]
    ret = _frames(kps, (37, 53), LIMBS, colors, target_size=(16, wt), out=view)
    assert ret.data_ptr() == view.data_ptr()
    assert torch.equal(view, plain) and bool((plain != 255).any())
    grid[:, 16:32, 2 * wt:3 * wt] = 77
    assert bool((grid == 77).all())


# ---- 6. edge cases
def test_no_limbs_give_background_frames_and_no_frames_no_launch():
    kps = np.zeros((2, 17, 2), dtype=np.float32)
    got = _frames(kps, (37, 53), [], [], target_size=(16, 15), background=9)
    assert tuple(got.shape) == (2, 16, 15, 3) and bool((got == 9).all())
    empty = _frames(np.zeros((0, 17, 2), dtype=np.float32), (37, 53), target_size=(16, 16))
    assert tuple(empty.shape) == (0, 16, 16, 3)
    frames, span = _frames(np.zeros((0, 17, 2), dtype=np.float32), (37, 53), target_size=(16, 16), crop=True, target_width=8)
    assert tuple(frames.shape) == (0, 16, 8, 3) and tuple(span.shape) == (0, 2, 2)
    with pytest.raises(ValueError, match="colours"):
        _frames(kps, (37, 53), [(0, 1)], [(1, 2, 3), (4, 5, 6)])
    with pytest.raises(ValueError, match="joint"):
        _frames(kps, (37, 53), [(0, 17)], [(1, 2, 3)])
    with pytest.raises(RuntimeError, match="vunet_skeleton_raster"):
        _frames(kps, (37, 53), [(0, 1)], [(1, 2, 3)], thickness=80)


# ---- 7. project_image, add_joints_to_img
def test_project_image_vs_the_float64_chain():
    """The projection launch with a scale of (1, 1) against the numpy restatement in float64, to the bound ``project`` is held to
    (tests/test_hip_seq.py: fp32 storage of pixel coordinates)."""
    from oracle import behavior_oracle as B
    from behavior_driven_video_synthesis_amd.render import PoseCamera
    rng = np.random.RandomState(11)
    dims, ignore = 51, [3, 4, 5]
    use = [i for i in range(dims) if i not in ignore]
    mean, std = rng.randn(dims) * 300.0, 50.0 + 200.0 * rng.rand(dims)
    ang = 0.4
    rot = np.array([[np.cos(ang), 0.0, np.sin(ang)], [0.0, 1.0, 0.0], [-np.sin(ang), 0.0, np.cos(ang)]])
    ext = np.concatenate([rot, np.array([[50.0], [-120.0], [5200.0]])], axis=1)
    intr = (1145.0, 512.5, 1143.8, 515.4)
    x = rng.randn(37, len(use)).astype(np.float32)
    ref = B.poses_to_keypoints(x, mean, std, ignore, ext, intr, (1.0, 1.0), 1)        # size / image size = 1: image pixels
    cam = PoseCamera(mean, std, use, ext, intr, (1000, 1002), 256)
    assert cam.image_size == (1000, 1002)
    xs = torch.from_numpy(x).cuda()
    got = cam.project_image(xs)
    assert got.shape == (37, 17, 2) and got.dtype == torch.float32
    np.testing.assert_allclose(got.cpu().numpy(), ref, rtol=2e-6, atol=2e-4)
    np.testing.assert_allclose(cam.project(xs).cpu().numpy(), B.poses_to_keypoints(x, mean, std, ignore, ext, intr, (1000, 1002), 256),
                               rtol=2e-6, atol=2e-4)                                   # project itself is untouched


def test_add_joints_to_img_reference_signature():
    from behavior_driven_video_synthesis_amd.lib.utils import H36M_LIMBS, add_joints_to_img, skeleton_colors
    kps = _person(np.random.default_rng(12), 1, 64, 48)[0]
    img = add_joints_to_img(np.zeros((64, 48, 3), np.uint8).shape, kps, H36M_LIMBS, skeleton_colors(), skeleton_colors())
    assert img.shape == (64, 48, 3) and img.dtype == np.uint8
    assert np.array_equal(img, R.canvas(kps[None], H36M_LIMBS, skeleton_colors(), 64, 48, 3, 0)[0])
    one = add_joints_to_img((64, 48, 3), kps, H36M_LIMBS, None, [[9, 8, 7]], background=255)
    assert np.array_equal(one, R.canvas(kps[None], H36M_LIMBS, [[9, 8, 7]] * 16, 64, 48, 3, 255)[0])


# ---- 8. skeleton_video, 9. transfer_grid
def _net_and_camera():
    from test_hip_behavior_interp import _camera, _small_net
    return _small_net(51, 23), _camera()


def test_skeleton_video_on_the_poses_transfer_video_returns():
    from synth import seeded_randn
    from behavior_driven_video_synthesis_amd.render import skeleton_frames, skeleton_video, transfer_video
    net, cam = _net_and_camera()
    beh, start = (0.5 * seeded_randn("skel.beh", (2, 3, 51), 23)).cuda(), (0.5 * seeded_randn("skel.start", (2, 5, 51), 23)).cuda()
    frames, poses, _ = transfer_video(net, None, None, beh, start, cam, start_frame=1)
    assert frames is None                                             # the pose-only branch of the roll-out ...
    video = skeleton_video(poses, cam, target_size=(64, 64))          # ... no longer ends there
    kps = cam.project_image(poses.reshape(-1, 51)).reshape(2, 4, 17, 2)
    assert video.dtype == torch.uint8 and tuple(video.shape) == (2, 4, 64, 64, 3)
    assert torch.equal(video, skeleton_frames(kps, cam.image_size, target_size=(64, 64)))
    from behavior_driven_video_synthesis_amd.lib.utils import H36M_LIMBS, skeleton_colors
    want = R.frames(kps.cpu().numpy().reshape(8, 17, 2), H36M_LIMBS, skeleton_colors(), (1000, 1000), (64, 64))["skel"]
    assert np.array_equal(video.cpu().numpy().reshape(8, 64, 64, 3), want) and (want != 255).any()
    rows = skeleton_video([poses, None], cam, target_size=(64, 64))
    assert rows[1] is None and torch.equal(rows[0], video)


@pytest.mark.parametrize("with_vunet", [False, True])
def test_transfer_grid_tiles_poses_and_enrollment(with_vunet):
    from synth import seeded_randn, synth_image
    from test_hip_behavior_interp import _by_hand, _small_vunet
    from behavior_driven_video_synthesis_amd.render import enrollment, skeleton_frames, transfer_grid, transfer_video
    net, cam = _net_and_camera()
    vunet = _small_vunet(23) if with_vunet else None
    app = synth_image("grid.app", (1, 3, 64, 64), 23).cuda() if with_vunet else None
    nb, ns, t, s = 2, 2, 5, 64
    beh, starts = (0.5 * seeded_randn("grid.beh", (nb, t, 51), 23)).cuda(), (0.5 * seeded_randn("grid.start", (ns, 3, 51), 23)).cuda()
    given = torch.randint(0, 256, (nb, t, s, s, 3), dtype=torch.uint8, device="cuda")
    torch.manual_seed(7)
    grid, grid_rgb, poses = transfer_grid(net, vunet, app, beh, starts, cam, behavior_frames=given, start_frame=1, target_size=(s, s))
    assert grid.dtype == torch.uint8 and tuple(grid.shape) == (t, (1 + ns) * s, (1 + nb) * s, 3) and tuple(poses.shape) == (nb, ns, t, 51)

    def tile(g, row, col):
        return g[:, row * s:(row + 1) * s, col * s:(col + 1) * s]

    assert int(tile(grid, 0, 0).max()) == 0
    for b in range(nb):
        assert torch.equal(tile(grid, 0, 1 + b), skeleton_frames(cam.project_image(beh[b]), cam.image_size, target_size=(s, s)))
        for r in range(ns):
            want = skeleton_frames(cam.project_image(poses[b, r]), cam.image_size, target_size=(s, s))
            assert torch.equal(tile(grid, 1 + r, 1 + b), want) and bool((want != 255).any())
            if b == 0:
                assert torch.equal(tile(grid, 1 + r, 0), want[:1].expand(t, s, s, 3))
    # the poses: one roll-out per (behaviour, start pose) pair through transfer_video, the start pose in front, cut to t frames
    for r in range(ns):
        _, single, _ = transfer_video(net, None, None, beh, starts[r:r + 1].expand(nb, -1, -1).contiguous(), cam, start_frame=1,
                                      length=t - 1)
        np.testing.assert_allclose(poses[:, r].cpu().numpy(), single.cpu().numpy(), **TOL)
        assert torch.equal(poses[:, r, 0], starts[r, 1].expand(nb, -1))
    if not with_vunet:
        assert grid_rgb is None
    else:
        assert grid_rgb.dtype == torch.uint8 and grid_rgb.shape == grid.shape
        assert int(tile(grid_rgb, 0, 0).min()) == 255 and all(int(tile(grid_rgb, 1 + r, 0).min()) == 255 for r in range(ns))
        torch.manual_seed(7)
        by_hand = _by_hand(vunet, app, cam, poses.transpose(0, 1).contiguous())          # the grid renders row after row
        for b in range(nb):
            assert torch.equal(tile(grid_rgb, 0, 1 + b), given[b])
            for r in range(ns):
                assert torch.equal(tile(grid_rgb, 1 + r, 1 + b), by_hand[r, b])
    row = tile(grid, 1, 1)
    still = enrollment(row, step=2)
    assert tuple(still.shape) == (s, 3 * s, 3) and torch.equal(still, torch.cat([row[0], row[2], row[4]], dim=1))
    both = enrollment(torch.stack([tile(grid, 1, 1), tile(grid, 2, 1)]), step=4)
    assert tuple(both.shape) == (2 * s, 2 * s, 3) and torch.equal(both[s:, s:], tile(grid, 2, 1)[4])
