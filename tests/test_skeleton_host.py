"""The host side of the skeleton frames, without a GPU: the test reference itself (tests/skeleton_ref.c against the exported
stickman oracle), the nearest-neighbour tables, the host mirror of the crop rule, and the header."""
import numpy as np
import pytest

import skeleton_ref as R
from oracle import stickman as S

LIMBS = [(0, 1), (1, 2), (3, 4), (4, 5), (3, 6), (0, 6), (6, 7), (7, 8), (8, 9), (9, 10), (8, 11), (8, 14), (11, 12), (12, 13),
         (14, 15), (15, 16)]


@pytest.mark.parametrize("background", [255, 0, 37])
def test_the_wrapper_equals_the_exported_oracle_by_the_xor_construction(background):
    """On joints that are not negative (the exported oracle skips the others) the wrapper's canvas must equal the oracle driven
    through 48 commands: ``colour ^ background`` per limb and plane on its zero canvas, the result ``^ background`` -- coverage
    does not depend on the colour.  200 frames per background, thickness 1 to 6, joints up to 1.4 x the canvas."""
    rng = np.random.default_rng(background)
    h, w = 37, 53
    colors = rng.integers(0, 256, size=(len(LIMBS), 3)).astype(np.uint8)
    colors[3] = background                                # a limb in the background colour still overwrites what lies under it
    cmds = [(1, a, b, 0, p, int(colors[c, p]) ^ background) for c, (a, b) in enumerate(LIMBS) for p in range(3)]
    assert len(cmds) == 48
    for thickness in (1, 2, 3, 6):
        kps = (rng.uniform(0.0, 1.4, size=(50, 17, 2)) * (w, h)).astype(np.float32)
        want = S.raster(kps, [], cmds, h, w, thickness).transpose(0, 2, 3, 1) ^ np.uint8(background)
        got = R.canvas(kps, LIMBS, colors, h, w, thickness, background)
        assert np.array_equal(got, want), thickness
        assert (got != background).any()


def test_the_wrapper_draws_limbs_with_negative_end_points():
    kps = np.zeros((1, 17, 2), dtype=np.float32)
    kps[0, 0], kps[0, 1] = (-6.0, 4.0), (12.0, 4.0)
    got = R.canvas(kps, [(0, 1)], [(9, 8, 7)], 9, 9, 1, 255)
    assert (got[0, 4, :, 0] == 9).all() and (got[0, 3] == 255).all() and (got[0, 5] == 255).all()
    # int() truncates toward zero: -0.9 is column 0
    kps[0, 0], kps[0, 1] = (-0.9, 2.0), (-0.9, 6.0)
    got = R.canvas(kps, [(0, 1)], [(9, 8, 7)], 9, 9, 1, 0)
    assert (got[0, 2:7, 0, 1] == 8).all() and got[0, :, 1:].max() == 0


@pytest.mark.parametrize("n_src,n_dst", [(1000, 256), (1002, 256), (53, 16), (20, 64)])
def test_nearest_tables_equal_the_float64_formula(n_src, n_dst):
    from behavior_driven_video_synthesis_amd.render import nearest_table
    got = nearest_table(n_src, n_dst)
    assert got.dtype == np.int32 and got.shape == (n_dst,)
    ifx = 1.0 / (float(n_dst) / n_src)
    want = [min(int(np.floor(x * ifx)), n_src - 1) for x in range(n_dst)]
    assert got.tolist() == want == R.table(n_src, n_dst).tolist()
    assert got[0] == 0 and got.max() <= n_src - 1 and (np.diff(got) >= 0).all()


@pytest.mark.parametrize("hs,ws,size,tw,subset", [(1002, 1000, 256, 128, None), (1002, 1000, 256, 128, [0, 3, 6, 8]),
                                                  (37, 53, 16, 8, None), (37, 53, 16, 8, [16, 2])])
def test_the_host_mirror_of_the_span_rule_equals_numpy(hs, ws, size, tw, subset):
    from behavior_driven_video_synthesis_amd.render import crop_spans
    rng = np.random.default_rng(3)
    centres = np.concatenate([np.linspace(-0.2, 1.2, 40) * ws, rng.uniform(0, ws, 24)])
    kps = (centres[:, None, None] + rng.normal(0, ws / 16, size=(64, 17, 2))).astype(np.float32)
    rgb = np.zeros((64, size, size, 3), dtype=np.uint8)
    want = R.frames(kps, [], [], (hs, ws), (size, size), crop=True, target_width=tw, crop_joints=subset, rgb=rgb)["span"]
    got = crop_spans(kps, (hs, ws), (size, size), tw, subset, rgb_size=size)
    assert np.array_equal(got, want)
    assert got[:, :, 0].min() == 0 and got[:, 0, 1].max() == size and len(np.unique(got[:, 0, 0])) > 4
    assert np.array_equal(crop_spans(kps, (hs, ws), (size, size), tw, subset)[:, 0], want[:, 0])


def test_the_header_parses_and_the_colour_lists_are_the_references():
    import ctypes
    from behavior_driven_video_synthesis_amd import _lib
    from behavior_driven_video_synthesis_amd.lib.utils import H36M_LIMBS, skeleton_colors
    proto = _lib.declared_prototypes()["vunet_skeleton_raster"]
    assert len(proto) == 28 and proto.count(ctypes.c_double) == 2 and proto.count(ctypes.c_int64) == 2
    assert proto.count(ctypes.c_void_p) == 12
    assert [list(p) for p in H36M_LIMBS] == [list(p) for p in LIMBS]
    red, blue, sky = [255, 0, 0], [0, 0, 255], [0, 102, 255]
    assert skeleton_colors() == [red, red, blue, blue, blue, red, blue, blue, blue, blue, blue, red, blue, blue, red, red]
    assert skeleton_colors(overlay=True) == [sky if c == blue else c for c in skeleton_colors()]
    two = skeleton_colors([[1, 2, 3], [4, 5, 6]])
    assert two == [[1, 2, 3] if c == red else [4, 5, 6] for c in skeleton_colors()]
    assert skeleton_colors([[1, 2, 3], [4, 5, 6]], overlay=True) == skeleton_colors(overlay=True)   # (as upstream: the expanded list)
    assert skeleton_colors([[7, 7, 7]] * 16) == [[7, 7, 7]] * 16
