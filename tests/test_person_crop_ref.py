"""Host tests (no GPU) of the person-box crop's restatements: the closed form the kernels implement against kornia 0.2.0's steps
taken literally, the box rule on hand-worked cases, the Inception score's statistic against the package's host function, and the
metric-tagged checkpoint's file names."""
import os

import numpy as np
import pytest
import torch

import person_crop_ref as R
from synth import seeded_randn

HS, WS = 37, 29
CASES = {"interior": (5, 7, 12, 20), "right_edge": (17, 3, 12, 30), "x0": (0, 4, 9, 11), "one_pixel_wide": (11, 6, 1, 25)}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("S", [2, 8, 16])
def test_closed_form_reference_is_kornia_literal(case, S):
    """Both sides are float64; the only difference is the 8 x 8 solve (and two 3 x 3 inverses): 1e-9 of the image maximum."""
    box = CASES[case]
    assert case != "right_edge" or box[0] + box[2] == WS      # taps past the right edge
    img = seeded_randn("person_crop.img", (1, 3, HS, WS), 3).double()
    boxes = np.asarray([box], dtype=np.int32)
    want = R.kornia_crop_literal(img, boxes, S)
    got = R.crop_closed_form(img, boxes, S, "reference")
    assert got.shape == want.shape == (1, 3, S, S)
    assert float((got - want).abs().max()) <= 1e-9 * float(img.abs().max())


def test_closed_form_exact_samples_the_box_corners():
    """EXACT: output pixel (0, 0) is the source pixel (y, x) and (S - 1, S - 1) is (y + h, x + w) -- the intended geometry."""
    img = seeded_randn("person_crop.img", (1, 3, HS, WS), 3).double()
    x, y, w, h = CASES["interior"]
    out = R.crop_closed_form(img, np.asarray([CASES["interior"]]), 8, "exact")
    assert torch.equal(out[0, :, 0, 0], img[0, :, y, x]) and torch.equal(out[0, :, 7, 7], img[0, :, y + h, x + w])


def test_box_rule_hand_worked():
    kps = np.zeros((4, 3, 2), np.float32)
    kps[0] = [[4.0, 6.0], [9.5, 7.25], [5.0, 12.0]]            # an integer-valued keypoint at the minimum: x = 4, not 3
    kps[1] = [[10.5, 11.5], [13.2, 0.0], [12.0, 30.9]]         # (13.2, 0) would widen the box to x = 13: it does not count
    kps[2] = [[0.0, 5.0], [-3.0, 2.0], [7.0, -1.0]]            # no valid keypoint
    kps[3] = [[2.9, 2.1], [2.9, 2.1], [2.9, 2.1]]              # one point: a 1 x 1 box
    boxes, valid = R.keypoint_boxes_ref(kps)
    assert valid.tolist() == [1, 1, 0, 1]
    assert boxes.tolist() == [[4, 6, 6, 7], [10, 11, 3, 20], [0, 0, 0, 0], [2, 2, 1, 1]]
    # a third coordinate <= 0 removes the keypoint as well (np.all over the whole row)
    kps3 = np.concatenate([kps, np.ones((4, 3, 1), np.float32)], axis=2)
    kps3[0, 1, 2] = 0.0
    boxes3, valid3 = R.keypoint_boxes_ref(kps3)
    assert boxes3.tolist() == [[4, 6, 2, 7], [10, 11, 3, 20], [0, 0, 0, 0], [2, 2, 1, 1]] and valid3.tolist() == [1, 1, 0, 1]


@pytest.mark.parametrize("splits", [1, 2, 3])
def test_inception_score_ref_is_the_host_statistic(splits):
    """N = 7: splits = 3 takes two rows each and drops the last row."""
    from behavior_driven_video_synthesis_amd.lib.metrics import inception_score_from_probs
    logits = 3.0 * seeded_randn("person_crop.logits", (7, 11), 5).double()
    probs = torch.softmax(logits, dim=1).numpy()
    want = inception_score_from_probs(probs, splits)
    got = R.inception_score_ref(logits.numpy(), splits)
    assert got.shape == (splits,)
    assert abs(float(np.mean(got)) - want[0]) <= 1e-12 * abs(want[0]) and abs(float(np.std(got)) - want[1]) <= 1e-12
    if splits == 3:   # the seventh row belongs to no split
        changed = logits.clone()
        changed[6] = -changed[6]
        assert np.array_equal(R.inception_score_ref(changed.numpy(), 3), got)


def test_save_metric_ckpt_file_names(tmp_path):
    from behavior_driven_video_synthesis_amd.experiments.checkpoint import save_metric_ckpt

    class Trainer:
        def __init__(self):
            self.model = torch.nn.Linear(3, 2)
            self.opt = torch.optim.Adam(self.model.parameters(), lr=1e-3)

        def state_dict(self):
            return {"model": self.model.state_dict(), "optimizer": self.opt.state_dict()}
    tr = Trainer()
    ssim, is_rec = 0.8125, 2.5
    paths = save_metric_ckpt(str(tmp_path), tr, 3, ssim, is_rec)
    save_dir = os.path.join(str(tmp_path), "epoch_ckpts")
    assert sorted(os.listdir(save_dir)) == ["model@e3@ssim=0.8125-is=2.5.pth", "opt@e3@ssim=0.8125-is=2.5.pth"]
    assert paths == (os.path.join(save_dir, "model@e3@ssim=0.8125-is=2.5.pth"), os.path.join(save_dir, "opt@e3@ssim=0.8125-is=2.5.pth"))
    fresh = torch.nn.Linear(3, 2)
    fresh.load_state_dict(torch.load(paths[0]))
    assert all(torch.equal(a, b) for a, b in zip(fresh.state_dict().values(), tr.model.state_dict().values()))
    assert set(torch.load(paths[1])) == {"state", "param_groups"}
