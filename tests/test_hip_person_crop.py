"""-m gpu: the person-box crop (csrc/person_crop.hip) against its float64 restatement (tests/person_crop_ref.py): the boxes, the
crop under both sampling rules, the crop fused into the Inception input, and InceptionV3 with boxes."""
import ctypes

import numpy as np
import pytest
import torch

import person_crop_ref as R
from synth import seeded_rand, seeded_randn

pytestmark = pytest.mark.gpu


def _mixed_keypoints(J, C):
    """N = 5: random poses with, where J allows, the hand-worked cases mixed in -- an integer-valued keypoint at the minimum, a
    keypoint with one coordinate <= 0 that would widen the box, an image without a valid keypoint, a single valid keypoint."""
    kps = 2.0 + 25.0 * seeded_rand(f"person_crop.kps.{J}.{C}", (5, J, C), 7)
    kps[0, 0, :2] = torch.tensor([1.0, 3.0])                     # integer-valued minimum
    kps[1, J - 1, :2] = torch.tensor([200.5, 0.0])               # y == 0: does not count, would widen x
    kps[2, :, 0] = -kps[2, :, 0]                                 # no valid keypoint
    kps[3, :, :] = -1.0
    kps[3, J // 2, :] = torch.tensor([6.75, 9.5, 1.0][:C])       # exactly one valid keypoint: a 1 x 1 box
    if C == 3:
        kps[4, 0, :] = torch.tensor([300.25, 300.25, -2.0])      # third coordinate <= 0 removes it
    return kps


@pytest.mark.parametrize("J", [17, 1])
@pytest.mark.parametrize("C", [2, 3])
def test_boxes_equal_the_restatement(J, C):
    from behavior_driven_video_synthesis_amd import person_crop
    kps = _mixed_keypoints(J, C)
    boxes, valid = person_crop.keypoint_boxes(kps.cuda())
    want_b, want_v = R.keypoint_boxes_ref(kps.numpy())
    assert boxes.dtype == torch.int32 and valid.dtype == torch.int32
    assert np.array_equal(boxes.cpu().numpy(), want_b) and np.array_equal(valid.cpu().numpy(), want_v)
    assert want_v[2] == 0 and want_b[2].tolist() == [0, 0, 0, 0]
    if J > 1:
        assert want_v.tolist() == [1, 1, 0, 1, 1] and want_b[3].tolist() == [6, 9, 1, 1]


def _boxes_for(hs, ws):
    """interior, touching each edge (the right / bottom ones reach one past the last pixel), one pixel wide, one pixel high, and a
    box whose image is not valid."""
    rows = [(3, 4, 7, 9), (0, 5, 6, 6), (ws - 8, 2, 8, 9), (4, 0, 9, 5), (2, hs - 6, 10, 6), (5, 3, 1, 10), (1, 6, 11, 1), (3, 3, 5, 5)]
    return torch.tensor(rows, dtype=torch.int32), torch.tensor([1, 1, 1, 1, 1, 1, 1, 0], dtype=torch.int32)


@pytest.mark.parametrize("shape", [(3, 16, 16), (3, 37, 29), (1, 37, 29)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("S", [2, 8, 16])
@pytest.mark.parametrize("sampling", ["reference", "exact"])
def test_crop_against_float64_restatement(shape, S, sampling):
    """The kernel's maximum error against the float64 closed form may be at most 4 x the error of the same restatement run in
    fp32 through F.grid_sample on the CPU (the kernel does the same three fp32 lerps from float64 coordinates; plain torch also
    rounds the coordinates to fp32).  Both figures are printed."""
    from behavior_driven_video_synthesis_amd import person_crop
    ch, hs, ws = shape
    boxes, valid = _boxes_for(hs, ws)
    n = boxes.shape[0]
    img = seeded_randn("person_crop.crop_img", (n, ch, hs, ws), 11)
    got = person_crop.crop_and_resize(img.cuda(), boxes.cuda(), S, valid.cuda(), sampling).cpu()
    want = R.crop_closed_form(img, boxes.numpy(), S, sampling, valid.numpy())
    fp32 = R.crop_grid_sample_fp32(img, boxes.numpy(), S, sampling)
    keep = valid.bool()
    err_kernel = float((got.double() - want).abs().max())
    err_fp32 = float((fp32.double()[keep] - want[keep]).abs().max())
    print(f"crop {shape} S={S} {sampling}: kernel max error {err_kernel:.3e}, fp32 grid_sample max error {err_fp32:.3e}")
    assert got.shape == (n, ch, S, S) and torch.all(got[~keep] == 0)
    assert err_kernel <= 4.0 * err_fp32
    # valid=None: every box counts
    all_valid = person_crop.crop_and_resize(img.cuda(), boxes.cuda(), S, None, sampling).cpu()
    assert torch.equal(all_valid[keep], got[keep])
    assert float((all_valid.double() - R.crop_closed_form(img, boxes.numpy(), S, sampling)).abs().max()) <= 4.0 * err_fp32


def test_crop_size_one_is_an_argument_error():
    from behavior_driven_video_synthesis_amd import _lib, person_crop
    img = torch.zeros(1, 3, 16, 16, device="cuda")
    boxes, valid = torch.tensor([[2, 2, 4, 4]], dtype=torch.int32).cuda(), torch.ones(1, dtype=torch.int32).cuda()
    out = torch.zeros(1, 3, 1, 1, device="cuda")

    def p(t):
        return ctypes.c_void_p(t.data_ptr())
    rc = _lib.lib().vunet_box_crop(p(img), 1, 3, 16, 16, p(boxes), p(valid), 1, 0, p(out), None)
    assert rc == -1                                              # VUNET_ERR_ARG
    y = torch.zeros(1, 3, 299, 299, device="cuda")
    assert _lib.lib().vunet_inception_input_boxes(p(img), 1, 16, 16, p(boxes), p(valid), 1, 0, 0, p(y), None) == -1
    assert _lib.lib().vunet_box_crop(p(img), 1, 3, 16, 16, p(boxes), p(valid), 4, 2, p(out), None) == -1   # unknown sampling
    with pytest.raises(ValueError):
        person_crop.crop_and_resize(img, boxes, 1)


@pytest.mark.parametrize("sampling", ["reference", "exact"])
def test_bounding_box_batch_is_boxes_then_crop(sampling):
    from behavior_driven_video_synthesis_amd import person_crop
    from behavior_driven_video_synthesis_amd.lib.utils import bounding_box_batch
    kps = _mixed_keypoints(17, 2).cuda()
    img = seeded_randn("person_crop.bbb", (5, 3, 32, 32), 13).cuda()
    sizes = torch.full((5, 2), 32)
    got = bounding_box_batch(kps, img, sizes, 32, sampling=sampling)
    boxes, valid = person_crop.keypoint_boxes(kps)
    assert got.is_cuda and got.shape == (5, 3, 32, 32)
    assert torch.equal(got, person_crop.crop_and_resize(img, boxes, 32, valid, sampling))
    assert torch.all(got[2] == 0) and not torch.all(got[0] == 0)
    if sampling == "reference":
        assert torch.equal(got, bounding_box_batch(kps, img, sizes, 32))


@pytest.mark.parametrize("shape", [(32, 32), (37, 29)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("crop_size", [32, 16])
@pytest.mark.parametrize("mode", ["none", "fid"])
@pytest.mark.parametrize("sampling", ["reference", "exact"])
def test_fused_inception_input_is_bit_identical_to_two_steps(shape, crop_size, mode, sampling):
    from behavior_driven_video_synthesis_amd import person_crop
    from behavior_driven_video_synthesis_amd.models.inception import inception_input
    hs, ws = shape
    boxes, valid = _boxes_for(hs, ws)
    img = seeded_randn("person_crop.fused", (boxes.shape[0], 3, hs, ws), 17).cuda()
    boxes, valid = boxes.cuda(), valid.cuda()
    two = inception_input(person_crop.crop_and_resize(img, boxes, crop_size, valid, sampling), mode)
    one = person_crop.inception_input_boxes(img, boxes, crop_size, valid, mode, sampling)
    assert one.shape == (boxes.shape[0], 3, 299, 299)
    assert torch.equal(one, two)


def test_inception_v3_with_boxes():
    """The boxed forward is the plain forward of the two-step input, bit for bit, and a boxed call in between does not change what
    the plain forward returns (the plan cache keeps the two apart)."""
    from behavior_driven_video_synthesis_amd import person_crop
    from behavior_driven_video_synthesis_amd.models.inception import FIDInceptionModel, InceptionV3, inception_input
    net = InceptionV3(seed=7).cuda()
    x = seeded_randn("person_crop.v3", (3, 3, 32, 32), 19).cuda()
    boxes = torch.tensor([(3, 4, 7, 9), (20, 2, 12, 25), (5, 5, 9, 9)], dtype=torch.int32).cuda()
    valid = torch.tensor([1, 1, 0], dtype=torch.int32).cuda()
    big = inception_input(x)
    plain_before = net(big).clone()
    resized_before = net(x, resize=True).clone()
    assert torch.equal(plain_before, resized_before)
    for sampling in ("reference", "exact"):
        got = net(x, boxes=boxes, valid=valid, crop_size=32, sampling=sampling, resize=True).clone()
        want = net(inception_input(person_crop.crop_and_resize(x, boxes, 32, valid, sampling))).clone()
        assert got.shape == (3, 1000) and torch.equal(got, want)
    assert not torch.equal(got, plain_before)
    assert torch.equal(net(big), plain_before) and torch.equal(net(x, resize=True), resized_before)
    feats = net.features(x, boxes=boxes, valid=valid, crop_size=16, resize=True).clone()
    assert torch.equal(feats, net.features(inception_input(person_crop.crop_and_resize(x, boxes, 16, valid))))
    with pytest.raises(ValueError):
        net(x, boxes=boxes, crop_size=32)                        # boxes need the resize step
    fid = FIDInceptionModel(seed=7).cuda()
    got = fid(x, boxes=boxes, valid=valid, crop_size=32).clone()
    two = inception_input(person_crop.crop_and_resize(x, boxes, 32, valid), "fid")
    assert torch.equal(got, super(FIDInceptionModel, fid).features(two))
