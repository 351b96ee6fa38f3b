"""GPU parity of the Inception-v3 path (csrc/inception.hip, models/inception.py) against float64 ATen on the CPU: the general
convolution layer by layer at the network's real channel counts, the pools, the resize-to-299 input kernel, the whole network
from a random state dict (tests/inception_ref.py), the FID path and the two drivers of lib/metrics.py.

No golden fixture exists: the reference takes the network from torchvision, which is absent, so nothing of the reference's can
be run; the float64 restatement is the reference."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import inception_ref as R
from hip_parity_utils import assert_close

pytestmark = pytest.mark.gpu


def _I():
    from behavior_driven_video_synthesis_amd.models import inception
    return inception


def _ops():
    from behavior_driven_video_synthesis_amd import ops
    return ops


def gen(seed):
    return torch.Generator().manual_seed(seed)


def convg(x, w, bias, stride, pad, relu, y=None, y_coff=0, x_coff=0, tile=0):
    """vunet_convg on device tensors: x [N, x_ctot, H, W] (channels [x_coff, x_coff + C)), w [M, C, KH, KW] -> y (a new tensor, or
    the channel slice [y_coff, y_coff + M) of ``y``)."""
    I, ops = _I(), _ops()
    n, x_ctot, h, wd = x.shape
    m, cin, kh, kw = w.shape
    (sh, sw), (ph, pw) = I._pair(stride), I._pair(pad)
    ho, wo = I._out(h, kh, sh, ph), I._out(wd, kw, sw, pw)
    if y is None:
        y = torch.empty(n, m, ho, wo, device=x.device)
    wp = I.pack_weight(w.double().cpu()).to(x.device)
    d = I.ConvgDesc(n, cin, h, wd, m, ho, wo, kh, kw, sh, sw, ph, pw, x_ctot, x_coff, y.shape[1], y_coff, int(relu), wp.shape[0],
                    wp.shape[1], tile)
    b = None if bias is None else bias.to(x.device).contiguous()
    ops._call("vunet_convg", ctypes.byref(d), ops._p(x), ops._p(wp), ops._p(b), ops._p(y), ops._stream())
    return y


# (cin, cout, kernel, stride, pad, H, W): the network's channel counts on small maps (the issue's table)
LAYERS = {
    "1a_3to32_s2": (3, 32, (3, 3), 2, 0, 19, 21),
    "3b_64to80_1x1": (64, 80, (1, 1), 1, 0, 7, 9),
    "4a_80to192": (80, 192, (3, 3), 1, 0, 11, 11),
    "5x5_48to64": (48, 64, (5, 5), 1, 2, 9, 9),
    "6a_288to384_s2": (288, 384, (3, 3), 2, 0, 9, 9),
    "1x7_160": (160, 160, (1, 7), 1, (0, 3), 17, 17),
    "7x1_160": (160, 160, (7, 1), 1, (3, 0), 17, 17),
    "448to384_p1": (448, 384, (3, 3), 1, 1, 8, 8),
    "1x3_384": (384, 384, (1, 3), 1, (0, 1), 8, 8),
    "3x1_384": (384, 384, (3, 1), 1, (1, 0), 8, 8),
    "2048to320_1x1": (2048, 320, (1, 1), 1, 0, 8, 8),
    "768to192_at_1x1": (768, 192, (1, 1), 1, 0, 1, 1),
}


def layer_case(name, n=2):
    cin, cout, k, s, p, h, w = LAYERS[name]
    g = gen(sum(map(ord, name)))
    kk = cin * k[0] * k[1]
    x = torch.randn(n, cin, h, w, generator=g)
    wt = torch.randn(cout, cin, *k, generator=g) / kk ** 0.5
    b = 0.1 * torch.randn(cout, generator=g)
    ref = F.relu(F.conv2d(x.double(), wt.double(), b.double(), stride=s, padding=p))
    return x, wt, b, s, p, ref


@pytest.mark.parametrize("tile", [64, 32])
@pytest.mark.parametrize("name", list(LAYERS))
def test_single_layers_match_float64_conv2d(name, tile):
    x, wt, b, s, p, ref = layer_case(name)
    y = convg(x.cuda(), wt.cuda(), b, s, p, True, tile=tile)
    assert_close(y, ref, name=f"{name} tile {tile}")
    assert torch.equal(convg(x.cuda(), wt.cuda(), b, s, p, True, tile=tile), y)      # bit-identical from run to run


def test_the_tile_the_library_picks():
    """tile = 0: 64 x 64 where M > 32 and that makes at least 512 workgroups, else 32 x 32 -- and the result is that tile's, bit
    for bit."""
    I = _I()
    from behavior_driven_video_synthesis_amd import _lib
    tile_of = _lib.lib().vunet_convg_tile
    # 64 -> M on 7 x 9 (63 pixels per image): N = 2 -> 2 x 2 tiles of 64; 260 -> 256 x 2 = 512; 259 -> 255 x 2; M = 32: never 64
    for n, m, want in ((2, 80, 32), (260, 80, 64), (259, 80, 32), (600, 32, 32)):
        d = I.ConvgDesc(n, 64, 7, 9, m, 7, 9, 1, 1, 1, 1, 0, 0, 64, 0, m, 0, 1, 64, 128, 0)
        assert tile_of(ctypes.byref(d)) == want, (n, m)
    x, wt, b, s, p, _ = layer_case("3b_64to80_1x1")
    assert torch.equal(convg(x.cuda(), wt.cuda(), b, s, p, True, tile=0), convg(x.cuda(), wt.cuda(), b, s, p, True, tile=32))


def test_fc_layer_is_a_1x1_map_without_relu():
    g = gen(11)
    x = torch.randn(2, 2048, generator=g)
    wt, b = torch.randn(1000, 2048, generator=g) / 2048 ** 0.5, 0.1 * torch.randn(1000, generator=g)
    ref = F.linear(x.double(), wt.double(), b.double())
    y = convg(x.view(2, 2048, 1, 1).cuda(), wt.view(1000, 2048, 1, 1).cuda(), b, 1, 0, False)
    assert float(ref.min()) < -0.5          # no ReLU: negative outputs survive
    assert_close(y.view(2, 1000), ref, name="fc")
    y2 = convg(x.view(2, 2048, 1, 1).cuda(), wt.view(1000, 2048, 1, 1).cuda(), None, 1, 0, False)
    assert_close(y2.view(2, 1000), ref - b.double(), name="fc without bias")


@pytest.mark.parametrize("tile", [64, 32])
def test_channel_slices_in_and_out(tile):
    """64 -> 96, 3x3 pad 1 on 5x7, reading channels [16, 80) of a 96-channel tensor and writing channels [128, 224) of a
    256-channel tensor: the other channels keep their pre-filled values bit for bit."""
    g = gen(5)
    xw = torch.randn(2, 96, 5, 7, generator=g)
    wt, b = torch.randn(96, 64, 3, 3, generator=g) / 576 ** 0.5, 0.1 * torch.randn(96, generator=g)
    fill = torch.randn(2, 256, 5, 7, generator=g)
    y = fill.clone().cuda()
    convg(xw.cuda(), wt.cuda(), b, 1, 1, True, y=y, y_coff=128, x_coff=16, tile=tile)
    ref = F.relu(F.conv2d(xw[:, 16:80].double(), wt.double(), b.double(), padding=1))
    assert_close(y[:, 128:224], ref, name="slice")
    assert torch.equal(y[:, :128].cpu(), fill[:, :128]) and torch.equal(y[:, 224:].cpu(), fill[:, 224:])


def test_convg_refuses_inconsistent_descriptors():
    I, ops = _I(), _ops()
    from behavior_driven_video_synthesis_amd import _lib
    x, y, wp = torch.zeros(1, 4, 5, 5).cuda(), torch.zeros(1, 8, 5, 5).cuda(), torch.zeros(64, 64).cuda()
    good = [1, 4, 5, 5, 8, 5, 5, 3, 3, 1, 1, 1, 1, 4, 0, 8, 0, 1, 64, 64, 0]
    fn = _lib.lib().vunet_convg

    def rc(vals):
        return fn(ctypes.byref(I.ConvgDesc(*vals)), ops._p(x), ops._p(wp), None, ops._p(y), ops._stream())
    assert rc(good) == 0
    for idx, val in ((5, 4), (14, 1), (16, 1), (18, 32), (18, 40), (19, 32), (20, 48), (9, 0)):   # Ho, x_coff, y_coff, Kpad, Kpad, Mpad, tile, stride
        bad = list(good)
        bad[idx] = val
        assert rc(bad) == -1, (idx, val)
    torch.cuda.synchronize()


# ---- pools ---------------------------------------------------------------------------------------------------
def pool(x, stride, pad, mode, y=None, y_coff=0):
    I, ops = _I(), _ops()
    n, c, h, w = x.shape
    ho, wo = I._out(h, 3, stride, pad), I._out(w, 3, stride, pad)
    if y is None:
        y = torch.empty(n, c, ho, wo, device=x.device)
    d = I.Pool2dDesc(n, c, h, w, ho, wo, stride, pad, mode, c, 0, y.shape[1], y_coff)
    ops._call("vunet_pool2d", ctypes.byref(d), ops._p(x), ops._p(y), ops._stream())
    return y


@pytest.mark.parametrize("hw", [(35, 33), (3, 3)])
@pytest.mark.parametrize("kind", ["avg_s1_p1", "avg_s2_p0", "max_s2_p0"])
def test_pools_with_channel_slice_output(kind, hw):
    g = gen(hw[0])
    x = torch.randn(2, 5, *hw, generator=g)
    if kind == "avg_s1_p1":
        ref, args = F.avg_pool2d(x.double(), 3, 1, 1), (1, 1, 1)
    elif kind == "avg_s2_p0":
        ref, args = F.avg_pool2d(x.double(), 3, 2), (2, 0, 1)
    else:
        ref, args = F.max_pool2d(x.double(), 3, 2), (2, 0, 0)
    fill = torch.randn(2, 9, *ref.shape[2:], generator=g)
    y = fill.clone().cuda()
    pool(x.cuda(), *args, y=y, y_coff=3)
    got = y[:, 3:8].cpu()
    if kind.startswith("max"):
        assert torch.equal(got.double(), ref)
    else:
        assert float((got.double() - ref).abs().max()) <= 1e-6
    assert torch.equal(y[:, :3].cpu(), fill[:, :3]) and torch.equal(y[:, 8:].cpu(), fill[:, 8:])


@pytest.mark.parametrize("hw", [64, 1, 35 * 35])
def test_global_average(hw):
    ops = _ops()
    x = torch.randn(7, hw, generator=gen(hw))
    y = torch.empty(7).cuda()
    ops._call("vunet_global_avgpool", ops._p(x.cuda()), ops._p(y), 7, hw, ops._stream())
    assert float((y.cpu().double() - x.double().mean(dim=1)).abs().max()) <= 1e-6


# ---- the input kernel ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("hw", [(128, 96), (256, 256)])
def test_input_kernel_three_modes(hw):
    """atol 2e-6: about eight roundings (2^-24 each) of values <= 1, scaled by 1 / 0.224 -- the kernel evaluates in float64 and
    rounds once, which is inside that budget."""
    I = _I()
    x = (torch.rand(2, 3, *hw, generator=gen(hw[0])) * 2.4 - 1.2)     # beyond [-1, 1]: the FID clamp acts
    x64 = x.double()
    aten = F.interpolate(x64, size=(299, 299), mode="bilinear", align_corners=False)
    for mode in ("none", "transform", "fid"):
        got = I.inception_input(x.cuda(), mode).cpu().double()
        ref = R.resize_formula(x64, mode)
        assert float((got - ref).abs().max()) <= 2e-6, mode
        via_aten = {"none": aten, "transform": R.transform_input(aten), "fid": R.fid_input(x64)}[mode]
        assert float((got - via_aten).abs().max()) <= 2e-6, mode


# ---- the whole network ---------------------------------------------------------------------------------------
_cache = {}


def nets():
    """One random state dict; the models on the GPU, the state dict in float64 and fp32 for the restatement."""
    if not _cache:
        from behavior_driven_video_synthesis_amd.models.imagenet_pretrained import FIDInceptionModel, InceptionV3
        src = InceptionV3(seed=4321)
        sd = {k: v.clone() for k, v in src.state_dict().items()}
        _cache.update(sd=sd, sd64=R.cast(sd, torch.float64), sd32=R.cast(sd, torch.float32),
                      max=InceptionV3(state_dict=sd, stem_pool="max").cuda(), avg=InceptionV3(state_dict=sd, stem_pool="avg").cuda(),
                      fid=FIDInceptionModel(state_dict=sd).cuda())
    return _cache


def noise_bar(ref64, ref32):
    """The whole-network bar: the restatement's own fp32 noise on the CPU (max deviation of its fp32 run from its float64 run,
    relative to the feature maximum), times 4 because the summation order differs per layer.  -> (relative noise, absolute bar)"""
    scale = float(ref64.abs().max())
    noise = float((ref32.double() - ref64).abs().max()) / scale
    return noise, 4.0 * noise * scale


@pytest.mark.parametrize("stem_pool", ["max", "avg"])
@pytest.mark.parametrize("hw", [(75, 75), (107, 91)])
def test_whole_network_random_state_dict(hw, stem_pool):
    """features and logits at N = 3 against the float64 restatement; bar = 4 x the restatement's own fp32 noise (noise_bar).

    Measured on an MI355X (max deviation relative to the maximum of the float64 result; CPU fp32 restatement / GPU):
    75 x 75: max features 5.7e-7 / 8.9e-7, max logits 7.9e-7 / 9.2e-7, avg features 5.3e-7 / 7.9e-7, avg logits 5.2e-7 / 8.1e-7;
    107 x 91: max features 5.9e-7 / 9.8e-7, max logits 7.1e-7 / 1.0e-6, avg features 6.6e-7 / 5.9e-7, avg logits 6.9e-7 / 1.2e-6."""
    c = nets()
    x = torch.randn(3, 3, *hw, generator=gen(hw[1]))
    net = c[stem_pool]
    for what, fn64, got in (("features", R.features, net.features(x.cuda()).cpu()), ("logits", R.logits, net(x.cuda()).cpu())):
        ref64 = fn64(c["sd64"], x.double(), stem_pool)
        ref32 = fn64(c["sd32"], x, stem_pool)
        noise, bar = noise_bar(ref64, ref32)
        err = float((got.double() - ref64).abs().max())
        print(f"whole network {hw} {stem_pool} {what}: max|ref| {float(ref64.abs().max()):.4f} cpu fp32 noise {noise:.3e} "
              f"gpu deviation {err / float(ref64.abs().max()):.3e} (bar {4 * noise:.3e})")
        assert tuple(got.shape) == tuple(ref64.shape) and torch.isfinite(got).all()
        assert err <= bar, (what, err, bar)


def test_transform_input_is_folded_into_the_first_convolution():
    from behavior_driven_video_synthesis_amd.models.imagenet_pretrained import InceptionV3
    c = nets()
    x = torch.randn(3, 3, 75, 75, generator=gen(2))
    net = InceptionV3(state_dict=c["sd"], transform_input=True).cuda()
    ref64, ref32 = R.features(c["sd64"], x.double(), transform=True), R.features(c["sd32"], x, transform=True)
    _, bar = noise_bar(ref64, ref32)
    assert float((net.features(x.cuda()).cpu().double() - ref64).abs().max()) <= bar
    assert float((ref64 - R.features(c["sd64"], x.double())).abs().max()) > 100 * bar     # the transform matters


def fid_images():
    """The 2-batch toy problem of the driver test: two batches of two 128 x 128 images, a 'model' that shifts them; the
    restatement's float64 / fp32 FID features of all eight images, computed once."""
    if "fid_ref" not in _cache:
        g = gen(99)
        batches = [{"pose_img": torch.rand(2, 3, 128, 128, generator=g) * 2.2 - 1.1, "stickman": torch.rand(2, 3, 128, 128, generator=g)}
                   for _ in range(2)]
        c = nets()
        allx = torch.cat([b["pose_img"] for b in batches] + [toy_model(b["pose_img"], b["stickman"])[0] for b in batches])
        _cache["fid_batches"] = batches
        _cache["fid_all"] = allx
        _cache["fid_ref"] = (R.fid_features(c["sd64"], allx.double()), R.fid_features(c["sd32"], allx))
    return _cache["fid_batches"], _cache["fid_all"], _cache["fid_ref"]


class ToyModel(torch.nn.Module):
    spatial_size = 128

    def forward(self, app, stickman):
        return (0.8 * app + 0.3 * stickman - 0.1,)


toy_model = ToyModel()


def test_fid_path_through_the_resize():
    """FIDInceptionModel at N = 2 from 128 x 128: same bar as the whole network; and the average stem pools are in.

    Measured on an MI355X (relative to the feature maximum, 4.14): CPU fp32 restatement 3.8e-7, GPU 2.0e-7."""
    I = _I()
    c = nets()
    _, allx, (ref64, ref32) = fid_images()
    x = allx[:2]
    got = c["fid"](x.cuda()).cpu()
    noise, bar = noise_bar(ref64[:2], ref32[:2])
    err = float((got.double() - ref64[:2]).abs().max())
    print(f"fid path: max|ref| {float(ref64[:2].abs().max()):.4f} cpu fp32 noise {noise:.3e} gpu deviation "
          f"{err / float(ref64[:2].abs().max()):.3e} (bar {4 * noise:.3e})")
    assert tuple(got.shape) == (2, 2048) and err <= bar, (err, bar)
    with_max = c["max"].features(I.inception_input(x.cuda(), "fid")).cpu()
    assert float((with_max - got).abs().max()) > 1e-2 * float(got.abs().max())


def test_drivers_run_on_the_new_modules():
    """compute_fid and inception_score with the new modules against the same drivers fed the float64 restatement's features.

    The toy problem has 4 + 4 images, which cannot support a 2048 x 2048 covariance (scipy's sqrtm of that singular product is
    tens of seconds and ill-conditioned), so the FID driver sees TWO feature dimensions of the module -- those with the largest
    variance in the restatement's features; the statistics are then smooth in the features.  The GPU features differ from the
    float64 restatement's by fp32 noise, at most the whole-network bar d (absolute, 4 x the restatement's own fp32 noise), so
    the scores agree to what d becomes in the statistics, not to float64 noise:
    * FID, every feature moving by at most d.  m = mu1 - mu2 moves by 2 d per dimension: |m|^2 by 4 |m|_1 d.  A centred feature
      moves by 2 d, a variance with standard deviation s by about 6 s d: tr S1 + tr S2 by 6 sum(s) d.  tr sqrtm(S1 S2) is
      sqrt(cond) times as sensitive as the traces, and counts twice: with cond < 1e3 (checked) 2 * 32 * 6 sum(s) d.  Together
      (4 |m|_1 + 400 sum(s)) d, sum(s) over both sets and both dimensions.
    * log-softmax moves by at most 2 d under a logit change of d, so each KL term by about 4 d: |d log IS| <= 8 d."""
    from behavior_driven_video_synthesis_amd.lib import metrics
    c = nets()
    batches, allx, (ref64, ref32) = fid_images()
    dev = [{k: v.cuda() for k, v in b.items()} for b in batches]
    dims = torch.topk(ref64.var(dim=0), 2).indices.sort().values
    calls = []

    def extractor(x):
        f = c["fid"](x)
        calls.append(f.clone())
        return f[:, dims.to(f.device)]
    fid = metrics.compute_fid(toy_model, dev, feature_extractor=extractor)
    again = metrics.compute_fid(toy_model, dev, feature_extractor=extractor)
    assert np.isfinite(fid) and fid == again
    assert all(torch.equal(a, b) for a, b in zip(calls[:4], calls[4:]))        # bit-identical from call to call
    gt, gen_ = ref64[:4, dims].numpy(), ref64[4:, dims].numpy()
    fid_ref = metrics.fid_from_features(gt, gen_)
    _, d = noise_bar(ref64, ref32)
    c1, c2 = np.cov(gt, rowvar=False), np.cov(gen_, rowvar=False)
    assert max(np.linalg.cond(c1), np.linalg.cond(c2)) < 1e3
    bar = (4 * np.abs(gt.mean(0) - gen_.mean(0)).sum() + 400 * (np.sqrt(np.diag(c1)).sum() + np.sqrt(np.diag(c2)).sum())) * d
    print(f"drivers: fid {fid!r} restatement {fid_ref!r} bar {bar:.3e}")
    assert abs(fid - fid_ref) <= bar
    # the module as it is (all 2048 dimensions) went through the driver's loop
    assert all(tuple(f.shape) == (2, 2048) and bool(torch.isfinite(f).all()) for f in calls)

    imgs = torch.rand(6, 3, 75, 75, generator=gen(17)) * 2 - 1
    is_mean, is_std = metrics.inception_score(imgs, classifier=c["max"], batch_size=3, splits=2, device="cuda")
    lg64, lg32 = R.logits(c["sd64"], imgs.double()), R.logits(c["sd32"], imgs)
    ref_mean, ref_std = metrics.inception_score_from_probs(torch.softmax(lg64, dim=1).numpy(), 2)
    _, dl = noise_bar(lg64, lg32)
    print(f"drivers: inception score {is_mean!r} +- {is_std!r} restatement {ref_mean!r} +- {ref_std!r} bar {8 * dl:.3e}")
    assert np.isfinite(is_mean) and np.isfinite(is_std)
    assert abs(np.log(is_mean) - np.log(ref_mean)) <= 8 * dl
    assert metrics.inception_score(imgs, classifier=c["max"], batch_size=3, splits=2, device="cuda") == (is_mean, is_std)


def test_no_allocation_after_the_first_call_and_weights_repack_on_change():
    c = nets()
    x = torch.randn(3, 3, 75, 75, generator=gen(2)).cuda()
    net = c["max"]
    first = net.features(x).clone()
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    second = net.features(x)
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before
    assert torch.equal(first, second)
    # an in-place parameter update bumps the version stamp: the layer is folded and packed again
    w = net.Mixed_7c.branch1x1.bn.weight
    old = w.clone()
    try:
        w.mul_(0.5)
        assert not torch.equal(net.features(x)[:, :320], first[:, :320])
    finally:
        w.copy_(old)
    assert torch.equal(net.features(x), first)
