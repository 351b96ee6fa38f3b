"""-m gpu: the one-term ("f16") mode of the pre-split VGG19 convolutions (csrc/conv_p2_kernel.h with P2_TERMS = 1; tuning key
``p2_terms``): ONE product per tap on the hi planes of activations and weights.

The kernels are held to the float64 convolution OF THE OPERANDS THEY READ (the hi plane of the input, the hi term of the weight
image) with the bound tests/test_hip_p2.py holds the three-product kernels to, and to the unrounded float64 convolution with
the bound that two operands within 2^-11 of their values imply.  The default (two terms) must come back bit for bit after a
switch; the whole loss and one training step run in the mode end to end."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu


def _ops():
    from behavior_driven_video_synthesis_amd import ops
    return ops


def _rand(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale)


@pytest.fixture(autouse=True)
def _restore_the_dispatcher():
    yield
    ops = _ops()
    ops.set_tuning("p2_terms", 0)
    ops.set_tuning("p2_form", 0)


def _variant(ops, n, c, h, w, m):
    d = ops.P2Desc(n, c, h, w, m, 0)
    buf = ctypes.create_string_buffer(96)
    ops._call("vunet_p2_conv_variant", ctypes.byref(d), buf, 96)
    return buf.value.decode()


def _is_one_term(name):
    import re
    return re.fullmatch(r"conv_p2_kernel<4, (16|32), 1, 1>|conv_p2a_kernel<(16|32), 1>", name) is not None


def _one_term_name(form, w, m, name):
    """The variant query must report a one-term kernel, and the forced form's one."""
    ct = 16 if w == 16 else 32
    four, eight = f"conv_p2_kernel<4, {ct}, 1, 1>", f"conv_p2a_kernel<{ct}, 1>"
    if form == 1 or m % 128:
        return name == four
    if form in (2, 3):
        return name == eight
    return name in (four, eight)


def _hi_operand(planes):
    """What a one-term kernel reads of a planes tensor: its hi plane, de-scaled, as float64 NCHW."""
    n, c, h, w = planes.shape
    hi = planes.buf[0].double() / 2.0 ** int(planes.meta[0])            # [N, C / 8, H + 2, W + 2, 8]
    return hi[:, :, 1:-1, 1:-1, :].permute(0, 1, 4, 2, 3).reshape(n, c, h, w).cpu()


def _hi_weights(wt, wk):
    """The hi term of the weight image as p2_wpack_kernel rounds it: f16(w 2^ew) / 2^ew, ew = wk[2]."""
    ew = int(wk[2])
    return (wt * 2.0 ** ew).half().double() / 2.0 ** ew


def _forward_inputs(case):
    n, c, h, w, m, _ = case
    x = _rand((n, c, h, w), 11, 2.0).clamp_min(0)          # a ReLU output, like every input of the stack
    wt = _rand((m, c, 3, 3), 12, (2.0 / (9 * c)) ** 0.5)
    bias = _rand((m,), 13, 0.1)
    return x, wt, bias


def _run_forward(ops, case, x, wt, bias, terms=1):
    n, c, h, w, m, form = case
    ops.set_tuning("p2_form", form)
    ops.set_tuning("p2_terms", terms)
    px = ops.p2_from_nchw(x.cuda())
    W = ops.P2Weights(wt.cuda(), bias.cuda())
    out = ops.Planes((n, m, h, w), "cuda")
    ops.p2_conv(px, W, out)
    return px, W, out


FWD_CASES = [(1, 32, 8, 32, 64, 1), (1, 96, 8, 32, 192, 1), (2, 64, 16, 16, 128, 2), (2, 288, 8, 32, 256, 2), (4, 32, 8, 32, 128, 2),
             (1, 128, 24, 96, 64, 0)]


@pytest.mark.parametrize("case", FWD_CASES)
def test_forward_equals_the_convolution_of_the_operands_it_reads(case):
    ops = _ops()
    n, c, h, w, m, form = case
    x, wt, bias = _forward_inputs(case)
    px, W, out = _run_forward(ops, case, x, wt, bias)
    name = _variant(ops, n, c, h, w, m)
    assert _one_term_name(form, w, m, name), (case, name)              # (fails where the library has no one-term kernels)
    x_hi, w_hi = _hi_operand(px), _hi_weights(wt, W.image(False)[1].cpu())
    ref = torch.relu(torch.nn.functional.conv2d(x_hi, w_hi, bias.double(), padding=1))
    y = out.to_nchw().double().cpu()
    scale = float(ref.abs().max())
    err = float((y - ref).abs().max())
    print(f"{case}: {name}: max |y - ref| / max |ref| = {err / scale:.2e}")
    assert err <= 3e-6 * scale, (case, err / scale)
    # the published maximum bounds what was stored; the scale keeps every value below 2^14; the border stays zero
    amax = float(out.meta[16:80].view(torch.float32).max())
    assert amax >= float(y.abs().max()) * (1 - 1e-6) and amax <= scale * (1 + 1e-5)
    assert float(out.buf[0].float().abs().max()) < 2.0 ** 14
    b = out.buf
    assert float(b[:, :, :, 0].abs().max()) == 0 and float(b[:, :, :, -1].abs().max()) == 0
    assert float(b[:, :, :, :, 0].abs().max()) == 0 and float(b[:, :, :, :, -1].abs().max()) == 0
    # both output planes are written: the lo plane carries what the hi plane cannot
    assert float(b[1].float().abs().max()) > 0


@pytest.mark.parametrize("case", [(2, 64, 16, 32, 64, 1), (1, 128, 8, 64, 128, 2), (2, 128, 16, 16, 64, 0)])
def test_data_gradient_with_and_without_the_relu_mask(case):
    ops = _ops()
    n, cin, h, w, cout, form = case      # the layer maps cin -> cout; dy has cout channels, dx has cin
    dy = _rand((n, cout, h, w), 21, 1e-3)
    wt = _rand((cout, cin, 3, 3), 22, (2.0 / (9 * cin)) ** 0.5)
    act = _rand((n, cin, h, w), 23).clamp_min(0)           # the forward activation that fed the layer (a ReLU output)
    ops.set_tuning("p2_form", form)
    ops.set_tuning("p2_terms", 1)
    name = _variant(ops, n, cout, h, w, cin)
    assert _one_term_name(form, w, cin, name), (case, name)
    pdy, pact = ops.p2_from_nchw(dy.cuda()), ops.p2_from_nchw(act.cuda())
    W = ops.P2Weights(wt.cuda(), None)
    out = ops.Planes((n, cin, h, w), "cuda")
    ops.p2_conv(pdy, W, out, dgrad=True, mask=pact)
    dy_hi, w_hi = _hi_operand(pdy), _hi_weights(wt, W.image(True)[1].cpu())
    ref2 = torch.nn.functional.conv_transpose2d(dy_hi, w_hi, padding=1)
    ref = ref2 * (act > 0).double()
    y = out.to_nchw().double().cpu()
    err = float((y - ref).abs().max()) / float(ref.abs().max())
    print(f"{case}: {name}: masked data gradient, max |y - ref| / max |ref| = {err:.2e}")
    assert err <= 3e-6, (case, err)
    # masked entries are exact zeros in BOTH planes
    n_, c_, h_, w_ = out.shape
    for p in (0, 1):
        plane = out.buf[p][:, :, 1:-1, 1:-1, :].permute(0, 1, 4, 2, 3).reshape(n_, c_, h_, w_).cpu()
        assert float(plane[act == 0].abs().max()) == 0.0
    assert float(out.buf[:, :, :, 0].abs().max()) == 0 and float(out.buf[:, :, :, :, -1].abs().max()) == 0
    # without the mask
    out2 = ops.Planes((n, cin, h, w), "cuda")
    ops.p2_conv(pdy, W, out2, dgrad=True)
    err2 = float((out2.to_nchw().double().cpu() - ref2).abs().max()) / float(ref2.abs().max())
    print(f"{case}: unmasked data gradient, max |y - ref| / max |ref| = {err2:.2e}")
    assert err2 <= 3e-6, (case, err2)
    amax = float(out2.meta[16:80].view(torch.float32).max())
    assert amax >= float(out2.to_nchw().abs().max()) * (1 - 1e-6)


@pytest.mark.parametrize("case", [(1, 96, 8, 32, 192, 1), (2, 288, 8, 32, 256, 2)])
def test_distance_to_the_unrounded_convolution_stays_inside_the_derivable_bound(case):
    """Each operand the kernel reads is within 2^-11 (relative) of its value -- fp16's round-to-nearest on NORMAL numbers -- so
    every product is within (1 + 2^-11)^2 - 1 <= 2^-10 + 2^-20 of the exact one, and per output element
        |y - conv64(x, w)| <= (2^-10 + 2^-20) conv(|x|, |w|) + 3e-6 max |ref|
    (the second term: accumulation and the output's own representation, as in the test above; ReLU is 1-Lipschitz and the bias
    is not rounded).  The bound has no subnormal term: that no scaled operand is subnormal is checked on the CPU first."""
    ops = _ops()
    n, c, h, w, m, form = case
    x, wt, bias = _forward_inputs(case)
    # ---- CPU: the scaled operands (maximum in [2^13, 2^14)) hold no non-zero value below fp16's smallest normal, 2^-14
    for t in (x, wt):
        e = 14 - int(torch.frexp(t.abs().max()).exponent)
        scaled = (t * 2.0 ** e).abs()
        assert 2.0 ** 13 <= float(scaled.max()) < 2.0 ** 14
        assert bool(((scaled == 0) | (scaled >= 2.0 ** -14)).all())
    px, W, out = _run_forward(ops, case, x, wt, bias)
    assert float(_hi_operand(px)[x > 0].abs().min()) * 2.0 ** int(px.meta[0]) >= 2.0 ** -14     # (the same on the planes themselves)
    y = out.to_nchw().double().cpu()
    ref = torch.relu(torch.nn.functional.conv2d(x.double(), wt.double(), bias.double(), padding=1))
    mag = torch.nn.functional.conv2d(x.double().abs(), wt.double().abs(), padding=1)
    bound = (2.0 ** -10 + 2.0 ** -20) * mag + 3e-6 * float(ref.abs().max())
    excess = float(((y - ref).abs() - bound).max())
    print(f"{case}: max |y - conv64| / max |ref| = {float((y - ref).abs().max()) / float(ref.abs().max()):.2e}, "
          f"largest |y - conv64| / bound = {float(((y - ref).abs() / bound).max()):.3f}")
    assert excess <= 0.0, (case, excess)
    # ... and the mode IS a rounding of the operands: the result differs from the three-product kernel's
    _, _, out2 = _run_forward(ops, case, x, wt, bias, terms=2)
    assert not torch.equal(out2.buf, out.buf)


def test_the_default_is_untouched_by_a_switch_and_back():
    ops = _ops()
    case = (2, 64, 16, 32, 128, 0)
    n, c, h, w, m, _ = case
    x, wt, bias = _forward_inputs(case)
    dy = _rand((n, m, h, w), 21, 1e-3)

    def two_term():
        px, W, out = _run_forward(ops, case, x, wt, bias, terms=0)
        pdy = ops.p2_from_nchw(dy.cuda())
        g = ops.Planes((n, c, h, w), "cuda")
        ops.p2_conv(pdy, W, g, dgrad=True, mask=px)
        return out.buf.clone(), out.meta.clone(), g.buf.clone(), g.meta.clone(), _variant(ops, n, c, h, w, m)

    before = two_term()
    _, _, one = _run_forward(ops, case, x, wt, bias, terms=1)
    assert _is_one_term(_variant(ops, n, c, h, w, m)) and not torch.equal(one.buf, before[0])
    after = two_term()            # (sets p2_terms back to 0)
    assert before[4] == after[4] and not _is_one_term(before[4])
    for a, b in zip(before[:4], after[:4]):
        assert torch.equal(a, b)
    ops.set_tuning("p2_terms", 2)   # 2 is the default too
    assert _variant(ops, n, c, h, w, m) == before[4]


# ---- the whole loss.  Figures measured on an MI355X (seed 9), "f16" against "split":
#   64 x 64   the engine declines the geometry (conv4_x / conv5_x maps are 8 and 4 wide, and an engine covers a whole stack or
#             none of it): BOTH modes run the per-layer three-product path on every layer, no layer runs one-term, and the two
#             modes agree bit for bit (loss terms 0, gradient 0)
#   128 x 256 (the smallest input whose whole stack the p2 kernels cover) all 13 p2 layers one-term:
#             loss terms 4.256e-05 (max relative difference), d loss / d pred 8.582e-02 (relative L2)
#             (256 x 256: 7.08e-05 / 9.22e-02; seed 10 at 128 x 256: 4.82e-05 / 8.87e-02)
# The gradient figure is ABOVE the 5e-2 up to which the mode was to count as usable for training.  It is the forward's doing:
# with the forward in split mode and only the data gradient one-term the same figure is 7.6e-04 -- the rounded features flip
# ReLU masks, sign(p - t) and pool argmaxima, and every flip is a whole-unit change that the chain spreads over a receptive field.
LOSS_REL_MEASURED = 4.256e-05
GRAD_REL_MEASURED = 8.582e-02


def _vgg_layers(n, h, w):
    """(name, N, C, H, W, M) of the 13 convolutions of the full-width stack that the p2 engine runs (conv1_2 .. conv5_2)."""
    out, c, blk, idx = [], 64, 1, 2
    for v in [64, "M", 128, 128, "M", 256, 256, 256, 256, "M", 512, 512, 512, 512, "M", 512, 512]:
        if v == "M":
            h, w, blk, idx = h // 2, w // 2, blk + 1, 1
            continue
        out.append((f"conv{blk}_{idx}", n, c, h, w, v))
        c, idx = v, idx + 1
    return out


def _loss_and_gradient(ip, pv, target, pred0, mode):
    from behavior_driven_video_synthesis_amd.lib.losses import vgg_loss
    prev = ip.set_p2_precision(mode)
    try:
        p = pred0.clone().requires_grad_(True)
        ld = vgg_loss(pv, target, p)
        torch.stack([v.sum() for v in ld.values()]).sum().backward()
        return {k: float(v) for k, v in ld.items()}, p.grad.double().cpu()
    finally:
        ip.set_p2_precision(prev)


@pytest.mark.parametrize("size", [(64, 64), (128, 256)])
def test_whole_loss_in_f16_mode_against_split_mode(size):
    """lib.losses.vgg_loss, full-width synthetic VGG19, batch 2, "f16" against "split".  Neither tolerance can be derived (the
    gradient is discontinuous in the features: sign(p - t), pool argmax): both figures were measured on this seed and are
    asserted with a margin of 4x; they are printed.  64 x 64: the p2 engine declines the geometry, so the two modes run the same
    three-product kernels and must agree exactly; 128 x 256: every p2 layer runs one-term (see the figures above)."""
    ops = _ops()
    from behavior_driven_video_synthesis_amd.models import imagenet_pretrained as ip
    hh, ww = size
    weights = [1.0, 0.5, 1.5, 1.0, 2.0, 1.0]
    pv = ip.PerceptualVGG(ip.vgg19(seed=78, width_div=1, synthetic=True, pretrained=True), weights).cuda()
    g = torch.Generator().manual_seed(9)
    target = (torch.rand(2, 3, hh, ww, generator=g) * 2 - 1).cuda()
    pred0 = (torch.rand(2, 3, hh, ww, generator=g) * 2 - 1).cuda()
    engaged = pv._p2_engine(pred0) is not None
    # which layers run one-term, from the variant query (none where the engine declines the geometry)
    ops.set_tuning("p2_terms", 1)
    one_term = {name: _variant(ops, *geo) for name, *geo in _vgg_layers(2, hh, ww)} if engaged else {}
    ops.set_tuning("p2_terms", 0)
    print(f"{hh} x {ww}: p2 engine {'on' if engaged else 'declines the geometry'}; one-term layers: {one_term}")
    ls, gs = _loss_and_gradient(ip, pv, target, pred0, "split")
    lf, gf = _loss_and_gradient(ip, pv, target, pred0, "f16")
    assert ip.p2_precision() == "split"
    assert list(ls) == list(lf) == ["input", "relu1_2", "relu2_2", "relu3_2", "relu4_2", "relu5_2"]
    loss_rel = max(abs(lf[k] - ls[k]) / abs(ls[k]) for k in ls)
    grad_rel = float((gf - gs).norm() / gs.norm())
    print(f"{hh} x {ww}: f16 vs split: loss terms max relative difference {loss_rel:.3e}, d loss / d pred relative L2 {grad_rel:.3e}")
    if not engaged:
        assert size == (64, 64) and loss_rel == 0.0 and grad_rel == 0.0 and torch.equal(gf, gs)
        return
    assert len(one_term) == 13 and all(_is_one_term(v) for v in one_term.values()), one_term
    assert lf["input"] == ls["input"]                      # (no convolution in it)
    assert 0.0 < loss_rel <= 4 * LOSS_REL_MEASURED, loss_rel
    assert 0.0 < grad_rel <= 4 * GRAD_REL_MEASURED, grad_rel


def test_one_shape_pose_net_step_in_f16_mode_eager_and_replayed():
    """``training.vgg_precision: "f16"`` on the smallest configuration whose VGG pass reaches the p2 kernels (full-width VGG19,
    256^2 -- conv5_x needs 16-wide maps -- batch 2): the step replayed from its hipGraph equals the eagerly launched one bit for
    bit, the mode changes the loss, and a switch of the mode AFTER the capture records the step again (the mode is part of
    the graph key) instead of replaying the old kernels."""
    import copy
    ops = _ops()
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import DEFAULT_CONFIG, ShapePoseNet, synthetic_batch
    from behavior_driven_video_synthesis_amd.models import imagenet_pretrained as ip

    def run(capture, mode="f16", steps=6, then_split=2):
        ops.set_dropout_seed(777)
        cfg = copy.deepcopy(DEFAULT_CONFIG)
        cfg["training"].update(train_regressor=False, two_streams=True, n_init_batches=1, gamma_step=1e-4, information_max=50.0,
                               vgg_precision=mode)
        try:
            tr = ShapePoseNet(cfg, device="cuda:0", total_steps=1000, vgg_synthetic=True, hip_graph=False)
            assert tr.vgg_precision == mode and ip.p2_precision() == mode        # read at construction
            assert tr.custom_vgg._p2_engine(torch.empty(2, 3, 256, 256, device="cuda")) is not None
            tr.enable_hip_graph(capture=capture)
            outs = []
            for i in range(steps + then_split):
                if i == steps:
                    assert ip.set_p2_precision("split") == mode                  # the switch after the capture
                o = tr.train_fn(synthetic_batch(2, 256, "cuda:0", seed=500 + i))
                outs.append({k: float(o[k]) for k in ("loss", "likelihood_loss", "kl_loss", "gamma")})
            torch.cuda.synchronize()
            state = [(b.flat.clone(), b.grad.clone(), b.exp_avg.clone(), b.exp_avg_sq.clone()) for b in tr.optimizer.buckets]
            keys = sorted(dict(k[:1])["vgg_precision"] for k in tr._graphs)
            return outs, state, keys
        finally:
            ops.set_dropout_step(None)
            ip.set_p2_precision("split")

    oa, sa, ka = run(True)
    assert ka == ["f16", "split"], ka                     # one recording per mode: the switch recorded the step again
    ob, sb, kb = run(False)
    assert kb == []
    assert oa == ob, (oa, ob)
    assert all(o["loss"] == o["loss"] for o in oa) and len({o["loss"] for o in oa}) == len(oa)
    for (pa, ga, ma, va), (pb, gb, mb, vb), name in zip(sa, sb, ("eu", "ed", "du", "dd")):
        assert torch.equal(pa, pb), name + ": parameters"
        assert torch.equal(ga, gb), name + ": gradients of the last step"
        assert torch.equal(ma, mb) and torch.equal(va, vb), name + ": Adam moments"
    # the mode is not a no-op: the same steps in "split" mode give a different perceptual loss from the first step on
    oc, _, _ = run(False, mode="split", steps=2, then_split=0)
    assert oc[0]["likelihood_loss"] != oa[0]["likelihood_loss"]
