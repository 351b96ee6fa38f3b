"""-m gpu: the "f16grad" mode of the pre-split VGG19 convolutions (tuning value ``p2_terms`` = 3): the forward launches are the
"split" kernels bit for bit, the data-gradient launches (no ReLU, no shift) run the one-term kernels -- four waves (two x buffers
up to 256 workgroups, ``conv_p2_kernel<4, CT, 2, 1>``, else one) unless ``p2_form`` asks for the antiphase kernel.  Loss terms
are therefore those of "split" exactly, and d loss / d pred stays within the 5e-3 (relative L2) by which the project lets its
two fp32-accurate paths differ (tests/test_hip_p2.py).

Measured on an MI355X (seed 9, 128 x 256, batch 2): d loss / d pred, "f16grad" against "split": relative L2 7.592e-04; against
the fp32-tensor path 1.984e-03 (that path against "split": 1.832e-03)."""
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


def _variant(ops, n, c, h, w, m, relu):
    d = ops.P2Desc(n, c, h, w, m, relu)
    buf = ctypes.create_string_buffer(96)
    ops._call("vunet_p2_conv_variant", ctypes.byref(d), buf, 96)
    return buf.value.decode()


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
    n, c, h, w, m = case
    x = _rand((n, c, h, w), 11, 2.0).clamp_min(0)          # a ReLU output, like every input of the stack
    wt = _rand((m, c, 3, 3), 12, (2.0 / (9 * c)) ** 0.5)
    bias = _rand((m,), 13, 0.1)
    return x, wt, bias


def test_forward_is_the_split_kernel_bit_for_bit():
    ops = _ops()
    case = (2, 64, 16, 32, 128)
    n, c, h, w, m = case
    x, wt, bias = _forward_inputs(case)
    res = {}
    for terms in (0, 3, 1):
        ops.set_tuning("p2_terms", terms)
        px = ops.p2_from_nchw(x.cuda())
        W = ops.P2Weights(wt.cuda(), bias.cuda())
        out = ops.Planes((n, m, h, w), "cuda")
        ops.p2_conv(px, W, out)
        res[terms] = (out.buf.clone(), out.meta.clone(), _variant(ops, n, c, h, w, m, 1))
    assert res[3][2] == res[0][2] == "conv_p2_kernel<4, 32, 1>", res
    assert torch.equal(res[3][0], res[0][0]) and torch.equal(res[3][1], res[0][1])
    assert float(res[0][0].float().abs().max()) > 0
    assert not torch.equal(res[1][0], res[0][0])           # (the comparison can tell the arithmetics apart)


def _planes_nchw(out, p):
    n, c, h, w = out.shape
    return out.buf[p][:, :, 1:-1, 1:-1, :].permute(0, 1, 4, 2, 3).reshape(n, c, h, w).cpu()


# (N, cin, H, W, cout, p2_form) of a layer cin -> cout: dy has cout channels, dx has cin (the launch's M)
DGRAD_CASES = [(2, 64, 16, 32, 64, 0),       # M = 64: four waves only
               (1, 128, 8, 64, 128, 0), (1, 128, 8, 64, 128, 2),    # M % 128 == 0: both forms
               (2, 128, 16, 16, 64, 0),      # the 16-wide tile
               (2, 64, 16, 32, 64, 1), (2, 128, 16, 16, 64, 1),     # p2_form = 1: the single x buffer
               (1, 64, 8, 32, 32, 0),        # one chunk of input channels: nothing to fetch ahead
               (256, 64, 8, 32, 32, 0), (257, 64, 8, 32, 32, 0)]    # 256 workgroups: two x buffers; 257: one


@pytest.mark.parametrize("case", DGRAD_CASES)
def test_data_gradient_is_the_one_term_kernel(case):
    ops = _ops()
    n, cin, h, w, cout, form = case
    ct = 16 if w == 16 else 32
    dy = _rand((n, cout, h, w), 21, 1e-3)
    wt = _rand((cout, cin, 3, 3), 22, (2.0 / (9 * cin)) ** 0.5)
    act = _rand((n, cin, h, w), 23).clamp_min(0)           # the forward activation that fed the layer (a ReLU output)
    pdy, pact = ops.p2_from_nchw(dy.cuda()), ops.p2_from_nchw(act.cuda())
    W = ops.P2Weights(wt.cuda(), None)
    dy_hi, w_hi = _hi_operand(pdy), _hi_weights(wt, W.image(True)[1].cpu())
    ref_unmasked = torch.nn.functional.conv_transpose2d(dy_hi, w_hi, padding=1)
    wide = form == 2 and cin % 128 == 0
    xbuf = 2 if form != 1 and n * (h // 8) * (w // ct) * (cin // 64) <= 256 else 1
    expect = f"conv_p2a_kernel<{ct}, 1>" if wide else f"conv_p2_kernel<4, {ct}, {xbuf}, 1>"
    forced = f"conv_p2a_kernel<{ct}, 1>" if wide else f"conv_p2_kernel<4, {ct}, 1, 1>"

    def launch(terms, frm, mask):
        ops.set_tuning("p2_terms", terms)
        ops.set_tuning("p2_form", frm)
        out = ops.Planes((n, cin, h, w), "cuda")
        ops.p2_conv(pdy, W, out, dgrad=True, mask=mask)
        return out, _variant(ops, n, cout, h, w, cin, 0)

    for mask in (pact, None):
        out, name = launch(3, form, mask)
        assert name == expect, (case, name)
        # ... the same bits as the "f16" mode's launch forced onto that form.  The two-buffer kernel differs from
        # conv_p2_kernel<4, CT, 1, 1> in WHEN a chunk's tile is copied only: the same fragments meet the same accumulators in
        # the same order (chunk by chunk, tap by tap), so its sums are the same bits too
        same, same_name = launch(1, 2 if wide else 1, mask)
        assert same_name == forced
        assert torch.equal(out.buf, same.buf) and torch.equal(out.meta, same.meta), (case, mask is not None)
        # ... and not the two-term kernel's
        two, two_name = launch(0, form, mask)
        assert two_name != expect and not torch.equal(two.buf, out.buf)
        ref = ref_unmasked if mask is None else ref_unmasked * (act > 0).double()
        y = out.to_nchw().double().cpu()
        err = float((y - ref).abs().max()) / float(ref.abs().max())
        print(f"{case}: {name}: {'masked' if mask is not None else 'unmasked'} data gradient, max |y - ref| / max |ref| = {err:.2e}")
        assert err <= 3e-6, (case, err)
        if mask is not None:                               # masked entries are exact zeros in BOTH planes
            for p in (0, 1):
                assert float(_planes_nchw(out, p)[act == 0].abs().max()) == 0.0
        assert float(out.buf[1].float().abs().max()) > 0   # both planes are written
        b = out.buf                                        # the border stays zero
        assert float(b[:, :, :, 0].abs().max()) == 0 and float(b[:, :, :, -1].abs().max()) == 0
        assert float(b[:, :, :, :, 0].abs().max()) == 0 and float(b[:, :, :, :, -1].abs().max()) == 0
        # the published maximum bounds what was stored
        amax = float(out.meta[16:80].view(torch.float32).max())
        assert amax >= float(y.abs().max()) * (1 - 1e-6) and amax <= float(ref_unmasked.abs().max()) * (1 + 1e-5)
        assert float(out.buf[0].float().abs().max()) < 2.0 ** 14


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


def _is_one_term(name):
    import re
    return re.fullmatch(r"conv_p2_kernel<4, (16|32), [12], 1>|conv_p2a_kernel<(16|32), 1>", name) is not None


@pytest.mark.parametrize("size", [(64, 64), (128, 256)])
def test_whole_loss_in_f16grad_mode(size):
    """lib.losses.vgg_loss, full-width synthetic VGG19 (seed 78), batch 2, images from seed 9.  128 x 256 is the smallest input
    whose whole stack the p2 engine covers: the loss terms equal "split"'s exactly (the forward passes are the same launches),
    the gradient differs from it by 0 < rel <= 5e-3 -- the allowance tests/test_hip_p2.py gives the project's two fp32-accurate
    paths -- and against the fp32-tensor path the mode keeps the bounds that test holds the default to (2e-6 on the loss terms,
    5e-3 on the gradient).  64 x 64: the engine declines the geometry and the mode equals "split" exactly."""
    ops = _ops()
    from behavior_driven_video_synthesis_amd.models import imagenet_pretrained as ip
    hh, ww = size
    weights = [1.0, 0.5, 1.5, 1.0, 2.0, 1.0]
    pv = ip.PerceptualVGG(ip.vgg19(seed=78, width_div=1, synthetic=True, pretrained=True), weights).cuda()
    g = torch.Generator().manual_seed(9)
    target = (torch.rand(2, 3, hh, ww, generator=g) * 2 - 1).cuda()
    pred0 = (torch.rand(2, 3, hh, ww, generator=g) * 2 - 1).cuda()
    engaged = pv._p2_engine(pred0) is not None
    ls, gs = _loss_and_gradient(ip, pv, target, pred0, "split")
    lm, gm = _loss_and_gradient(ip, pv, target, pred0, "f16grad")
    assert ip.p2_precision() == "split"
    assert list(ls) == list(lm) == ["input", "relu1_2", "relu2_2", "relu3_2", "relu4_2", "relu5_2"]
    rel = float((gm - gs).norm() / gs.norm())
    print(f"{hh} x {ww}: p2 engine {'on' if engaged else 'declines the geometry'}; f16grad vs split: d loss / d pred relative L2 {rel:.3e}")
    assert lm == ls, (lm, ls)                              # all six terms, exactly
    if not engaged:
        assert size == (64, 64) and rel == 0.0 and torch.equal(gm, gs)
        return
    assert size == (128, 256)
    # what runs where, from the variant query: forward layers (relu = 1) two-term, data gradients (relu = 0; C and M swapped) one-term
    fwd_split = {name: _variant(ops, *geo, 1) for name, *geo in _vgg_layers(2, hh, ww)}
    ops.set_tuning("p2_terms", 3)
    fwd = {name: _variant(ops, *geo, 1) for name, *geo in _vgg_layers(2, hh, ww)}
    grad = {name: _variant(ops, n, m, h, w, c, 0) for name, n, c, h, w, m in _vgg_layers(2, hh, ww)}
    ops.set_tuning("p2_terms", 0)
    print(f"forward: {fwd}\ndata gradient: {grad}")
    assert len(fwd) == len(grad) == 13 and fwd == fwd_split
    assert not any(_is_one_term(v) for v in fwd.values()) and all(_is_one_term(v) for v in grad.values())
    assert all(v.startswith("conv_p2_kernel<4, ") for v in grad.values()), grad
    assert 0.0 < rel <= 5e-3, rel
    # against the fp32-tensor path (the per-layer three-product kernels on fp32 NCHW tensors)
    ip.enable_p2(False)
    try:
        lt, gt = _loss_and_gradient(ip, pv, target, pred0, "split")
    finally:
        ip.enable_p2(True)
    rel_t, rel_st = float((gm - gt).norm() / gt.norm()), float((gs - gt).norm() / gt.norm())
    print(f"{hh} x {ww}: against the fp32-tensor path: f16grad {rel_t:.3e} (split: {rel_st:.3e}); loss terms "
          f"{max(abs(lm[k] - lt[k]) / abs(lt[k]) for k in lt):.2e}")
    for k in lt:
        assert abs(lm[k] - lt[k]) <= 2e-6 * abs(lt[k]), (k, lm[k], lt[k])
    assert rel_t <= 5e-3, rel_t


def test_one_shape_pose_net_step_in_f16grad_mode_eager_and_replayed():
    """``training.vgg_precision: "f16grad"`` at 256^2, batch 2 (the smallest configuration whose VGG pass reaches the p2 kernels):
    the step replayed from its hipGraph equals the eagerly launched one bit for bit, a switch of the mode AFTER the capture
    records the step again, step 0's perceptual loss is "split"'s exactly (same forward, same weights) and the parameters after
    step 1 are not (the gradient is the one-term one)."""
    import copy
    ops = _ops()
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import DEFAULT_CONFIG, ShapePoseNet, synthetic_batch
    from behavior_driven_video_synthesis_amd.models import imagenet_pretrained as ip

    def run(capture, mode="f16grad", steps=6, then_split=2):
        ops.set_dropout_seed(777)
        cfg = copy.deepcopy(DEFAULT_CONFIG)
        cfg["training"].update(train_regressor=False, two_streams=True, n_init_batches=1, gamma_step=1e-4, information_max=50.0,
                               vgg_precision=mode)
        try:
            tr = ShapePoseNet(cfg, device="cuda:0", total_steps=1000, vgg_synthetic=True, hip_graph=False)
            assert tr.vgg_precision == mode and ip.p2_precision() == mode        # read at construction
            assert tr.custom_vgg._p2_engine(torch.empty(2, 3, 256, 256, device="cuda")) is not None
            tr.enable_hip_graph(capture=capture)
            outs, after_step_1 = [], None
            for i in range(steps + then_split):
                if i == steps:
                    assert ip.set_p2_precision("split") == mode                  # the switch after the capture
                o = tr.train_fn(synthetic_batch(2, 256, "cuda:0", seed=500 + i))
                outs.append({k: float(o[k]) for k in ("loss", "likelihood_loss", "kl_loss", "gamma")})
                if i == 1:
                    after_step_1 = [b.flat.clone() for b in tr.optimizer.buckets]
            torch.cuda.synchronize()
            state = [(b.flat.clone(), b.grad.clone(), b.exp_avg.clone(), b.exp_avg_sq.clone()) for b in tr.optimizer.buckets]
            keys = sorted(dict(k[:1])["vgg_precision"] for k in tr._graphs)
            return outs, state, keys, after_step_1
        finally:
            ops.set_dropout_step(None)
            ip.set_p2_precision("split")

    oa, sa, ka, _ = run(True)
    assert ka == ["f16grad", "split"], ka                 # one recording per mode: the switch recorded the step again
    ob, sb, kb, pb1 = run(False)
    assert kb == []
    assert oa == ob, (oa, ob)
    assert all(o["loss"] == o["loss"] for o in oa) and len({o["loss"] for o in oa}) == len(oa)
    for (pa, ga, ma, va), (pb, gb, mb, vb), name in zip(sa, sb, ("eu", "ed", "du", "dd")):
        assert torch.equal(pa, pb), name + ": parameters"
        assert torch.equal(ga, gb), name + ": gradients of the last step"
        assert torch.equal(ma, mb) and torch.equal(va, vb), name + ": Adam moments"
    # against "split": the same forward on the same weights in step 0, another gradient from there on
    oc, _, _, pc1 = run(False, mode="split", steps=2, then_split=0)
    assert oc[0]["likelihood_loss"] == ob[0]["likelihood_loss"]
    assert any(not torch.equal(a, b) for a, b in zip(pc1, pb1))                  # parameters after step 1
