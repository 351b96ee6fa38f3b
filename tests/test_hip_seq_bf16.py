"""The flow's bf16 weight mode on the GPU (csrc/seq_bf16.hip, include/vunet_seq_bf16.h): bf16 weight images, fp32-accurate
products (each operand value split into three bf16 terms), against the pinned oracle run on bf16-ROUNDED weight matrices."""
import numpy as np
import pytest
import torch

from synth import seeded_randn
from test_hip_seq import FLOW_TOL, _random_flow, close

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _no_grad():
    with torch.no_grad():
        yield


def _rounded(sd):
    """The state dict the bf16 mode computes with: the coupling MLPs' weight MATRICES rounded to bf16 (round-to-nearest-even),
    biases, ActNorm and shuffles left alone."""
    return {k: (v.bfloat16().float() if ".coupling." in k and k.endswith(".weight") and v.dim() == 2 else v.clone())
            for k, v in sd.items()}


def _f64(sd):
    return {k: (v.double() if v.dtype.is_floating_point else v) for k, v in sd.items()}


def _image_index(M, K):
    """include/vunet_seq_bf16.h: the bf16 index of element (m, k) in the tile image."""
    m, k = np.meshgrid(np.arange(M), np.arange(K), indexing="ij")
    return ((m // 16) * (K // 32) + k // 32) * 512 + (((k % 32) // 8) * 16 + m % 16) * 8 + k % 8


@pytest.mark.parametrize("M,K,ld", [(16, 32, 32), (48, 96, 104), (160, 64, 64)])
def test_packer_writes_the_rounded_weights_in_the_operand_order(M, K, ld):
    from behavior_driven_video_synthesis_amd.ops import _call, _p, _stream
    w = seeded_randn(f"bf16.pack.{M}.{K}", (M, ld), 21)
    bits = w.view(torch.int32)
    # one row with the special values: +-inf, NaN, an fp32 subnormal, and exact ties between two bf16 values -- one whose even
    # neighbour is below (0x3F80 | 8000 -> 0x3F80), one whose even neighbour is above (0x3F81 | 8000 -> 0x3F82), and negative
    special = [0x7F800000, 0xFF800000, 0x7FC00000, 0x00012345, 0x3F808000, 0x3F818000, 0xBF808000, 0xBF818000, 0x807FFFFF]
    row = M - 3
    for j, v in enumerate(special):
        bits[row, 2 * j + 1] = int(np.array(v, dtype=np.uint32).view(np.int32))
    want16 = w[:, :K].bfloat16()
    # (torch's cast has no single NaN pattern -- its scalar path gives 0x7FC0, a vectorised CPU path 0xFFFF -- so the NaN of the
    #  expected image is put into the header's form, the quiet NaN 0x7FC0; every other value is torch's, bit for bit)
    assert bool(torch.isnan(want16[row, 5])) and int(torch.isnan(want16).sum()) == 1
    want16.view(torch.int16)[row, 5] = 0x7FC0
    sp = want16[row, 1:2 * len(special):2].view(torch.int16).numpy().view(np.uint16).tolist()
    assert sp == [0x7F80, 0xFF80, 0x7FC0, 0x0001, 0x3F80, 0x3F82, 0xBF80, 0xBF82, 0x8080], [hex(v) for v in sp]
    wd = w.cuda()
    img = torch.zeros(M * K, device="cuda", dtype=torch.bfloat16)
    _call("vunet_seq_pack_tiles_bf16", _p(wd), ld, M, K, _p(img), _stream())
    got = img.cpu().view(torch.int16).numpy()
    want = np.empty(M * K, dtype=np.int16)
    want[_image_index(M, K).reshape(-1)] = want16.view(torch.int16).numpy().reshape(-1)
    assert np.array_equal(got, want)


def _single_layer(w, b, x, mode):
    """y [rows, M] of one Linear through ``MlpGroup`` in weight mode ``mode``."""
    from behavior_driven_video_synthesis_amd.seq import MlpGroup
    M, K = w.shape
    g = MlpGroup([[(w.cuda(), b.cuda())]], K, [False], weights=mode)
    rows, b_pad = x.shape[0], (x.shape[0] + 15) // 16 * 16
    xin = torch.zeros(b_pad, K, device="cuda")
    xin[:rows].copy_(x)
    bufs = [torch.zeros(g.act_floats(b_pad), device="cuda") for _ in range(2)]
    y = g.run(rows, xin, K, bufs)
    return y[:b_pad * g.out_pad].view(b_pad, g.out_pad)[:rows, :M].cpu()


@pytest.mark.parametrize("operand", ["normal", "all_bits"])
@pytest.mark.parametrize("rows", [1, 16, 17])
def test_single_layer_is_the_fp32_accurate_product_with_rounded_weights(rows, operand):
    """M = 48, K = 64.  Error relative to max|y| against x.double() @ w.bfloat16().double().T + b: at most the larger of 3 x the
    fp32 kernel's own error (against its float64 product, same inputs) and 2e-6.  ``all_bits``: every operand value has all 24
    significand bits set -- a dropped third term loses 2^-16 of each value, about 2^8 times the bound."""
    M, K = 48, 64
    w = seeded_randn("bf16.lin.w", (M, K), 22) / 8.0
    b = seeded_randn("bf16.lin.b", (M,), 22)
    x = seeded_randn(f"bf16.lin.x.{rows}", (rows, K), 22)
    if operand == "all_bits":
        x = ((x.view(torch.int32) & ~0x7FFFFF) | 0x7FFFFF).view(torch.float32)   # sign and exponent kept, significand all ones
        assert bool(((x.view(torch.int32) & 0x7FFFFF) == 0x7FFFFF).all())
    y16 = _single_layer(w, b, x, "bf16")
    y32 = _single_layer(w, b, x, "f32")
    ref16 = x.double() @ w.bfloat16().double().T + b.double()
    ref32 = x.double() @ w.double().T + b.double()
    e16 = float((y16.double() - ref16).abs().max() / ref16.abs().max())
    e32 = float((y32.double() - ref32).abs().max() / ref32.abs().max())
    print(f"single layer {rows} rows ({operand}): max err / max|y|  bf16 weights {e16:.2e}  fp32 kernel {e32:.2e}")
    assert e16 <= max(3.0 * e32, 2e-6), (e16, e32)


def _run_bf16w(ops, S, layout, B, M, K, ldx, var, x, w, bias, pad, split=1):
    """One launch of vunet_seq_linear_bf16w on host-built images (``_image_index``; the operand by ``to_tiles``); returns y as
    [nets][split][Bp][M] row-major (un-tiled by ``from_tiles`` with bit 4).  Padding rows of the operand hold ``pad``."""
    import ctypes

    from test_hip_seq_kernels import Outs, _d, from_tiles, to_tiles
    nets, shared, acts, nobias = var
    b_pad = (B + 15) // 16 * 16
    xp = x.clone()
    xp[:, B:] = pad
    xop = torch.stack([to_tiles(xi[:, :K].contiguous()) for xi in xp]) if layout & 2 else xp
    idx = torch.from_numpy(_image_index(M, K).reshape(-1))
    wd = []
    for n in range(nets):
        img = torch.empty(M * K, dtype=torch.bfloat16)
        img[idx] = w[n].bfloat16().reshape(-1)
        wd.append(_d(img))
    bd = [None if nobias == n else _d(bias[n]) for n in range(nets)]
    o = Outs()
    y = o.new(nets, split, b_pad, M)
    d = S.SeqLinearDesc(B, M, K, ldx, acts[0], acts[1], nets, shared, split)
    ops._call("vunet_seq_linear_bf16w", ctypes.byref(d), layout, ops._p(wd[0]), ops._p(wd[1] if nets > 1 else None), ops._p(_d(xop)),
              ops._p(bd[0]), ops._p(bd[1] if nets > 1 else None), ops._p(y), ops._stream())
    o.check()
    y = y.cpu()
    if layout & 4:
        y = torch.stack([from_tiles(y[n].reshape(-1), b_pad, M) for n in range(nets)]).view(nets, 1, b_pad, M)
    return y


# B x K: 1, 5, 17 and 34 chunks -- one chunk, groups of 4 + 1, the 16-wave form with one wave holding two chunks, an uneven
# split over four waves -- at 1 - 4 batch tiles; then the raw split-K slabs
BF16W_CASES = [(b, k, 1) for k in (32, 160, 544, 1088) for b in (1, 17, 33, 64)] + [(b, k, s) for k, s in ((128, 2), (2048, 4))
                                                                                       for b in (16, 64)]


@pytest.mark.parametrize("B,K,split", BF16W_CASES)
def test_linear_bf16w_every_layout_vs_float64(B, K, split):
    """vunet_seq_linear_bf16w called directly.  M = 16 (layouts 1, 3) and 32 (1, 3, 5, 7); nets / shared_in / the four
    activations / a NULL bias rotate as in tests/test_hip_seq_kernels.py.  Layouts 3, 5, 7 bit-equal to layout 1 after un-tiling;
    rows < B bit-equal with the padding rows at 0 and at NaN; no unwritten output; against x.double() @ w.bfloat16().double().T
    + b through the activation, error / max|y| at most the larger of 3 x the fp32 kernel's own (same inputs, against its float64
    product) and 2e-6.  split > 1 (layouts 1, 3): RAW slabs -- the bias is given and tanh asked for, neither may be applied."""
    from behavior_driven_video_synthesis_amd import ops, seq as S
    from test_hip_seq_kernels import LINEAR_VARIANTS, NAN, _act64, _linear_operands, _run_linear, assert_same
    case = BF16W_CASES.index((B, K, split))
    kb = K // split
    for mi, M in enumerate((16, 32)):
        var = LINEAR_VARIANTS[(case * 2 + mi) % len(LINEAR_VARIANTS)] if split == 1 else ((1, 1, (2, 0), None), (2, 0, (2, 2), None))[mi]
        nets, shared, acts, nobias = var
        nin = 1 if (shared or nets == 1) else nets
        x, w, bias, ldx = _linear_operands(7000 + 10 * case + mi, B, M, K, nets, nin)
        y32, _ = _run_linear(ops, S, 0, B, M, K, ldx, var, x, w, bias, 0.0, split=split)
        base = None
        for layout in ((1, 3) if (M % 32 or split > 1) else (1, 3, 5, 7)):
            y0 = _run_bf16w(ops, S, layout, B, M, K, ldx, var, x, w, bias, 0.0, split)
            yn = _run_bf16w(ops, S, layout, B, M, K, ldx, var, x, w, bias, NAN, split)
            tag = f"B {B} M {M} K {K} S {split} layout {layout} {var}"
            assert not torch.isnan(y0).any(), f"{tag}: unwritten output"
            assert_same(yn[:, :, :B], y0[:, :, :B], f"{tag}: rows < B depend on the padding rows")
            if base is not None:
                assert_same(y0, base, f"{tag}: differs from layout 1")
                continue
            base = y0
            for n in range(nets):
                for s in range(split):
                    xi = x[n if nin > 1 else 0][:B, s * kb:(s + 1) * kb].double()
                    b64 = torch.zeros(M, dtype=torch.float64) if (nobias == n or split > 1) else bias[n].double()
                    act = 0 if split > 1 else acts[n]
                    ref16 = _act64(xi @ w[n][:, s * kb:(s + 1) * kb].bfloat16().double().t() + b64, act)
                    ref32 = _act64(xi @ w[n][:, s * kb:(s + 1) * kb].double().t() + b64, act)
                    e16 = float((y0[n, s, :B].double() - ref16).abs().max() / ref16.abs().max())
                    e32 = float((y32[n, s, :B].double() - ref32).abs().max() / ref32.abs().max())
                    print(f"{tag} net {n} slab {s}: max err / max|y|  bf16 weights {e16:.2e}  fp32 kernel {e32:.2e}")
                    assert e16 <= max(3.0 * e32, 2e-6), (tag, n, s, e16, e32)


@pytest.mark.parametrize("bsz", [1, 16, 17, 48, 64, 100])
def test_flow_vs_oracle_on_rounded_weights_over_batch_sizes(bsz):
    """Every batch-tile count of the kernel (1..4 tiles of 16 rows) and the chunking above 64 rows: forward, logdet, reverse."""
    from oracle import behavior_oracle as B
    flow, sd = _random_flow(96, 160, 2, 2, 5)
    assert flow.set_weight_precision("bf16") == "f32"
    sd16 = _rounded(sd)
    x = seeded_randn("bs16.x", (bsz, 96), 5)
    z = seeded_randn("bs16.z", (bsz, 96), 5)
    out, logdet = flow(x.cuda())
    o_ref, l_ref = B.flow_forward(sd16, x)
    close(out.reshape(bsz, 96), o_ref, **FLOW_TOL)
    close(logdet, l_ref, **FLOW_TOL)
    close(flow.reverse(z.cuda()).reshape(bsz, 96), B.flow_reverse(sd16, z), **FLOW_TOL)


def test_flow_at_the_reference_width_in_bf16_mode():
    """1024 channels, 2048 hidden, depth 2, 2 blocks, 16 rows: eager == replay bit for bit; against the float64 oracle on the
    rounded weights, next to the CPU fp32 oracle's own distance from it; the round trip.  The printed distance between the two
    MODES is a property of the weights' rounding, not a pass criterion."""
    from oracle import behavior_oracle as B
    flow, sd = _random_flow(1024, 2048, 2, 2, 9, s_gain=0.1)
    eng = flow.flow.engine()
    z = seeded_randn("full16.z", (16, 1024), 9)
    x_f32_mode = flow.reverse(z.cuda()).reshape(16, 1024).cpu()
    flow.set_weight_precision("bf16")
    sd16 = _rounded(sd)
    x_ref = B.flow_reverse(sd16, z)
    x_f64 = B.flow_reverse(_f64(sd16), z.double())
    eng.graph.enabled = False
    x_eager = flow.reverse(z.cuda())
    eng.graph.enabled = True
    x_graph = [flow.reverse(z.cuda()) for _ in range(3)][-1]
    assert torch.equal(x_eager, x_graph)
    e_hip = float((x_graph.reshape(16, 1024).cpu().double() - x_f64).abs().max() / x_f64.abs().max())
    e_cpu = float((x_ref.double() - x_f64).abs().max() / x_f64.abs().max())
    d_mode = float((x_graph.reshape(16, 1024).cpu().double() - x_f32_mode.double()).abs().max() / x_f32_mode.abs().max())
    print(f"flow reverse at 1024 / 2048 x 2 blocks, bf16 weights: max err / max|x|  HIP {e_hip:.2e}  CPU fp32 {e_cpu:.2e};  "
          f"bf16 mode vs f32 mode {d_mode:.2e}")
    assert e_hip <= max(3.0 * e_cpu, 2e-6), (e_hip, e_cpu)
    back, _ = flow(x_graph)
    close(back.reshape(16, 1024), z, rtol=1e-3, atol=2e-4)


def test_switching_modes_and_updating_weights_in_bf16_mode():
    from oracle import behavior_oracle as B
    flow, sd = _random_flow(96, 160, 2, 2, 6)
    eng = flow.flow.engine()
    z = seeded_randn("mode.z", (5, 96), 6)
    first = flow.reverse(z.cuda()).clone()
    flow.set_weight_precision("bf16")
    in16 = flow.reverse(z.cuda()).clone()
    assert not torch.equal(first, in16)
    assert all(h.wt16 is not None and h.wt is None and h.w == [] for blk in eng.blocks for h in blk["halves"])   # one mode's images
    flow.set_weight_precision("f32")
    assert torch.equal(flow.reverse(z.cuda()), first)
    assert all(h.wt16 is None for blk in eng.blocks for h in blk["halves"])
    # an in-place update in bf16 mode moves the version counters: the next call packs the new weights
    flow.set_weight_precision("bf16")
    assert torch.equal(flow.reverse(z.cuda()), in16)
    g = torch.Generator().manual_seed(6)
    for name, p in flow.named_parameters():
        if ".coupling." in name and name.endswith(".weight"):
            p.add_((0.05 * torch.randn(p.shape, generator=g)).cuda())
    new_sd = {k: v.detach().cpu() for k, v in flow.state_dict().items()}
    after = flow.reverse(z.cuda())
    assert not torch.equal(after, in16)
    close(after.reshape(5, 96), B.flow_reverse(_rounded(new_sd), z), **FLOW_TOL)
    with pytest.raises(ValueError, match="weight precision"):
        flow.set_weight_precision("fp8")
    assert flow.flow.weight_precision == "bf16"


def test_a_call_that_needs_grad_is_refused_in_bf16_mode():
    flow, _ = _random_flow(32, 48, 1, 1, 3)
    flow.set_weight_precision("bf16")
    z = torch.randn(2, 32, device="cuda")
    msg = "bf16 images are for inference only"
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match=msg):
            flow(z)                                   # trainable parameters: the autograd / training path
        with pytest.raises(RuntimeError, match=msg):
            flow.reverse(z)
        with pytest.raises(RuntimeError, match=msg):
            flow.flow.train_engine()
        for p in flow.parameters():
            p.requires_grad_(False)
        with pytest.raises(RuntimeError, match=msg):
            flow(z.clone().requires_grad_(True))      # an input that requires grad
        assert flow(z)[0].shape == (2, 32, 1, 1)      # frozen parameters, plain input: nothing to record
    flow.set_weight_precision("f32")
    for p in flow.parameters():
        p.requires_grad_(True)
    from behavior_driven_video_synthesis_amd import seq_train
    te = flow.flow.train_engine()
    flow.set_weight_precision("bf16")
    with torch.enable_grad():
        with pytest.raises(RuntimeError, match=msg):
            seq_train.flow_autograd(te, z)
        with pytest.raises(RuntimeError, match=msg):
            te._pack(z.device)


def test_behavior_video_selects_the_flow_weight_mode_for_one_call():
    from behavior_driven_video_synthesis_amd.models.pose_behavior_rnn import ResidualBehaviorNet
    from behavior_driven_video_synthesis_amd.models.vunets import VunetAlter
    from behavior_driven_video_synthesis_amd.render import PoseCamera, behavior_video
    from synth import synth_behavior_state, synth_image, synth_state_dict
    flow, _ = _random_flow(64, 96, 1, 2, 13, s_gain=0.3)
    torch.manual_seed(13)
    net = ResidualBehaviorNet(51, information_bottleneck=True, decoder_arch="lstm", linear_in_decoder=False, dim_hidden_b=64)
    nsd = synth_behavior_state({k: list(v.shape) for k, v in net.state_dict().items()}, 13, {})
    nsd["decoder.n_out.weight"] = nsd["decoder.n_out.weight"] * 0.05
    net.load_state_dict(nsd)
    net = net.cuda()
    cfg = dict(spatial_size=64, bottleneck_factor=2, box_factor=2, n_scales=0, n_latent_scales=2, conv_layer_type="l1", nf_start=8,
               nf_max=16, subpixel_upsampling=True, dropout_prob=0.0)
    vunet = VunetAlter(**cfg)
    vunet.load_state_dict(synth_state_dict({k: list(v.shape) for k, v in vunet.state_dict().items()}, 13))
    vunet = vunet.cuda().eval()
    rng = np.random.RandomState(5)
    mean = (rng.randn(51) * 250.0).astype(np.float32)
    std = (40.0 + 40.0 * rng.rand(51)).astype(np.float32)
    ext = np.concatenate([np.eye(3), np.array([[0.0], [0.0], [5000.0]])], axis=1)
    cam = PoseCamera(mean, std, list(range(51)), ext, (1145.0, 500.0, 1145.0, 500.0), (1000, 1000), 64)
    bsz, t_in, length = 2, 5, 3
    start = (0.5 * seeded_randn("e2e16.start", (bsz, t_in, 51), 13)).cuda()
    z = seeded_randn("e2e16.z", (bsz, 64), 13).cuda()
    app = synth_image("e2e16.app", (1, 3, 64, 64), 13).cuda()
    kw = dict(z=z, dtype="f32", share_appearance=False)
    torch.manual_seed(31)          # (the renderer draws its latent noise per call: the same draw for both)
    plain = behavior_video(flow, net, vunet, app, start, length, cam, **kw)
    torch.manual_seed(31)
    keyed = behavior_video(flow, net, vunet, app, start, length, cam, flow_weights="f32", **kw)
    assert all(torch.equal(a, b) for a, b in zip(plain, keyed))
    frames, poses, kps = behavior_video(flow, net, vunet, app, start, length, cam, flow_weights="bf16", **kw)
    assert flow.flow.weight_precision == "f32"                      # the previous mode is back
    assert frames.shape == plain[0].shape and not torch.equal(poses, plain[1])
    flow.set_weight_precision("bf16")
    b16 = flow.reverse(z).reshape(bsz, -1)
    flow.set_weight_precision("f32")
    by_hand, *_ = net.generate_seq(b16, start, len=length, start_frame=t_in - 1)
    assert torch.equal(poses, by_hand)
    assert torch.equal(kps, cam.project(by_hand.reshape(bsz * length, -1)).reshape(bsz, length, -1, 2))
    with pytest.raises(ValueError, match="weight precision"):
        behavior_video(flow, net, vunet, app, start, length, cam, flow_weights="fp8", **kw)
