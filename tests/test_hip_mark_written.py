"""Raw-kernel parameter writes move version counters (``ops.mark_written``), and every weight-image cache compares one stamp
(``ops._versions``): after a writer ran, a reader that packed before it packs again, a reader nobody wrote to keeps its images,
and a backward on activations saved before the write is refused.  Comparisons between a used engine and a freshly constructed one
on the same module are bit for bit: same kernels, same inputs, same order."""
import copy

import pytest
import torch

import test_hip_blk as K                # the smallest decoder the blocked render path accepts
import test_hip_seq_passes as P         # the small behaviour net / flow and their gradients run alone
from synth import seeded_randn, synth_behavior_state, synth_image

pytestmark = pytest.mark.gpu


def _fill_grads(params, tag, seed=3):
    for i, p in enumerate(params):
        p.grad.copy_(seeded_randn(f"{tag}.{i}", tuple(p.shape), seed))


def _versions(params):
    return [p._version for p in params]


# ------------------------------------------------------------------------------------------------ the writers
@pytest.mark.parametrize("device_schedule", [False, True])
@pytest.mark.parametrize("groups", [1, 2])
def test_fused_adam_moves_every_parameters_version(groups, device_schedule):
    """One group: a bucket of its own, one launch per bucket; two groups with equal hyper-parameters: the arena, one launch.
    Each with the step count on the host and on the device: the four branches of ``step``."""
    from behavior_driven_video_synthesis_amd.optim import FusedAdam
    torch.manual_seed(2)
    a, b, other = (torch.nn.Linear(5, 7).cuda() for _ in range(3))
    params = list(a.parameters()) + list(b.parameters())
    opt = FusedAdam([{"params": params}] if groups == 1 else [{"params": list(a.parameters())}, {"params": list(b.parameters())}], lr=1e-2)
    assert (opt._arena is not None) == (groups == 2)
    if device_schedule:
        opt.use_device_schedule()
    before, before_other = _versions(params), _versions(other.parameters())
    values = [p.detach().clone() for p in params]
    _fill_grads(params, "fa.g")
    opt.step()
    assert _versions(params) == [v + 1 for v in before]
    assert all(not torch.equal(p.detach(), v) for p, v in zip(params, values))     # (the step did write them)
    opt.note_replayed_steps(2)
    assert all(now > was + 1 for now, was in zip(_versions(params), before))
    assert opt.buckets[0].step == 3
    assert _versions(other.parameters()) == before_other


def test_actnorm_initialisation_moves_the_versions_and_the_flow_engine_follows():
    from behavior_driven_video_synthesis_amd import seq
    from behavior_driven_video_synthesis_amd.lib.modules import ActNorm
    from behavior_driven_video_synthesis_amd.models.flow.simple_flow import UnsupervisedTransformer2
    with torch.no_grad():
        an = ActNorm(40, logdet=True).cuda()
        before = _versions((an.loc, an.scale))
        seq.actnorm_initialize(an, (seeded_randn("mw.an", (24, 40), 2) * 3.0 + 1.5).cuda())
        assert all(now > was for now, was in zip(_versions((an.loc, an.scale)), before))
        # a flow whose initialisation ran inside its engine's first forward: the second call sees the initialised parameters
        torch.manual_seed(4)
        flow = UnsupervisedTransformer2(flow_in_channels=32, flow_mid_channels=64, flow_hidden_depth=1, n_flows=3).cuda()
        norms = [p for blk in flow.flow.sub_layers for p in (blk.norm_layer.loc, blk.norm_layer.scale)]
        before = _versions(norms)
        x = (seeded_randn("mw.an.flow", (32, 32), 2) * 2.0 - 0.5).cuda()
        flow(x)
        assert all(now > was for now, was in zip(_versions(norms), before))
        got = flow.flow.engine().forward(x)
        want = seq.FlowEngine(flow.flow).forward(x)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ------------------------------------------------------------------------------------------------ the readers
def test_bf16_render_after_a_fused_adam_step_uses_the_new_weights():
    from behavior_driven_video_synthesis_amd.optim import FusedAdam
    from behavior_driven_video_synthesis_amd.render_blk import BlockedTransfer, engine_for
    net = K._tiny_net()
    params = list(net.du.parameters()) + list(net.dd.parameters())
    opt = FusedAdam(params, lr=5e-2)
    eng = engine_for(net)
    app = synth_image("app16", (1, 3, 64, 64), 9).cuda()
    c = synth_image("stick", (3, 3, 64, 64), 4).cuda()
    with torch.no_grad():
        code = net.appearance_code(app)
        first = eng.transfer_code(eng.encode_code(code), c)
        _fill_grads(params, "mw.render.g")
        opt.step()
        got = eng.transfer_code(eng.encode_code(code), c)
        fresh = BlockedTransfer(net)
        want = fresh.transfer_code(fresh.encode_code(code), c)
    assert torch.equal(got, want)
    assert not torch.equal(got, first)


def test_mlp_engine_after_a_fused_adam_step_uses_the_new_weights():
    from behavior_driven_video_synthesis_amd import seq
    from behavior_driven_video_synthesis_amd.lib.modules import BasicFullyConnectedNet
    from behavior_driven_video_synthesis_amd.optim import FusedAdam
    net = BasicFullyConnectedNet(dim=17, depth=2, hidden_dim=48, use_tanh=True, out_dim=9)     # (padded images: copies)
    net.load_state_dict(synth_behavior_state({k: list(v.shape) for k, v in net.state_dict().items()}, 6, {}))
    net = net.cuda()
    params = list(net.parameters())
    opt = FusedAdam(params, lr=5e-2)
    x = seeded_randn("mw.mlp.x", (70, 17), 6).cuda()
    with torch.no_grad():
        first = net(x)
        _fill_grads(params, "mw.mlp.g")
        opt.step()
        got = net(x)
        want = seq.MlpEngine(net)(x)
    assert torch.equal(got, want)
    assert not torch.equal(got, first)


@pytest.mark.parametrize("graph", [True, False])
def test_behavior_net_eval_train_eval(graph):
    """Eval under no_grad, two fused cVAE steps, eval again: the inference engine answers as a fresh one on the stepped module."""
    from behavior_driven_video_synthesis_amd import seq
    tr, _, _ = P.S._small_trainer(False, graph=graph)
    x = (0.5 * seeded_randn("mw.bn.x", (6, 7, 51), 5)).cuda()
    eps = seeded_randn("mw.bn.eps", (6, 64), 5).cuda()

    def evaluate(eng):
        with torch.no_grad():
            b, mu, logstd, pre = eng.infer_b(x, eps)
            xs, cs = eng.generate_seq(b, x, 6, 6)
        return xs, cs, b, mu, logstd, pre
    first = evaluate(tr.net.engine())
    for it in range(2):
        kps = 0.5 * seeded_randn(f"mw.bn.kps{it}", (6, 8, 51), 5)
        tr.train_fn({"keypoints": kps.cuda()}, eps=seeded_randn(f"mw.bn.eps{it}", (6, 64), 5).cuda(), sync=False)
    got, want = evaluate(tr.net.engine()), evaluate(seq.BehaviorEngine(tr.net))
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    assert not torch.equal(got[0], first[0])


def test_flow_eval_train_eval_and_the_train_engine_repacks_nothing():
    from behavior_driven_video_synthesis_amd import seq
    flow = P._flow()
    inf, eng = flow.flow.engine(), flow.flow.train_engine(lr=1e-3)
    x = seeded_randn("mw.flow.x", (17, P.FLOW["chan"]), 5).cuda()
    with torch.no_grad():
        first = inf.forward(x)
    layers = None
    for it in range(2):
        eng.train_step(seeded_randn(f"mw.flow.b{it}", (17, P.FLOW["chan"]), 5).cuda(), noise=torch.zeros(17, P.FLOW["chan"], device="cuda"))
        if layers is None:
            layers = eng._all_layers()
    now = eng._all_layers()
    assert len(now) == len(layers) and all(a is b for a, b in zip(now, layers))     # the writer took the new stamp itself
    assert eng.adam.step == 2
    with torch.no_grad():
        got, want = inf.forward(x), seq.FlowEngine(flow.flow).forward(x)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(got[0], first[0])


def test_frozen_vgg_is_packed_once_across_training_steps():
    """The perceptual loss's frozen extractor is never written: its packs and plane-weight images stay the same objects."""
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import DEFAULT_CONFIG, ShapePoseNet, synthetic_batch
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["data"]["spatial_size"] = 32
    cfg["architecture"].update(nf_start=8, nf_max=16)
    cfg["training"].update(n_init_batches=1, lr=2e-3)
    tr = ShapePoseNet(cfg, device="cuda:0", vgg_width_div=8, total_steps=50, vgg_synthetic=True)
    batch = synthetic_batch(4, 32, "cuda:0")

    def records():
        out = {}
        for name, m in tr.custom_vgg.named_modules():
            for key in ("_p2w", "_p2first"):
                rec = m.__dict__.get(key)
                if rec is not None:
                    out[(name, key)] = rec
                    for dgrad, img in getattr(rec, "_img", {}).items():
                        out[(name, key, dgrad)] = img
        for name, p in tr.custom_vgg.named_parameters():
            for sub, hit in getattr(p, "_vunet_frozen_pack", {}).items():
                out[(name, sub)] = hit
        return out
    tr.train_fn(batch)
    first = records()
    assert first
    for _ in range(2):
        tr.train_fn(batch)
    now = records()
    assert set(now) == set(first) and all(now[k] is first[k] for k in first)


# ------------------------------------------------------------------------------------------------ the tokens
def test_flow_backward_after_a_fused_step_is_refused():
    from behavior_driven_video_synthesis_amd.seq_train import STALE_WEIGHTS
    rows = 17
    flow, inp = P._flow(), P._flow_inputs("A", rows)
    eng = flow.flow.train_engine(lr=1e-3)
    _, _, token = eng.train_forward(inp["x"])
    dx, grads = eng.train_backward(token, inp["wz"], inp["wl"])                 # no step in between: the gradients of the pass alone
    want = P._flow_alone("A", rows)
    assert torch.equal(dx, want["x"])
    P._same({"flow." + n: g for n, g in grads.items()}, {n: g for n, g in want.items() if n != "x"}, "no step")
    eng.train_step(inp["x"], noise=torch.zeros_like(inp["x"]))
    with pytest.raises(RuntimeError, match=STALE_WEIGHTS.format("flow")[:60]):
        eng.train_backward(token, inp["wz"], inp["wl"])


def test_behavior_net_backward_after_a_fused_adam_step_is_refused():
    from behavior_driven_video_synthesis_amd.optim import FusedAdam
    from behavior_driven_video_synthesis_amd.seq_train import STALE_WEIGHTS
    rows, hid, t = 17, 128, 5
    net, inp = P._net(hid), P._inputs("A", rows, hid, t)
    params = list(net.parameters())
    opt = FusedAdam(params, lr=1e-3)
    loss = P._loss(P._forward(net, inp), inp)
    P._same(P._grads(net, loss, retain_graph=True), P._alone("A", rows, hid, t), "no step")
    _fill_grads(params, "mw.tok.g")
    opt.step()
    with pytest.raises(RuntimeError, match=STALE_WEIGHTS.format("behaviour net")[:60]):
        P._grads(net, loss)
    P._grads(net, P._loss(P._forward(net, inp), inp))                                # a new forward is fine again
