"""-m gpu: the training-loop surfaces (ShapePoseNet / Vunet) on tiny configs -- loss goes down, schedules and the
device-resident gamma controller follow the reference rules, checkpoints round-trip in the reference layout,
dropout is reproducible from the seed."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu


def _tiny(cfg_default, **training):
    cfg = copy.deepcopy(cfg_default)
    cfg["data"]["spatial_size"] = 32
    cfg["architecture"].update(nf_start=8, nf_max=16)
    cfg["training"].update(training)
    return cfg


def test_shape_pose_net_steps_checkpoint_and_gamma():
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import (DEFAULT_CONFIG, ShapePoseNet,
                                                                                     synthetic_batch)
    from oracle import vunet_oracle as O
    cfg = _tiny(DEFAULT_CONFIG, n_init_batches=1, gamma_step=1e-3, information_max=5.0, train_regressor=True,
                lr=2e-3)
    tr = ShapePoseNet(cfg, device="cuda:0", vgg_width_div=8, total_steps=50, vgg_synthetic=True)
    batch = synthetic_batch(4, 32, "cuda:0", with_regressor=True, reg_steps=2)
    gamma, losses = 0.0, []
    for it in range(1, 7):
        out = tr.train_fn(batch)
        losses.append(float(out["likelihood_loss"]))
        gamma = O.update_gamma(gamma, 1e-3, 5.0, float(out["kl_loss"]))
        assert abs(float(out["gamma"]) - gamma) <= 1e-5 * max(1.0, abs(gamma))   # device controller == host rule
        assert abs(out["learning_rate"] - O.linear_var(it, 0, 50, 2e-3, 0, 0, 2e-3)) < 1e-12
        assert "loss_reg" in out
    assert losses[-1] < losses[0]
    ckpt = tr.state_dict()
    # {"model", "optimizer"} = the reference's "reg_ckpt" file (:471-482); "regressor" = its second file (:483-494)
    assert set(ckpt) == {"model", "optimizer", "regressor"} and len(ckpt["model"]) == len(tr.vunet.state_dict())
    assert [g["name"] for g in ckpt["optimizer"]["param_groups"]] == ["eu", "ed", "du", "dd"]
    assert all(isinstance(g["gamma"], float) and g["gamma"] == float(tr.gamma) for g in ckpt["optimizer"]["param_groups"])
    tr2 = ShapePoseNet(cfg, device="cuda:0", vgg_width_div=8, total_steps=50, vgg_synthetic=True)
    tr2.load_state_dict(ckpt)
    # restart as the reference does (:87-95, :248-255): iteration from Adam's step, gamma from the param groups, lr / imax
    # re-derived -- the KL weight must not restart from 0
    assert tr2.iteration == 6 and float(tr2.gamma) == float(tr.gamma) and float(tr.gamma) > 0
    assert tr2.lr == tr.lr and tr2.imax == tr.imax
    for (k, a), (_, b) in zip(tr.vunet.state_dict().items(), tr2.vunet.state_dict().items()):
        assert torch.equal(a, b), k
    for (k, a), (_, b) in zip(tr.regressor.state_dict().items(), tr2.regressor.state_dict().items()):
        assert torch.equal(a, b), k
    # the step after the restart is the step the uninterrupted run takes (same dropout seeds, same noise)
    from behavior_driven_video_synthesis_amd import ops
    eps = [torch.randn(4, 16, 4, 4, device="cuda"), torch.randn(4, 16, 8, 8, device="cuda")]
    reg_eps = [[torch.randn(4, 16, 4, 4, device="cuda"), torch.randn(4, 16, 8, 8, device="cuda")] for _ in range(2)]
    ops.set_dropout_seed(99)
    o1 = tr.train_fn(batch, eps, reg_eps)
    ops.set_dropout_seed(99)
    o2 = tr2.train_fn(batch, eps, reg_eps)
    for k in ("loss", "kl_loss", "gamma", "loss_reg"):
        assert float(o1[k]) == float(o2[k]), k
    img = tr2.transfer(batch["pose_img"], batch["stickman"])
    assert img.shape == (4, 3, 32, 32) and torch.isfinite(img).all()


def test_vunet_org_loop_steps_and_kl_schedule():
    from behavior_driven_video_synthesis_amd.experiments.vunet import DEFAULT_CONFIG, Vunet
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import synthetic_batch
    cfg = _tiny(DEFAULT_CONFIG, lr=2e-3)
    cfg["architecture"].update(nf_start=4, nf_max=8)
    tr = Vunet(cfg, device="cuda:0", n_channels_x=3, vgg_width_div=8, total_steps=8, vgg_synthetic=True)
    batch = synthetic_batch(2, 32, "cuda:0")
    kls, first = [], None
    for it in range(1, 8):
        out = tr.train_fn(batch)
        first = first if first is not None else float(out["likelihood_loss"])
        kls.append(out["kl_weight"])
    assert float(out["likelihood_loss"]) < first
    assert kls[0] == pytest.approx(1e-6) and kls[-1] == pytest.approx(1.0) and kls[4] > kls[3]  # ramp between T/2 and 3T/4


def test_dropout_is_reproducible_from_the_seed():
    from behavior_driven_video_synthesis_amd import ops
    from behavior_driven_video_synthesis_amd.lib.modules import VunetRNB
    blk = VunetRNB(16, dropout_prob=0.3).cuda().train()
    x = torch.randn(2, 16, 8, 8, device="cuda")
    ops.set_dropout_seed(11)
    a = blk(x)
    b = blk(x)
    ops.set_dropout_seed(11)
    c = blk(x)
    assert torch.equal(a, c) and not torch.equal(a, b)


def test_shape_pose_net_with_adversarial_term():
    """training.gan: generator loss through the PartDiscriminator + one discriminator step per iteration (the
    reference ships the pieces, models/synth_discriminator.py:115-242, but never wires them -- SURVEY F2)."""
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import (DEFAULT_CONFIG, ShapePoseNet,
                                                                                     synthetic_batch)
    batch = synthetic_batch(4, 32, "cuda:0")

    def run(weight, **gan):
        cfg = _tiny(DEFAULT_CONFIG, lr=2e-3, train_regressor=False,
                    gan=dict(enabled=True, weight=weight, pd_scales=2, lr=2e-3, **gan))
        tr = ShapePoseNet(cfg, device="cuda:0", vgg_width_div=8, total_steps=50, vgg_synthetic=True)
        d0 = {k: v.clone() for k, v in tr.gan.disc.state_dict().items()}
        outs = [tr.train_fn(batch) for _ in range(6)]
        return tr, d0, outs

    tr, d0, outs = run(1.0)
    for o in outs:
        assert all(torch.isfinite(torch.as_tensor(float(o[k]))) for k in ("loss", "gen_loss", "dloss", "dloss_r", "dloss_f"))
    assert outs[-1]["dloss"] < outs[0]["dloss"]                      # the discriminator learns to tell the patches apart
    assert any(not torch.equal(v, d0[k]) for k, v in tr.gan.disc.state_dict().items())
    assert all(p.requires_grad for p in tr.vunet.parameters())       # toggle_grad restored after the disc step
    # the adversarial gradient reaches the generator: same seed, weight 0 -> different parameters after the steps
    tr0, _, _ = run(0.0)
    diff = max(float((a - b).abs().max()) for a, b in zip(tr.vunet.state_dict().values(), tr0.vunet.state_dict().values()))
    assert diff > 1e-6
    # R1 penalty + gradient-ratio weighting (autograd.grad on the output conv's weight_v) run on the same path
    tr2, _, outs2 = run(1.0, grad_pen=True, grad_weighting=True)
    assert "gp" in outs2[-1] and all(torch.isfinite(torch.as_tensor(float(o["loss"]))) for o in outs2)
    g = tr2.optimizer.buckets[0].grad
    assert torch.isfinite(g).all()


def test_second_hip_stream_changes_nothing_but_the_schedule():
    """The pose encoder runs on a second HIP stream beside the appearance encoder (forward and, through autograd's
    stream replay, backward): parameters, losses and the gamma controller must be bit-identical to the one-stream run."""
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import (DEFAULT_CONFIG, ShapePoseNet,
                                                                                     synthetic_batch)
    batch = synthetic_batch(4, 32, "cuda:0")

    def run(two):
        from behavior_driven_video_synthesis_amd import ops
        ops.set_dropout_seed(1234)          # the dropout counter is process-global: same masks for both runs
        cfg = _tiny(DEFAULT_CONFIG, lr=2e-3, n_init_batches=1, gamma_step=1e-3, information_max=5.0,
                    train_regressor=False, two_streams=two)
        tr = ShapePoseNet(cfg, device="cuda:0", vgg_width_div=8, total_steps=50, vgg_synthetic=True)
        assert (tr.vunet._side_stream is not None) == two and ops._wgrad_streams["on"] == two
        outs = [tr.train_fn(batch) for _ in range(4)]
        torch.cuda.synchronize()
        return tr, outs

    a, oa = run(True)
    b, ob = run(False)
    for x, y in zip(oa, ob):
        assert float(x["loss"]) == float(y["loss"]) and float(x["gamma"]) == float(y["gamma"])
    for (k, p), (_, q) in zip(a.vunet.state_dict().items(), b.vunet.state_dict().items()):
        assert torch.equal(p, q), k


def _drive_trajectory(name, with_regressor):
    """ShapePoseNet.train_fn ITSELF (loss assembly, n_init_batches gate, device-resident gamma, lr schedule, prepacked
    weights, fused Adam, the regressor side loop) against the trajectory recorded from the reference's modules driven by
    hand with torch.optim.Adam (tests/golden/make_golden.py g5_*)."""
    import copy
    from conftest import load_golden
    from hip_parity_utils import assert_close
    from synth import seeded_randn, synth_image, synth_state_dict
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import DEFAULT_CONFIG, ShapePoseNet
    meta, arr = load_golden(name)
    seed, R = meta["seed"], meta.get("reg_steps", 0)
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["data"]["spatial_size"] = meta["cfg"]["spatial_size"]
    cfg["architecture"].update(nf_start=meta["cfg"]["nf_start"], nf_max=meta["cfg"]["nf_max"])
    cfg["training"].update(dropout_prob=0.0, lr=meta["lr0"], adam_betas=tuple(meta["betas"]), gamma_step=meta["gamma_step"],
                           information_max=meta["imax"], n_init_batches=meta["n_init_batches"], ll_weight=1.0,
                           train_regressor=with_regressor, weight_regressor=meta.get("weight_regressor", 4.0))
    tr = ShapePoseNet(cfg, device="cuda:0", vgg_width_div=meta["vgg_width_div"], vgg_seed=meta["vgg_seed"],
                      vgg_synthetic=True, total_steps=meta["total_steps"])
    tr.vunet.load_state_dict(synth_state_dict(meta["shapes"], seed))
    if with_regressor:
        tr.regressor.load_state_dict(synth_state_dict(meta["reg_shapes"], meta["reg_seed"]))
    tr.gamma.fill_(meta["gamma0"])
    lat = [(2, 16, 4, 4), (2, 16, 8, 8)]
    pre = "rtraj" if with_regressor else "traj"
    for rec in meta["steps"]:
        it = rec["it"]
        batch = {"pose_img": synth_image(f"{pre}.x{it}", (2, 3, 32, 32), seed).cuda(),
                 "stickman": synth_image(f"{pre}.c{it}", (2, 3, 32, 32), seed).cuda()}
        eps = [seeded_randn(f"{pre}.{it}.eps{i}", s, seed).cuda() for i, s in enumerate(lat)]
        reg_eps = None
        if with_regressor:
            batch["reg_imgs"] = synth_image(f"rtraj.r{it}", (2, R, 3, 32, 32), seed).cuda()
            batch["reg_targets"] = (seeded_randn(f"rtraj.t{it}", (2, R, 17, 2), seed) * 0.25 + 0.5).cuda()
            reg_eps = [[seeded_randn(f"rtraj.{it}.reg{r}.eps{i}", s, seed).cuda() for i, s in enumerate(lat)]
                       for r in range(R)]
        assert abs(tr.lr - rec["lr"]) < 1e-12                       # the lr this step's Adam uses
        out = tr.train_fn(batch, eps, reg_eps)
        for key, want in (("loss", rec["loss"]), ("likelihood_loss", rec["ll"]), ("kl_loss", rec["kl"]),
                          ("gamma", rec["gamma_after"])):
            assert abs(float(out[key]) - want) <= 5e-4 * abs(want) + 1e-5, (it, key, float(out[key]), want)
        if with_regressor:
            assert abs(float(out["loss_reg"]) - rec["reg_losses"][-1]) <= 5e-4 * rec["reg_losses"][-1] + 1e-5
    sd = tr.vunet.state_dict()
    assert_close(sd["dd.out_conv.conv.weight_v"], arr["final.dd.out_conv.conv.weight_v"], rtol=2e-3, atol=2e-5,
                 name="final weight")
    for k, s in meta["param_checksums"].items():
        got = float(sd[k].double().abs().sum())
        assert abs(got - s[1]) <= 5e-4 * s[1] + 1e-5, (k, got, s[1])
    if with_regressor:
        rsd = tr.regressor.state_dict()
        assert_close(rsd["linears.1.weight"], arr["final.reg.linears.1.weight"], rtol=2e-3, atol=2e-5, name="regressor")
        for k, s in meta["reg_checksums"].items():
            got = float(rsd[k].double().abs().sum())
            assert abs(got - s[1]) <= 5e-4 * s[1] + 1e-5, (k, got, s[1])


def test_train_fn_follows_the_reference_trajectory():
    _drive_trajectory("g5_trajectory", with_regressor=False)


def test_train_fn_with_regressor_side_loop_follows_the_reference_trajectory():
    _drive_trajectory("g5_regressor_trajectory", with_regressor=True)


def test_train_fn_at_the_benchmark_size():
    """BASELINE config 2 at its real size (256^2, per-GPU batch 16, nf 32..128, dropout 0.05): properties that need no
    oracle -- finite and decreasing loss, run-to-run bit-identity, and stream overlap changing nothing but the schedule."""
    import copy
    from behavior_driven_video_synthesis_amd import ops
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import (DEFAULT_CONFIG, ShapePoseNet,
                                                                                     synthetic_batch)
    batch = synthetic_batch(16, 256, "cuda:0")

    def run(two_streams, steps):
        ops.set_dropout_seed(4242)
        torch.manual_seed(7)
        cfg = copy.deepcopy(DEFAULT_CONFIG)
        cfg["training"].update(train_regressor=False, two_streams=two_streams, n_init_batches=1)   # lr 5e-4: the shipped value
        tr = ShapePoseNet(cfg, device="cuda:0", total_steps=1000, vgg_synthetic=True)
        torch.manual_seed(7)   # the eps draws of the steps
        outs = [tr.train_fn(batch) for _ in range(steps)]
        torch.cuda.synchronize()
        sums = [float(b.flat.double().abs().sum()) for b in tr.optimizer.buckets]
        return [float(o["loss"]) for o in outs], [float(o["likelihood_loss"]) for o in outs], sums

    la, lla, sa = run(True, 6)
    assert all(v == v and abs(v) < 1e6 for v in la), la
    assert lla[-1] < lla[0], lla
    lb, _, sb = run(True, 6)
    assert la == lb and sa == sb, (la, lb)             # bit-identical from run to run
    lc, _, sc = run(False, 6)
    assert la == lc and sa == sc, (la, lc)             # one HIP stream == four HIP streams


def _benchmark_cfg(**training):
    """BASELINE config 2 as bench.py times it: 256^2, nf 32..128, dropout 0.05, no regressor side loop, four HIP streams."""
    import copy
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import DEFAULT_CONFIG
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["training"].update(train_regressor=False, two_streams=True, n_init_batches=1)
    cfg["training"].update(training)
    return cfg


def test_hip_graph_replay_is_bit_identical_to_eager_at_the_benchmark_size():
    """the execution mode the driver times -- ONE multi-stream hipGraph replayed at 256^2, per-GPU batch
    16, nf 32..128, dropout 0.05 -- against the same device-resident schedule launched eagerly.  This step differs from the
    tiny one of ``test_hip_graph_replay_is_bit_identical_to_eager`` exactly where a capture can go wrong: 512-way split-K slabs
    in the recycled 192 MB arena, the batched short weight-gradient launches deferred to the weight-norm flush, the
    target-pass fork, the companion streams.  A fresh batch per step, 8 steps (4 of them replays): losses, gamma, the four
    flat parameter buckets, their gradients and both Adam moments must be bit-identical."""
    from behavior_driven_video_synthesis_amd import ops
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import ShapePoseNet, synthetic_batch

    def run(capture, steps=8):
        ops.set_dropout_seed(777)
        tr = ShapePoseNet(_benchmark_cfg(gamma_step=1e-4, information_max=50.0), device="cuda:0", total_steps=1000,
                          vgg_synthetic=True, hip_graph=False)
        tr.enable_hip_graph(capture=capture)
        assert tr.vunet._side_stream is not None and ops._wgrad_streams["on"]       # the four-stream step
        outs = []
        for i in range(steps):
            o = tr.train_fn(synthetic_batch(16, 256, "cuda:0", seed=500 + i))
            outs.append({k: float(o[k]) for k in ("loss", "likelihood_loss", "kl_loss", "gamma", "learning_rate")})
        torch.cuda.synchronize()
        ops.set_dropout_step(None)
        state = [(b.flat.clone(), b.grad.clone(), b.exp_avg.clone(), b.exp_avg_sq.clone()) for b in tr.optimizer.buckets]
        n_graphs = len(tr._graphs)
        del tr
        torch.cuda.empty_cache()
        return outs, state, n_graphs

    oa, sa, na = run(True)
    assert na == 1
    ob, sb, nb = run(False)
    assert nb == 0
    assert oa == ob, (oa, ob)
    assert len({o["loss"] for o in oa}) == len(oa) and all(o["loss"] == o["loss"] for o in oa)   # real, different, finite steps
    assert oa[-1]["gamma"] != oa[1]["gamma"]                                     # the controller moved under replay
    for (pa, ga, ma, va), (pb, gb, mb, vb), name in zip(sa, sb, ("eu", "ed", "du", "dd")):
        assert torch.equal(pa, pb), name + ": parameters"
        assert torch.equal(ga, gb), name + ": gradients of the last step"
        assert torch.equal(ma, mb) and torch.equal(va, vb), name + ": Adam moments"


def test_benchmark_size_step_vs_oracle():
    """ONE step of BASELINE config 2 at its real size -- 256^2, batch 16, nf 32..128, dropout 0.05, four
    HIP streams, through ``ShapePoseNet.train_fn`` -- against the CPU oracle on the same weights, batch, posterior noise and
    dropout keep-masks (the masks are a stateless hash of (element, seed): the seeds every residual block drew are recorded
    and the masks handed to the oracle, as test_rnb_dropout_matches_oracle_with_same_mask does for one block).  At batch 16
    the split-K factor, the tile-to-image mapping of the small-map kernels (the whole batch is one pixel axis) and the
    batched weight-gradient grouping differ from the batch-2 / batch-4 full-size tests.

    Bars: the six perceptual terms, the KL term and the loss to 1e-4 relative.  The four gradient buckets by relative L2:
    the gradient of an L1 loss on ReLU / max-pool features is discontinuous in the features, so two float32 evaluations of
    d loss / d image can differ by ~3e-3 on adversarial inputs (profiles/r04_vgg_grad_cmp_256.txt: float32 oracle 2.6e-3 and
    this path 3.3e-3 from the float64 oracle on random images) and every generator gradient inherits that; on THIS step no
    feature sits on a kink and the measured distances are eu 3.9e-7, ed 3.1e-7, du 2.2e-5, dd 2.1e-5
    (profiles/r05_bench_size_parity.txt).  The bar is 2e-4 -- ten times the largest measured value (SURVEY 8c proposes 1e-3 on
    weight gradients); a step that lands a feature on a kink would have to be looked at, not waved through."""
    import copy
    from behavior_driven_video_synthesis_amd import ops
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import ShapePoseNet, synthetic_batch
    from behavior_driven_video_synthesis_amd.lib.modules import VunetRNB
    from behavior_driven_video_synthesis_amd.lib.utils import get_member
    from oracle import vunet_oracle as O
    cfg = _benchmark_cfg(n_init_batches=0)            # the KL term is part of the loss from the first step
    ops.set_dropout_seed(2024)
    tr = ShapePoseNet(cfg, device="cuda:0", total_steps=1000, vgg_synthetic=True, hip_graph=False)
    tr.gamma.fill_(0.5)
    gamma0 = 0.5
    batch = synthetic_batch(16, 256, "cuda:0", seed=11)
    g = torch.Generator().manual_seed(5)
    eps = [torch.randn(16, 128, 4, 4, generator=g), torch.randn(16, 128, 8, 8, generator=g)]
    sd0 = {k: v.detach().cpu().clone() for k, v in tr.vunet.state_dict().items()}
    vgg_sd = {k: v.detach().cpu().clone() for k, v in tr.vgg.state_dict().items()}
    # ---- record the dropout seed every residual block draws (one per block whose dropout is on)
    seeds, drawn = {}, []
    real_next = ops.next_dropout_seed

    def logging_next():
        s_ = real_next()
        drawn.append(s_)
        return s_
    hooks = []
    for name, m in tr.vunet.named_modules():
        if isinstance(m, VunetRNB):
            hooks.append(m.register_forward_pre_hook(lambda mod, inp, n=name: seeds.__setitem__(n, -len(drawn) - 1)))
            hooks.append(m.register_forward_hook(
                lambda mod, inp, out, n=name: seeds.__setitem__(n, drawn[-seeds[n] - 1] if len(drawn) > -seeds[n] - 1 else None)))
    ops.next_dropout_seed = logging_next
    try:
        out = tr.train_fn(batch, [e.cuda() for e in eps])
        torch.cuda.synchronize()
    finally:
        ops.next_dropout_seed = real_next
        for h in hooks:
            h.remove()
    p_drop = cfg["training"]["dropout_prob"]
    assert sum(v is not None for v in seeds.values()) == len(drawn) > 40       # every draw belongs to exactly one block
    groups = ("eu", "ed", "du", "dd")
    got = {n: torch.cat([p.grad.detach().reshape(-1).cpu() for p in get_member(tr.vunet, n).parameters()]) for n in groups}
    vals = {k: float(v) for k, v in out.items() if torch.is_tensor(v) and v.numel() == 1}

    def drop(name, xs, as_):
        seed = seeds.get(name)
        if seed is None:
            return None, 0.0
        m = ops.dropout_keep_mask(xs, p_drop, seed, "cuda").cpu()
        if as_ is not None:
            m = torch.cat([m, ops.dropout_keep_mask(as_, p_drop, (seed + ops.SEED2_OFFSET) & 0xFFFFFFFF, "cuda").cpu()], dim=1)
        return m, p_drop
    mcfg = dict(cfg["architecture"])
    mcfg.update(cfg["data"])
    mcfg["dropout_prob"] = p_drop
    sdr = {k: v.clone().requires_grad_(True) for k, v in sd0.items()}
    threads = torch.get_num_threads()
    torch.set_num_threads(min(threads, 64))     # (PyTorch-CPU thrashes on this path with hundreds of threads)
    try:
        img, means, logstds, _ = O.vunet_alter_forward(sdr, mcfg, batch["pose_img"].cpu(), batch["stickman"].cpu(), eps, drop=drop)
        ld = O.vgg_loss(vgg_sd, cfg["training"]["vgg_weights"], batch["pose_img"].cpu(), img)
        kl = O.compute_kl_with_prior(means, logstds)
        ll = cfg["training"]["ll_weight"] * torch.stack(list(ld.values()), dim=0).sum()
        loss = ll + gamma0 * kl
        loss.backward()
    finally:
        torch.set_num_threads(threads)
    want = {k: float(v) for k, v in ld.items()}
    want.update(kl_loss=float(kl), likelihood_loss=float(ll), loss=float(loss))
    for k, w in want.items():
        assert abs(vals[k] - w) <= 1e-4 * abs(w) + 1e-6, (k, vals[k], w)
    for n in groups:
        ref = torch.cat([(sdr[f"{n}.{k}"].grad if sdr[f"{n}.{k}"].grad is not None else torch.zeros_like(sdr[f"{n}.{k}"]))
                         .reshape(-1) for k, _ in get_member(tr.vunet, n).named_parameters()])
        rel = float((got[n].double() - ref.double()).norm() / ref.double().norm())
        print(f"bucket {n}: relative L2 distance to the oracle {rel:.2e}")
        assert rel <= 2e-4, (n, rel)


REG_FAR_SHARE = 1e-5     # measured: max |diff| 0.03 lr, no element more than 0.05 lr apart


def test_benchmark_size_step_with_the_regressor_side_loop_vs_oracle():
    """the configuration bench.py times as ``variants.regressor`` -- 256^2, batch 16, ``train_regressor`` --
    through ``ShapePoseNet.train_fn``: the side loop's five regressor steps (experiments/shape_and_pose_net.py:407-425: frozen
    ``ed(eu(reg_imgs[:, i]))``, L2-norm loss, the regressor's own Adam) against the oracle's ``regressor_side_loop`` on the same
    weights, images, targets and posterior noise: every step's loss is not exposed, the LAST one is (the value the step's loss
    subtracts, clamped and weighted, :424-425), and the regressor's parameters after its five updates.  Dropout is off here:
    the side loop's encoder passes would need their 5 x 28 keep-masks handed to the oracle; the kernels are the same."""
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import ShapePoseNet, synthetic_batch
    from oracle import vunet_oracle as O
    cfg = _benchmark_cfg(n_init_batches=0, train_regressor=True, dropout_prob=0.0)
    tr = ShapePoseNet(cfg, device="cuda:0", total_steps=1000, vgg_synthetic=True, hip_graph=False)
    batch = synthetic_batch(16, 256, "cuda:0", seed=11, with_regressor=True)
    R = batch["reg_imgs"].shape[1]
    assert R == 5
    g = torch.Generator().manual_seed(5)
    lat = [(16, 128, 4, 4), (16, 128, 8, 8)]
    eps = [torch.randn(*s_, generator=g) for s_ in lat]
    reg_eps = [[torch.randn(*s_, generator=g) for s_ in lat] for _ in range(R)]
    sd0 = {k: v.detach().cpu().clone() for k, v in tr.vunet.state_dict().items()}
    rsd = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in tr.regressor.state_dict().items()}
    out = tr.train_fn(batch, [e.cuda() for e in eps], [[e.cuda() for e in es] for es in reg_eps])
    torch.cuda.synchronize()
    mcfg = dict(cfg["architecture"])
    mcfg.update(cfg["data"])
    mcfg["dropout_prob"] = 0.0
    opt_reg = torch.optim.Adam(list(rsd.values()), lr=0.001)
    threads = torch.get_num_threads()
    torch.set_num_threads(min(threads, 64))
    try:
        last, values = O.regressor_side_loop(sd0, mcfg, rsd, opt_reg, batch["reg_imgs"].cpu(), batch["reg_targets"].cpu(), reg_eps)
    finally:
        torch.set_num_threads(threads)
    got = float(out["loss_reg"])
    print(f"regressor side loop at 256^2 / batch 16: last loss {got:.6f} vs oracle {values[-1]:.6f} (steps: {values})")
    assert abs(got - values[-1]) <= 1e-4 * abs(values[-1]), (got, values)
    # Adam moves every element by about lr per step whatever its gradient's size: an element whose gradient is summation noise
    # may go the other way on either side (2 lr apart per step) -- bounded in size, and counted
    lr, far, total, worst = 0.001, 0, 0, 0.0
    for k, v in tr.regressor.state_dict().items():
        d = (v.detach().cpu().double() - rsd[k].detach().double()).abs()
        worst = max(worst, float(d.max()))
        far += int((d > 0.05 * lr).sum())
        total += d.numel()
    print(f"regressor parameters after 5 Adam steps: max |diff| {worst / lr:.2f} lr, {far} of {total} elements more than 0.05 lr apart")
    assert worst <= 0.3 * lr and far <= REG_FAR_SHARE * total
    assert float(out["loss"]) == float(out["loss"])      # (the loss's composition is the trajectory tests' subject)


def test_shape_pose_net_l2_conv_variant_initialises_and_trains():
    """conv_layer_type l2 through the training loop: the data-dependent init of L2NormConv2d (lib/modules.py:95-99) runs
    while iteration <= n_init_batches (experiments/shape_and_pose_net.py:199-206), writes THROUGH the flat-bucket views
    (ADVICE r1), and the fused Adam then trains the initialised gamma / beta."""
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import (DEFAULT_CONFIG, ShapePoseNet,
                                                                                     synthetic_batch)
    from behavior_driven_video_synthesis_amd.lib.modules import L2NormConv2d
    cfg = _tiny(DEFAULT_CONFIG, lr=2e-3, n_init_batches=2, train_regressor=False, dropout_prob=0.0)
    cfg["architecture"]["conv_layer_type"] = "l2"
    tr = ShapePoseNet(cfg, device="cuda:0", vgg_width_div=8, total_steps=50, vgg_synthetic=True)
    l2 = [m for m in tr.vunet.modules() if isinstance(m, L2NormConv2d)]
    assert len(l2) > 10
    batch = synthetic_batch(4, 32, "cuda:0")
    g_before = [m.gamma.detach().clone() for m in l2]
    out1 = tr.train_fn(batch)
    flat_lo = min(b.flat.data_ptr() for b in tr.optimizer.buckets)
    flat_hi = max(b.flat.data_ptr() + 4 * b.numel for b in tr.optimizer.buckets)
    for m in l2:
        assert flat_lo <= m.gamma.data_ptr() < flat_hi and flat_lo <= m.beta.data_ptr() < flat_hi   # still bucket views
    changed = sum(int(not torch.equal(a, m.gamma.detach())) for a, m in zip(g_before, l2))
    assert changed == len(l2)                       # every reached layer re-initialised gamma from its batch statistics
    tr.train_fn(batch)                              # iteration 2 <= n_init_batches: init again (then Adam)
    g_init = [m.gamma.detach().clone() for m in l2]
    outs = [tr.train_fn(batch) for _ in range(3)]   # iterations 3..5: no more init, Adam moves the parameters
    assert all(torch.isfinite(torch.as_tensor(float(o["loss"]))) for o in [out1] + outs)
    moved = sum(int(not torch.equal(a, m.gamma.detach())) for a, m in zip(g_init, l2))
    assert moved > len(l2) // 2
    assert float(outs[-1]["likelihood_loss"]) < float(out1["likelihood_loss"]) * 1.5


def _graph_run(capture, steps, with_regressor=False, dropout=0.05, seed=4321, gan=False):
    from behavior_driven_video_synthesis_amd import ops
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import (DEFAULT_CONFIG, ShapePoseNet,
                                                                                     synthetic_batch)
    ops.set_dropout_seed(seed)
    cfg = _tiny(DEFAULT_CONFIG, lr=2e-3, n_init_batches=1, gamma_step=1e-3, information_max=5.0,
                train_regressor=with_regressor, dropout_prob=dropout, imax_scaling="ascend")
    if gan:
        cfg["training"]["gan"] = dict(enabled=True, weight=1.0, pd_scales=2, lr=2e-3)
    tr = ShapePoseNet(cfg, device="cuda:0", vgg_width_div=8, total_steps=50, vgg_synthetic=True, hip_graph=False)
    if capture is not None:
        tr.enable_hip_graph(capture=capture)
    torch.manual_seed(99)                       # the posterior draws (torch.randn_like) of both runs
    outs = []
    for i in range(steps):
        batch = synthetic_batch(4, 32, "cuda:0", seed=100 + i)   # a fresh batch every step: the static inputs are refilled
        if with_regressor:
            g = torch.Generator().manual_seed(7 + i)
            batch["reg_imgs"] = (torch.rand(4, 2, 3, 32, 32, generator=g) * 2 - 1).cuda()
            batch["reg_targets"] = torch.rand(4, 2, 17, 2, generator=g).cuda()
        o = tr.train_fn(batch)
        outs.append({k: float(v) for k, v in o.items() if k in ("loss", "kl_loss", "gamma", "learning_rate", "imax",
                                                                 "loss_reg", "gen_loss", "dloss", "dloss_r", "dloss_f")})
    torch.cuda.synchronize()
    ops.set_dropout_step(None)
    return tr, outs


@pytest.mark.parametrize("with_regressor", [False, True])
def test_hip_graph_replay_is_bit_identical_to_eager(with_regressor):
    """the whole step (forward, losses, backward on all HIP streams, Adam, gamma controller, regressor
    side loop) replayed from ONE captured hipGraph.  Same device-resident schedule launched eagerly = the baseline:
    losses, gamma, every parameter and Adam's state must be bit-identical after 7 steps (4 of them replays), with
    dropout on (fresh mask per replay through the device step counter) and a fresh input batch per step."""
    a, oa = _graph_run(True, 7, with_regressor)
    assert len(a._graphs) == 1
    b, ob = _graph_run(False, 7, with_regressor)
    assert not b._graphs
    assert oa == ob, (oa, ob)
    assert len({o["loss"] for o in oa}) == len(oa)          # the replays did real, different steps
    for (k, p), (_, q) in zip(a.vunet.state_dict().items(), b.vunet.state_dict().items()):
        assert torch.equal(p, q), k
    sa, sb = a.state_dict(), b.state_dict()
    assert sa["optimizer"]["param_groups"] == sb["optimizer"]["param_groups"]
    for i, st in sa["optimizer"]["state"].items():
        assert float(st["step"]) == float(sb["optimizer"]["state"][i]["step"]) == 7.0
        assert torch.equal(st["exp_avg"], sb["optimizer"]["state"][i]["exp_avg"])
    if with_regressor:
        for (k, p), (_, q) in zip(a.regressor.state_dict().items(), b.regressor.state_dict().items()):
            assert torch.equal(p, q), k
        assert float(sa["regressor"]["optimizer"]["state"][0]["step"]) == 14.0


def test_the_training_step_is_recorded_with_the_collector_off(monkeypatch):
    """The trainer records its step under ``ops._graph_recording``: no collector run while the stream captures (a finaliser
    that frees device memory there aborts the process); the eager steps before and the time after run with the collector on."""
    import gc
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import ShapePoseNet
    seen, step = [], ShapePoseNet._step

    def probe(self, *args):
        seen.append((torch.cuda.is_current_stream_capturing(), gc.isenabled()))
        return step(self, *args)
    monkeypatch.setattr(ShapePoseNet, "_step", probe)
    assert gc.isenabled()
    tr, _ = _graph_run(True, 5)
    assert len(tr._graphs) == 1
    assert seen == [(False, True)] * 3 + [(True, False)]     # (three eager steps, the recording; the fifth step is a replay)
    assert gc.isenabled()


def test_hip_graph_replay_with_the_adversarial_term():
    """the step WITH the adversarial term -- generator loss through the PartDiscriminator on a random window
    whose corner is read from device memory (ops.CropWindow), one discriminator step with its own fused Adam -- replayed
    from the captured multi-stream graph against the same schedule launched eagerly: bit-identical losses, generator and
    discriminator parameters after 7 steps (4 replays, a fresh window and batch per step)."""
    a, oa = _graph_run(True, 7, gan=True)
    assert len(a._graphs) == 1
    b, ob = _graph_run(False, 7, gan=True)
    assert oa == ob, (oa, ob)
    assert all("dloss" in o and "gen_loss" in o for o in oa) and len({o["dloss"] for o in oa}) == len(oa)
    for (k, p), (_, q) in zip(a.vunet.state_dict().items(), b.vunet.state_dict().items()):
        assert torch.equal(p, q), k
    for (k, p), (_, q) in zip(a.gan.disc.state_dict().items(), b.gan.disc.state_dict().items()):
        assert torch.equal(p, q), k
    assert float(a.state_dict()["discriminator"]["opt"]["state"][0]["step"]) == 7.0


def test_device_schedule_matches_the_host_schedule():
    """The device-resident lr / step count / information_max path against the plain eager trainer (host scalars as
    launch arguments), dropout off so that both draw nothing: same trajectory to fp32 rounding of Adam's bias
    correction (device pow vs host pow)."""
    a, oa = _graph_run(True, 6, dropout=0.0)
    b, ob = _graph_run(None, 6, dropout=0.0)
    for x, y in zip(oa, ob):
        assert x["learning_rate"] == y["learning_rate"] and x["imax"] == y["imax"]
        assert abs(x["loss"] - y["loss"]) <= 1e-5 * abs(y["loss"]), (x, y)
        assert abs(x["gamma"] - y["gamma"]) <= 1e-5 * abs(y["gamma"]) + 1e-9
    for (k, p), (_, q) in zip(a.vunet.state_dict().items(), b.vunet.state_dict().items()):
        torch.testing.assert_close(p, q, rtol=1e-4, atol=1e-6, msg=k)


def test_split_schemes_match_fp32_on_a_full_size_step():
    """One training step of the benchmark configuration (VunetAlter 256x256, full widths, batch 4, VGG19 perceptual + KL
    loss, dropout on) under the three convolution schemes from identical weights, batch, noise and dropout masks: the
    loss and every gradient bucket of the fp16 (h2) and bf16 (x6) split schemes must agree with the fp32-MFMA run to
    fp32 accuracy -- the whole-model statement of tests/test_hip_x6.py."""
    import copy
    from behavior_driven_video_synthesis_amd import ops
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import (DEFAULT_CONFIG, ShapePoseNet,
                                                                                     synthetic_batch)
    batch = synthetic_batch(4, 256, "cuda:0", seed=7)
    res = {}
    before = ops.conv_precision()
    try:
        for mode in ("f32", "h2", "x6"):
            ops.set_conv_precision(mode)
            ops.set_dropout_seed(99)
            cfg = copy.deepcopy(DEFAULT_CONFIG)
            cfg["training"]["n_init_batches"] = 0            # the KL term is part of the loss from the first step
            tr = ShapePoseNet(cfg, device="cuda:0", total_steps=1000, vgg_synthetic=True)
            tr.gamma.fill_(0.5)
            torch.manual_seed(1234)                          # the posterior draws
            # gradients without the optimiser step: run the step's own pieces
            tr.vunet.train()
            tr.optimizer.zero_grad()
            with ops.prepacked(tr.vunet):
                out_img, means, logstds, _ = tr.vunet(batch["pose_img"], batch["stickman"], None)
                from behavior_driven_video_synthesis_amd.lib.losses import compute_kl_with_prior, vgg_loss
                ld = vgg_loss(tr.custom_vgg, batch["pose_img"], out_img)
                loss = sum(ld.values()).sum() + tr.gamma * compute_kl_with_prior(means, logstds)
                loss.backward()
                tr.vunet.join_streams()
                ops.join_wgrad_streams()
            torch.cuda.synchronize()
            res[mode] = (float(loss.detach()), [b.grad.clone() for b in tr.optimizer.buckets], out_img.detach().clone())
            del tr
    finally:
        ops.set_conv_precision(before)
    l32, g32, y32 = res["f32"]
    for mode in ("h2", "x6"):
        l, g, y = res[mode]
        assert abs(l - l32) <= 2e-5 * abs(l32), (mode, l, l32)
        assert float((y - y32).abs().max()) <= 2e-5 * float(y32.abs().max()), mode
        for a, b in zip(g, g32):
            rel = float((a - b).norm() / b.norm())
            assert rel <= 2e-4, (mode, rel)       # fp32 backward through ~100 layers: the fp32 run itself is this far from fp64
            print(f"{mode}: loss rel {abs(l - l32) / abs(l32):.2e}, image max {float((y - y32).abs().max() / y32.abs().max()):.2e}, "
                  f"bucket grad rel {rel:.2e}")


def test_reference_shaped_loop_through_dropin_follows_the_trajectory(tmp_path):
    """VERDICT r2 #8b: what the reference's OWN loop does with these modules -- imported under the reference's names through
    ``dropin.install()``, a plain ``torch.optim.Adam`` over ``get_member`` param groups (autograd accumulates the
    gradients: no flat buckets, no prepacked weights), ``vgg_loss`` dict, ``compute_kl_with_prior``, the host-side gamma /
    lr rules of experiments/shape_and_pose_net.py:82-85,500-512, ``torch.randn_like`` for the posterior noise -- for the 3
    steps of g5_trajectory.npz, which the reference's modules produced under the same loop on the CPU."""
    import sys
    import numpy as np
    from conftest import load_golden
    from hip_parity_utils import assert_close
    from synth import seeded_randn, synth_image, synth_state_dict
    from behavior_driven_video_synthesis_amd import dropin
    co = tmp_path / "checkout"
    (co / "lib").mkdir(parents=True)
    (co / "models").mkdir()
    (co / "lib" / "utils.py").write_text(
        "from torch.nn import DataParallel\n"
        "def get_member(model, name):\n"
        "    return getattr(model.module, name) if isinstance(model, DataParallel) else getattr(model, name)\n")
    for f in ("lib/modules.py", "lib/losses.py", "models/vunets.py", "models/imagenet_pretrained.py"):
        (co / f).write_text("# the checkout's own file: every name the loop below uses comes from the MI355X package\n")
    before_path, before_mods = list(sys.path), set(sys.modules)
    orig_randn_like = torch.randn_like
    try:
        dropin.install(str(co))
        from models.vunets import VunetAlter                      # the reference's import lines, verbatim
        from models.imagenet_pretrained import PerceptualVGG, vgg19
        from lib.losses import vgg_loss, compute_kl_with_prior
        from lib.utils import get_member
        meta, arr = load_golden("g5_trajectory")
        seed = meta["seed"]
        net = VunetAlter(n_channels_x=3, **meta["cfg"])
        net.load_state_dict(synth_state_dict(meta["shapes"], seed))
        net = net.to("cuda:0")
        vgg = vgg19(pretrained=True, width_div=meta["vgg_width_div"], seed=meta["vgg_seed"], synthetic=True).to("cuda:0")
        vgg.eval()
        custom_vgg = PerceptualVGG(vgg, [1.0] * 6).to("cuda:0")
        opt = torch.optim.Adam([{"params": get_member(net, n).parameters(), "name": n} for n in ("eu", "ed", "du", "dd")],
                               lr=meta["lr0"], betas=tuple(meta["betas"]))
        gamma, lr = meta["gamma0"], meta["lr0"]
        net.train()
        for rec in meta["steps"]:
            it = rec["it"]
            x = synth_image(f"traj.x{it}", (2, 3, 32, 32), seed).cuda()
            c = synth_image(f"traj.c{it}", (2, 3, 32, 32), seed).cuda()
            draws = {"i": 0}

            def fake_randn_like(t, **kw):
                e = seeded_randn(f"traj.{it}.eps{draws['i']}", tuple(t.shape), seed).to(t.device)
                draws["i"] += 1
                return e
            torch.randn_like = fake_randn_like
            img, means, logstds, _ = net(x, c)
            torch.randn_like = orig_randn_like
            assert draws["i"] == 2
            ld = vgg_loss(custom_vgg, x, img)
            ll = 1.0 * torch.sum(torch.stack([ld[k] for k in ld], dim=0))
            kl = compute_kl_with_prior(means, logstds)
            loss = ll
            if it > meta["n_init_batches"]:
                loss = loss + torch.tensor(gamma, device=kl.device) * kl
            opt.zero_grad()
            loss.backward()
            opt.step()
            gamma = max(gamma - meta["gamma_step"] * (meta["imax"] - float(kl)), 0)
            for key, got, want in (("loss", float(loss), rec["loss"]), ("ll", float(ll), rec["ll"]),
                                   ("kl", float(kl), rec["kl"]), ("gamma", gamma, rec["gamma_after"])):
                assert abs(got - want) <= 5e-4 * abs(want) + 1e-5, (it, key, got, want)
            assert abs(lr - rec["lr"]) < 1e-12
            lr = float(np.clip(float(0 - meta["lr0"]) / (meta["total_steps"] - 0) * (it - 0) + meta["lr0"], 0, meta["lr0"]))
            for pg in opt.param_groups:
                pg["lr"] = lr
        sd = net.state_dict()
        assert_close(sd["dd.out_conv.conv.weight_v"], arr["final.dd.out_conv.conv.weight_v"], rtol=2e-3, atol=2e-5,
                     name="final weight")
        for k, s in meta["param_checksums"].items():
            got = float(sd[k].double().abs().sum())
            assert abs(got - s[1]) <= 5e-4 * s[1] + 1e-5, (k, got, s[1])
        # the regressor side loop's call shape (:413): encoder on encoder, four return values
        with torch.no_grad():
            hs, mu, ls, zs = net.ed(net.eu(x))
        assert len(mu) == len(ls) == len(zs) == 2 and mu[0].shape == (2, 16, 4, 4)
    finally:
        torch.randn_like = orig_randn_like
        sys.path[:] = before_path
        for name in set(sys.modules) - before_mods:
            if name.split(".")[0] in ("lib", "models") or name.startswith("_vunet_ref_"):
                del sys.modules[name]


def test_two_graph_mode_trainers_keep_their_own_dropout_counters():
    """the dropout step counter is ONE process-wide pointer inside the library.  A second graph-mode
    trainer -- or ``ops.set_dropout_step(None)`` -- used to replace / clear the first trainer's, after which its steps drew
    the same mask every step (or another trainer's sequence) without any error.  Every step now re-asserts the trainer's
    own counter: a trainer interleaved with another one, with the pointer cleared in between, must follow exactly the
    trajectory it follows alone."""
    import copy
    from behavior_driven_video_synthesis_amd import ops
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import (DEFAULT_CONFIG, ShapePoseNet,
                                                                                     synthetic_batch)
    def make():
        cfg = _tiny(DEFAULT_CONFIG, lr=2e-3, n_init_batches=1, gamma_step=1e-3, information_max=5.0,
                    train_regressor=False, dropout_prob=0.3)
        tr = ShapePoseNet(cfg, device="cuda:0", vgg_width_div=8, total_steps=50, vgg_synthetic=True, hip_graph=False)
        tr.enable_hip_graph(capture=False)     # device-resident schedule, eager launches
        return tr
    batches = [synthetic_batch(4, 32, "cuda:0", seed=300 + i) for i in range(5)]
    eps = [[torch.randn(4, 16, 4, 4, generator=torch.Generator().manual_seed(i)).cuda(),
            torch.randn(4, 16, 8, 8, generator=torch.Generator().manual_seed(50 + i)).cuda()] for i in range(5)]

    ops.set_dropout_seed(77)
    torch.manual_seed(5)
    alone = make()
    ref = [float(alone.train_fn(b, e)["loss"]) for b, e in zip(batches, eps)]
    assert len(set(ref)) == len(ref)
    ops.set_dropout_step(None)

    ops.set_dropout_seed(77)
    torch.manual_seed(5)
    a = make()
    torch.manual_seed(6)
    other = make()                              # takes over the library's pointer at construction
    got = []
    for i, (b, e) in enumerate(zip(batches, eps)):
        got.append(float(a.train_fn(b, e)["loss"]))
        other.train_fn(batches[-1 - i], eps[-1 - i])   # the other trainer steps in between ...
        if i % 2:
            ops.set_dropout_step(None)          # ... and somebody clears the pointer
    torch.cuda.synchronize()
    ops.set_dropout_step(None)
    assert got == ref, (got, ref)


def test_gradient_pass_through_changes_nothing_but_the_launch_count():
    """ops.ConvCfg.passthrough / ops.L1MeanThrough: the gradients of a tensor read by a loss term (VGG taps) or a skip
    connection (the pose pyramid) AND by the next layer meet inside a kernel epilogue instead of in an autograd add.
    Same operands, same additions: the trained weights are bit-identical, and the ATen adds are gone."""
    from torch.profiler import ProfilerActivity, profile
    from behavior_driven_video_synthesis_amd import ops
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import (DEFAULT_CONFIG, ShapePoseNet,
                                                                                     synthetic_batch)
    cfg = _tiny(DEFAULT_CONFIG, lr=1e-3)
    cfg["data"]["spatial_size"] = 64          # wide enough for the fp16 kernels (and their published maxima) to run
    cfg["architecture"].update(nf_start=16, nf_max=32)
    batch = synthetic_batch(2, 64, "cuda:0")

    def run(on):
        ops.enable_grad_passthrough(on)
        try:
            torch.manual_seed(3)
            tr = ShapePoseNet(cfg, device="cuda:0", vgg_width_div=4, total_steps=10, vgg_synthetic=True)
            ops.set_dropout_seed(5)
            eps = [torch.randn(2, 32, 4, 4, device="cuda", generator=torch.Generator("cuda").manual_seed(1)),
                   torch.randn(2, 32, 8, 8, device="cuda", generator=torch.Generator("cuda").manual_seed(2))]
            tr.train_fn(batch, eps)
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                out = tr.train_fn(batch, eps)
                torch.cuda.synchronize()
            adds = sum(e.count for e in prof.key_averages() if e.key in ("aten::add_", "aten::add") and e.device_time_total > 0)
            return out, {k: v.clone() for k, v in tr.vunet.state_dict().items()}, adds
        finally:
            ops.enable_grad_passthrough(True)
    out_on, sd_on, adds_on = run(True)
    out_off, sd_off, adds_off = run(False)
    assert float(out_on["loss"]) == float(out_off["loss"])
    for k in sd_on:
        assert torch.equal(sd_on[k], sd_off[k]), k
    # 5 VGG taps (the last has one reader) + one skip per pyramid level that is followed by a down-sampling layer
    assert adds_off - adds_on >= 4 + 3, (adds_on, adds_off)


@pytest.mark.parametrize("bsz", [4, 16])
def test_full_size_step_with_the_adversarial_term_vs_oracle(bsz):
    """BASELINE config 2's "+GAN" at full size -- VunetAlter 256x256 (nf 32 .. 128), full-width
    VGG19, batch 4 and batch 16 (the configuration bench.py times as ``variants.gan``), ``training.gan.enabled``: one training step.  Finite, bit-reproducible from the seed (two trainers: identical
    scalars and parameters), and the adversarial scalars against the oracle's restatement of DiscTrainer
    (models/synth_discriminator.py:139-191: BCE-with-logits of the PartDiscriminator on the step's real / generated
    window) evaluated on the CPU with the discriminator's pre-step weights -- 1e-4."""
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import (DEFAULT_CONFIG, ShapePoseNet,
                                                                                     synthetic_batch)
    from oracle import vunet_oracle as O
    batch = synthetic_batch(bsz, 256, "cuda:0", seed=11)
    g = torch.Generator().manual_seed(5)
    eps = [torch.randn(bsz, 128, w, w, generator=g).cuda() for w in (4, 8)]

    def run():
        cfg = copy.deepcopy(DEFAULT_CONFIG)
        cfg["training"].update(train_regressor=False, dropout_prob=0.0, batch_size=bsz,
                               gan=dict(enabled=True, weight=1.0, pd_scales=3, lr=2e-4))
        tr = ShapePoseNet(cfg, device="cuda:0", total_steps=1000, vgg_synthetic=True)
        dsd = {k: v.detach().clone().cpu() for k, v in tr.gan.disc.state_dict().items()}
        with torch.no_grad():
            img, _, _, _ = tr.vunet.train()(batch["pose_img"], batch["stickman"], eps)   # the step's generated batch
        out = tr.train_fn(batch, eps=eps)
        torch.cuda.synchronize()
        return tr, dsd, img, {k: float(v) for k, v in out.items() if torch.is_tensor(v) or isinstance(v, float)}

    tr, dsd, img, out = run()
    assert all(v == v and abs(v) < float("inf") for v in out.values()), out
    for k in ("loss", "gen_loss", "dloss", "dloss_r", "dloss_f", "likelihood_loss"):
        assert k in out
    oy, ox = (int(v) for v in tr._gan_off.cpu())
    P = tr.gan_patch
    assert P == 66 and 0 <= oy <= 256 - P and 0 <= ox <= 256 - P
    fake = img[:, :, oy:oy + P, ox:ox + P].cpu()
    real = batch["pose_img"][:, :, oy:oy + P, ox:ox + P].cpu()
    with torch.no_grad():
        lf = O.part_discriminator(dsd, fake, 3)
        lr_ = O.part_discriminator(dsd, real, 3)
    want = {"gen_loss": float(O.bce_with_logits(lf, 1.0)), "dloss_r": float(O.bce_with_logits(lr_, 1.0)),
            "dloss_f": float(O.bce_with_logits(lf, 0.0))}
    want["dloss"] = want["dloss_r"] + want["dloss_f"]
    for k, v in want.items():
        assert abs(out[k] - v) <= 1e-4 * max(1.0, abs(v)), (k, out[k], v)
    # the discriminator and the generator both moved, and toggle_grad was restored
    assert any(not torch.equal(v.cpu(), dsd[k]) for k, v in tr.gan.disc.state_dict().items())
    assert all(p.requires_grad for p in tr.vunet.parameters())
    # bit-reproducible from the seed
    tr2, _, img2, out2 = run()
    assert out == out2 and torch.equal(img, img2)
    for (k, p), (_, q) in zip(tr.vunet.state_dict().items(), tr2.vunet.state_dict().items()):
        assert torch.equal(p, q), k
    for (k, p), (_, q) in zip(tr.gan.disc.state_dict().items(), tr2.gan.disc.state_dict().items()):
        assert torch.equal(p, q), k


def test_vunet_org_train_fn_follows_the_reference_trajectory():
    """VERDICT r3 missing #4: ``experiments.vunet.Vunet.train_fn`` ITSELF -- VunetOrg forward with posterior and
    autoregressive-prior draws, ll_weight * perceptual + kl_weight * compute_kl_loss, fused Adam, lr decay and the linear KL
    warm-up between T/2 and 3T/4 (experiments/vunet.py:248-338,362-371) -- against the seven-step trajectory recorded from
    the reference's modules driven by hand with torch.optim.Adam (tests/golden/make_golden.py g5_org_trajectory; the
    warm-up ramp, kl_weight 1e-6 -> 0.5 -> 1.0, lies inside it).  Tolerance as for g5_trajectory: 5e-4 after Adam steps."""
    from conftest import load_golden
    from hip_parity_utils import assert_close
    from synth import seeded_randn, synth_image, synth_state_dict
    from behavior_driven_video_synthesis_amd.experiments.vunet import DEFAULT_CONFIG, Vunet
    meta, arr = load_golden("g5_org_trajectory")
    seed, n_lat, shapes = meta["seed"], meta["cfg"]["n_latent_scales"], meta["eps_shapes"]
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["data"]["spatial_size"] = meta["cfg"]["spatial_size"]
    cfg["architecture"].update(nf_start=meta["cfg"]["nf_start"], nf_max=meta["cfg"]["nf_max"])
    cfg["training"].update(dropout_prob=0.0, lr=meta["lr0"], adam_betas=tuple(meta["betas"]), kl_init=meta["kl_init"],
                           kl_max=meta["kl_max"], ll_weight=meta["ll_weight"])
    tr = Vunet(cfg, device="cuda:0", n_channels_x=3, vgg_width_div=meta["vgg_width_div"], vgg_seed=meta["vgg_seed"],
               vgg_synthetic=True, total_steps=meta["total_steps"])
    tr.vunet.load_state_dict(synth_state_dict(meta["shapes"], seed))
    for rec in meta["steps"]:
        it = rec["it"]
        batch = {"pose_img": synth_image(f"otraj.x{it}", (2, 3, 32, 32), seed).cuda(),
                 "stickman": synth_image(f"otraj.c{it}", (2, 3, 32, 32), seed).cuda()}
        eps = [seeded_randn(f"otraj.{it}.eps{i}", tuple(shapes[i]), seed).cuda() for i in range(n_lat)]
        prior = [[seeded_randn(f"otraj.{it}.eps{n_lat + 4 * i + l}", tuple(shapes[n_lat + 4 * i + l]), seed).cuda()
                  for l in range(4)] for i in range(n_lat)]
        assert abs(tr.lr - rec["lr"]) < 1e-12 and abs(tr.kl_weight - rec["kl_weight"]) < 1e-12   # what THIS step runs with
        out = tr.train_fn(batch, eps, prior)
        for key, want in (("loss", rec["loss"]), ("likelihood_loss", rec["ll"]), ("kl_loss", rec["kl"])):
            assert abs(float(out[key]) - want) <= 5e-4 * abs(want) + 1e-5, (it, key, float(out[key]), want)
    sd = tr.vunet.state_dict()
    assert_close(sd["dd.out_conv.conv.weight_v"], arr["final.dd.out_conv.conv.weight_v"], rtol=2e-3, atol=2e-5,
                 name="final weight")
    for k, s in meta["param_checksums"].items():
        got = float(sd[k].double().abs().sum())
        assert abs(got - s[1]) <= 5e-4 * s[1] + 1e-5, (k, got, s[1])
