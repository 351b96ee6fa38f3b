"""The cVAE step with the adversarial pose regressor, ``cvae: True`` and the last-ten-epochs freeze (BASELINE config 4,
experiments/behavior_net.py:606-660) on the MI355X: ``BehaviorNet.train_fn`` against the g12 fixture
(tests/golden/make_golden_regressor.py) and, at the reference size, against the float64 restatement in regressor_ref.py."""
import copy

import numpy as np
import pytest
import torch

from conftest import load_golden
from regressor_ref import KEYS, inner_steps, regressor_init, slice_of
from synth import seeded_randn, synth_behavior_state

pytestmark = pytest.mark.gpu


def _rel(a, b):
    a = a.detach().double().cpu() if isinstance(a, torch.Tensor) else torch.as_tensor(np.asarray(a)).double()
    b = b.detach().double().cpu() if isinstance(b, torch.Tensor) else torch.as_tensor(np.asarray(b)).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _trainer(hid, bsz, graph, w=0.01, cvae=False, lr=1e-3, gamma_init=0.05, gamma_step=1e-3, imax=5.0, recon=2.5, seed=121,
             shapes=None, reg_shapes=None):
    from behavior_driven_video_synthesis_amd.experiments.behavior_net import BehaviorNet, DEFAULT_CONFIG
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["architecture"].update(dim_hidden_b=hid, n_flows=1, flow_mid_channels_factor=1, flow_hidden_depth=1, cvae=cvae)
    cfg["training"].update(batch_size=bsz, lr_init=lr, recon_loss_weight=recon, gamma_init=gamma_init, gamma_step=gamma_step,
                           information_max=imax, use_regressor=True, weight_regressor=w)
    tr = BehaviorNet(cfg, n_kps=51, hip_graph=graph)
    shapes = shapes or {k: list(v.shape) for k, v in tr.net.state_dict().items()}
    tr.net.load_state_dict(synth_behavior_state(shapes, seed, {}))
    reg_shapes = reg_shapes or {k: list(v.shape) for k, v in tr.regressor.state_dict().items()}
    rsd = regressor_init(reg_shapes, seed)
    tr.regressor.load_state_dict(rsd)
    tr.regressor_engine.load_module()
    return tr, rsd


@pytest.mark.parametrize("graph", [False, True])
@pytest.mark.parametrize("tag", ["shipped", "w1", "cvae"])
def test_fused_cvae_regressor_follows_the_reference_trajectory(tag, graph):
    """Three fused steps -- cVAE forward, loss, five regressor steps, the adversarial term (W^5, the fifth forward's masks),
    BPTT, the net's Adam, gamma -- against the reference driven with torch 1.3.1's regressor Adam."""
    meta, arr = load_golden("g12_cvae_regressor")
    case, seed = meta["cases"][tag], meta["seed"]
    bsz, t_len, hid = meta["batch"], meta["seq_len"], meta["kw"]["dim_hidden_b"]
    tr, _ = _trainer(hid, bsz, graph, w=case["w"], cvae=case["cvae"], lr=meta["lr"], gamma_init=meta["gamma_init"],
                     gamma_step=meta["gamma_step"], imax=meta["imax"], recon=meta["recon_loss_weight"], seed=seed,
                     shapes=meta["shapes"], reg_shapes=meta["reg_shapes"])
    for it in range(meta["steps"]):
        kps = meta["kps_scale"][it] * seeded_randn(f"reg.kps{it}", (bsz, t_len + 1, 51), seed)
        eps = seeded_randn(f"reg.s{it}.eps0", (bsz, hid), seed).cuda()
        out = tr.train_fn({"keypoints": kps.cuda()}, eps=eps, reg_index=torch.as_tensor(arr["idx"][it]))
        want = case["logs"][it]
        for k in ("loss", "loss_recon", "kl_loss", "gamma", "mu_s", "logstd_s", "loss_regressor"):
            assert abs(out[k] - want[k]) <= 2e-5 * abs(want[k]) + 2e-6, (it, k, out[k], want[k])
        rp = tr.regressor_engine.plan(bsz)
        got_l = rp["reg"][:5].cpu().tolist()
        assert all(abs(a - b) <= 2e-5 * abs(b) for a, b in zip(got_l, want["L"])), (it, got_l, want["L"])
        assert _rel(rp["adv"], arr[f"{tag}.adv{it}"]) <= 3e-5, it
    sd = tr.state_dict()
    names = [n for n, _ in tr.net.named_parameters()]
    st, rst = sd["optimizer"]["state"], sd["regressor_optimizer"]["state"]
    err = {}
    for k, v in sd["model"].items():
        err[k] = _rel(slice_of(v), arr[f"{tag}.final.{k}"])
        s, a = case["checksums"][k]
        assert abs(float(v.double().abs().sum()) - a) <= 1e-4 * a + 1e-6, k
    for n in ("decoder.rnn.weight_hh", "b_enc.mu_fn.conv.weight_v", "decoder.n_out.bias"):
        err["exp_avg." + n] = _rel(slice_of(st[names.index(n)]["exp_avg"]), arr[f"{tag}.exp_avg.{n}"])
    for i, k in enumerate(KEYS):
        err["reg." + k] = _rel(slice_of(sd["regressor"][k]), arr[f"{tag}.reg.{k}"])
        s, a = case["reg_checksums"][k]
        assert abs(float(sd["regressor"][k].double().abs().sum()) - a) <= 1e-4 * a + 1e-6, k
        assert rst[i]["step"] == case["reg_adam_step"]
        err["reg_exp_avg." + k] = _rel(slice_of(rst[i]["exp_avg"]), arr[f"{tag}.reg_exp_avg.{k}"])
        err["reg_exp_avg_sq." + k] = _rel(slice_of(rst[i]["exp_avg_sq"]), arr[f"{tag}.reg_exp_avg_sq.{k}"])
    print(f"\n[g12 {tag} graph={graph}] " + " ".join(f"{k}={v:.1e}" for k, v in err.items()))
    # the regressor (and everything it feeds: L_1..5, the adversarial d/dmu, the logs) at g11's 3e-5.  The net's own parameters
    # and moments come out of the unchanged back-propagation through time over 50 frames at 256 hidden units (g11: 6 frames, 64),
    # where fp32 summation order alone separates two fp32 runs further: measured <= 8.5e-5 (parameters), <= 6.4e-4 (exp_avg)
    tol = {k: (1e-3 if k.startswith("exp_avg.") else 2e-4) if k in sd["model"] or k.startswith("exp_avg.") else 3e-5 for k in err}
    bad = {k: v for k, v in err.items() if v > tol[k]}
    assert not bad, bad


@pytest.mark.parametrize("graph", [False, True])
def test_update_false_freezes_the_net_and_gamma_but_trains_the_regressor(graph):
    """``update=False`` (the reference's last ten epochs, :656-660): no backward, no net step, no gamma move; the regressor
    still takes its five steps and the logs are produced."""
    tr, _ = _trainer(256, 8, graph)
    kps = 0.6 * seeded_randn("frz.kps", (8, 51, 51), 5)
    tr.train_fn({"keypoints": kps.cuda()}, eps=seeded_randn("frz.eps", (8, 256), 5).cuda())
    net0 = {k: v.clone() for k, v in tr.net.state_dict().items()}
    opt0 = copy.deepcopy(tr.optimizer.state_dict())
    gamma0 = tr.gamma_dev.clone()
    reg0 = {k: v.clone() for k, v in tr.state_dict()["regressor"].items()}
    step0 = tr.regressor_engine.adam.step
    for i in range(3):   # eager, recorded, replayed
        out = tr.train_fn({"keypoints": kps.cuda()}, eps=seeded_randn(f"frz.eps{i}", (8, 256), 5).cuda(), update=False)
        assert np.isfinite(out["loss"]) and np.isfinite(out["loss_regressor"]) and "kl_loss" in out
    for k, v in tr.net.state_dict().items():
        assert torch.equal(v, net0[k]), k
    opt1 = tr.optimizer.state_dict()
    for i, s in opt0["state"].items():
        assert s["step"] == opt1["state"][i]["step"]
        assert torch.equal(s["exp_avg"], opt1["state"][i]["exp_avg"]) and torch.equal(s["exp_avg_sq"], opt1["state"][i]["exp_avg_sq"])
    assert torch.equal(tr.gamma_dev, gamma0)
    assert tr.regressor_engine.adam.step == step0 + 15
    reg1 = tr.state_dict()["regressor"]
    assert all(not torch.equal(reg1[k], reg0[k]) for k in reg0), "every regressor parameter moves"


def _ref_size_inputs(seed=7):
    kps = 0.5 * seeded_randn("rs.kps", (64, 51, 51), seed)
    return kps, seeded_randn("rs.eps", (64, 1024), seed), torch.tensor([3, 17, 49, 0, 25], dtype=torch.int32)


def test_reference_size_step_vs_float64_restatement():
    """B 64, T 50, H 1024 (config/behavior_net.yaml): one step; the regressor's parameters after its five steps and the
    adversarial part of d loss / d mu against the float64 restatement from the same mu and indices."""
    kps, eps, idx = _ref_size_inputs()
    tr, rsd = _trainer(1024, 64, False)
    tr.train_fn({"keypoints": kps.cuda()}, eps=eps.cuda(), reg_index=idx)
    mu = tr.net.train_engine()._tplan(64, 50, 50, 50)["mu"].detach().double().cpu()
    P0 = {k: v.double() for k, v in rsd.items()}
    ls, P, _, adv, adv4 = inner_steps(P0, mu, kps[:, :-1].double(), idx.tolist(), 0.01)
    rp = tr.regressor_engine.plan(64)
    got_l = rp["reg"][:5].cpu().tolist()
    assert all(abs(a - b) <= 2e-5 * abs(b) for a, b in zip(got_l, ls)), (got_l, ls)
    assert ls[4] <= 0.7, ls                          # the adversarial term is live
    sd = tr.state_dict()["regressor"]
    worst = max(_rel(sd[k], P[k]) for k in KEYS)
    assert worst <= 3e-5, f"{worst:.2e}"
    err = _rel(rp["adv"], adv)
    assert err <= 3e-5, f"{err:.2e}"
    assert _rel(adv4, adv) > 10 * err                # the comparison tells W^5 from W^4
    print(f"\n[reference size] regressor parameters {worst:.2e}, adversarial d/dmu {err:.2e} (W^4 would be {_rel(adv4, adv):.1e})")


def test_graph_replay_is_bit_identical_to_eager_at_the_reference_size():
    kps, eps, idx = _ref_size_inputs()
    outs, trs = [], []
    for graph in (False, True):
        tr, _ = _trainer(1024, 64, graph)
        log = [tr.train_fn({"keypoints": kps.cuda()}, eps=(eps + 0.1 * i).cuda(), reg_index=(idx + i) % 50) for i in range(3)]
        outs.append(log)
        trs.append(tr)
    for a, b in zip(*outs):
        for k in ("loss", "loss_regressor", "kl_loss", "gamma"):
            assert a[k] == b[k], (k, a[k], b[k])
    sa, sb = trs[0].state_dict(), trs[1].state_dict()
    for part in ("model", "regressor"):
        for k, v in sa[part].items():
            assert torch.equal(v, sb[part][k]), (part, k)


def test_use_regressor_needs_seq_len_50():
    tr, _ = _trainer(256, 4, False)
    with pytest.raises(ValueError, match="seq_len == 50"):
        tr.train_fn({"keypoints": torch.zeros(4, 7, 51).cuda()})
