"""The real-vs-fake classifier study on the GPU (csrc/seq_cls.hip, seq_cls.py, behavior_eval.classifier_study and
BehaviorNet.evaluate(classifier_study=True)): the kernels against float64 torch modules, the study against the fixture the
reference's own classes wrote (tests/golden/g14_classifier_study.npz), batching and graph replay bit for bit, the collection
and its cap end to end, and a full-size smoke."""
import copy

import numpy as np
import pytest
import torch

import classifier_study_ref as R
from conftest import load_golden
from synth import seeded_randn

pytestmark = pytest.mark.gpu


def _E():
    from behavior_driven_video_synthesis_amd import behavior_eval
    return behavior_eval


def _cuda(sets):
    return {k: v.cuda() for k, v in sets.items()}


# ---- 1. the kernels against float64 torch (nn.GRU, autograd, SGD)
@pytest.mark.parametrize("bs,t", [(256, 50), (37, 7)])
def test_gru_forward_gradients_and_sgd_vs_float64(bs, t):
    from behavior_driven_video_synthesis_amd import seq_cls as C
    n, h = 3 * bs, 32
    sets = {k: seeded_randn(f"k.{bs}.{k}", (n, t, 51), 3) for k in ("orig", "prior", "cross", "self")}
    sets["embed"] = seeded_randn(f"k.{bs}.embed", (n, h), 3)
    init = R.inputs("noflow")[1][:1]
    blocks = torch.stack([torch.stack([C.pack_classifier(init[0][k]) for k in ("prior", "cross", "self")])])
    reg = torch.stack([C.pack_regressor(R.inputs("noflow")[1][0]["regressor"], h)])
    eng = C.StudyEngine(_cuda(sets), sets["embed"].cuda(), [t - 1], bs, 3, blocks, reg)
    ref = R.GRUClassifier(init[0]["prior"], torch.float64)
    opt = torch.optim.SGD(ref.parameters(), lr=1e-3, momentum=0.9)
    bce = torch.nn.BCEWithLogitsLoss()
    for it in range(3):
        eng.step(False, graph=False)
        sl = slice(it * bs, (it + 1) * bs)
        x = torch.cat([sets["prior"][sl], sets["orig"][sl]]).double()
        _, hT = ref.GRU(x)
        logit = ref.fc1(hT[0])
        loss = bce(logit[:bs], torch.zeros(bs, 1, dtype=torch.float64)) + bce(logit[bs:], torch.ones(bs, 1, dtype=torch.float64))
        opt.zero_grad()
        loss.backward()
        torch.cuda.synchronize()
        if it == 0:
            got_h = eng.grp_t["h"][0, t * 2 * bs * 256:(t + 1) * 2 * bs * 256].reshape(2 * bs, 256).cpu().double()
            np.testing.assert_allclose(got_h.numpy(), hT[0].detach().numpy(), rtol=0, atol=2e-5)
            got_loss = eng.loss_c[0, 0].item()
            np.testing.assert_allclose(got_loss, loss.item(), rtol=2e-5)
            g = eng.grad[0].sum(0).cpu().double()
            g[C.OFF_FCW:] = eng.grad[0, 0, C.OFF_FCW:].cpu().double()
            wg = {k: p.grad for k, p in ref.named_parameters()}
            got_sd = C.unpack_classifier(g)
            for k, v in wg.items():
                scale = float(v.abs().max())
                np.testing.assert_allclose(got_sd[k].numpy(), v.numpy(), rtol=0, atol=2e-4 * scale + 1e-9, err_msg=k)
        opt.step()
    got = C.unpack_classifier(eng.params[0])
    for k, p in ref.named_parameters():
        np.testing.assert_allclose(got[k].double().numpy(), p.detach().numpy(), rtol=0, atol=2e-6, err_msg=k)


# ---- 2. the study against the fixture
STUDY_TOL = dict(rtol=1e-3, atol=1e-4)   # the fixture's fp32 CPU run is within 2e-4 of float64 (test_classifier_study_golden)


@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_study_matches_the_fixture(tag):
    meta, arr = load_golden("g14_classifier_study")
    c = meta["cases"][tag]
    sets, init = R.inputs(tag)
    out = _E().classifier_study(_cuda(sets), times=c["times"], bs=c["bs"], iterations=c["iterations"], init=init)
    assert out["epochs"] == c["iterations"] // (c["rows"] // c["bs"])
    for si in range(len(c["times"])):
        for k, v in out["curves"][si].items():
            np.testing.assert_allclose(v, arr[f"{tag}.{si}.{k}"], err_msg=f"{si} {k}", **STUDY_TOL)
        assert set(out["final"][si]) == set(c["final"][si])
        for k, v in out["final"][si].items():
            np.testing.assert_allclose(v, c["final"][si][k], err_msg=f"{si} {k}", **STUDY_TOL)
            if k.startswith("Acc"):
                assert 0.0 <= v <= 1.0


# ---- 3. invariants: batching and graph replay, bit for bit
def test_batched_start_times_and_graph_replay_are_bit_identical():
    sets, init = R.inputs("flow")
    c = R.CASES["flow"]
    times, bs, iters = list(c[6]), c[4], c[5]
    E = _E()
    together = E.classifier_study(_cuda(sets), times=times, bs=bs, iterations=iters, init=init)
    eager = E.classifier_study(_cuda(sets), times=times, bs=bs, iterations=iters, init=init, graph=False)
    for si, s in enumerate(times):
        alone = E.classifier_study(_cuda(sets), times=[s], bs=bs, iterations=iters, init=[init[si]])
        assert alone["final"][0] == together["final"][si]
        for k, v in together["curves"][si].items():
            assert np.array_equal(alone["curves"][0][k], v), (s, k)
            assert np.array_equal(eager["curves"][si][k], v), (s, k)
        assert eager["final"][si] == together["final"][si]


def test_the_study_step_is_recorded_with_the_collector_off():
    """``StudyEngine.step`` records its iteration under ``ops._graph_recording``: no collector run while the stream captures
    (a finaliser that frees device memory there aborts the process), and the collector is back on afterwards."""
    import gc
    from behavior_driven_video_synthesis_amd import seq_cls as C
    bs, t, h = 37, 7, 32
    sets = {k: seeded_randn(f"k.{bs}.{k}", (3 * bs, t, 51), 3) for k in ("orig", "prior", "cross", "self")}
    embed = seeded_randn(f"k.{bs}.embed", (3 * bs, h), 3)
    init = R.inputs("noflow")[1][:1]
    blocks = torch.stack([torch.stack([C.pack_classifier(init[0][k]) for k in ("prior", "cross", "self")])])
    reg = torch.stack([C.pack_regressor(init[0]["regressor"], h)])
    eng = C.StudyEngine(_cuda(sets), embed.cuda(), [t - 1], bs, 3, blocks, reg)
    seen, issue = [], eng._iteration

    def probe(final):
        seen.append((torch.cuda.is_current_stream_capturing(), gc.isenabled()))
        issue(final)
    eng._iteration = probe
    assert gc.isenabled()
    eng.step(False)
    eng.step(False)              # (a replay: nothing is issued)
    torch.cuda.synchronize()
    assert seen == [(True, False)]
    assert gc.isenabled()


def test_argument_checks():
    sets, init = R.inputs("noflow")
    E = _E()
    with pytest.raises(ValueError):
        E.classifier_study(_cuda(sets), times=(0, 12), bs=32, iterations=3, init=init[:2])
    small = {k: v[:20] for k, v in sets.items()}
    with pytest.raises(ValueError):
        E.classifier_study(_cuda(small), times=(0,), bs=32, iterations=3, init=init[:1])


# ---- 4. end to end through BehaviorNet.evaluate
def _small_model():
    from behavior_driven_video_synthesis_amd.experiments.behavior_net import BehaviorNet, DEFAULT_CONFIG
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["architecture"].update(dim_hidden_b=64, n_flows=2, flow_mid_channels_factor=2, flow_hidden_depth=1)
    torch.manual_seed(7)
    return BehaviorNet(cfg, n_kps=51, device="cuda:0", hip_graph=True)


def _batches(n_batches, b=6, t=7):
    out = []
    for i in range(n_batches):
        out.append({k: (0.5 * seeded_randn(f"e2e.{i}.{k}", (b, t + 1, 51), 9)).cuda()
                    for k in ("keypoints", "future_keypoints", "paired_keypoints", "matched_keypoints")})
    return out


def _noise(n_batches, b=6, h=64):
    z = [seeded_randn(f"e2e.z{i}", (2, b // 2, h), 9).cuda() for i in range(n_batches)]
    eps = [seeded_randn(f"e2e.eps{i}", (b, h), 9).cuda() for i in range(n_batches)]
    sn = [{"prior": seeded_randn(f"e2e.prior{i}", (b, h), 9).cuda(), "flow": seeded_randn(f"e2e.flow{i}", (b, h), 9).cuda()}
          for i in range(n_batches)]
    return z, eps, sn


def test_evaluate_collects_caps_and_runs_the_study():
    from behavior_driven_video_synthesis_amd.behavior_eval import PoseStats
    bn = _small_model()
    batches = _batches(4)
    z, eps, sn = _noise(4)
    stats = PoseStats(np.zeros(51), np.ones(51), [], device="cuda")
    ev = bn.evaluate(batches, stats, n_samples=2, skip=2, z=z, eps=eps, classifier_study=True, study_noise=sn,
                     study_kwargs=dict(max_rows=10, times=(0, 6), bs=4, iterations=6))
    lists = ev.lists()
    # batches 0 and 1 are collected (6 < 10, then 12 >= 10); batch 2 is still scored, then the loop ends; batch 3 never runs
    assert ev.study_set.rows == 12
    assert lists["ADE"].shape == (3,) and lists["ADE_c"].shape == (2,)
    got = ev.study_set.tensors()
    flow = bn.latent_flow
    with torch.no_grad():
        for i in range(2):
            kps = batches[i]["keypoints"]
            x_s, tg = kps[:, :-1].contiguous(), kps[:, 1:].contiguous()
            x_t = batches[i]["paired_keypoints"][:, :-1].contiguous()
            _, _, _, _, mu, *_ = bn.net(x_s, x_t, 7, sample=False, eps=eps[i])
            sl = slice(6 * i, 6 * (i + 1))
            want = {"orig": x_s, "embed": mu,
                    "prior": bn.net(x_s, tg, 7, sample=True, start_frame=6, eps=sn[i]["prior"])[0],
                    "cross": bn.net.generate_seq(mu, x_t, 7, start_frame=0)[0],
                    "self": bn.net.generate_seq(mu, x_s, 7, start_frame=0)[0],
                    "flow": bn.net.generate_seq(flow.reverse(sn[i]["flow"]).reshape(6, 64), tg, 7, start_frame=6)[0]}
            for k, v in want.items():
                assert torch.equal(got[k][sl], v), (i, k)
    st = ev.study
    assert st["num_samples"] == 12 and st["epochs"] == 2 and len(st["final"]) == 2
    for fin in st["final"]:
        assert set(fin) == {"Acc Prior", "Acc Cross", "Acc Self", "Acc Flow", "Loss_regressor", "DE"}
        assert all(np.isfinite(v) for v in fin.values())
    # without the study: every batch scored, transfer metrics on every batch, the same summary as the plain call
    bn2 = _small_model()
    plain = bn2.evaluate(batches, stats, n_samples=2, skip=2, z=z, eps=eps).summary()
    bn3 = _small_model()
    off = bn3.evaluate(batches, stats, n_samples=2, skip=2, z=z, eps=eps, classifier_study=False).summary()
    assert plain == off
    assert not hasattr(bn3.evaluate(batches, stats, n_samples=2, skip=2, z=z, eps=eps), "study")
    with pytest.raises(ValueError):
        bn.evaluate([{k: v for k, v in batches[0].items() if k != "matched_keypoints"}], stats, n_samples=2, skip=2,
                    classifier_study=True)


# ---- 5. full size
def test_full_size_smoke():
    """25 024 rows, T 50, six start times, with a flow, H 1024: one epoch of 97 iterations and the final pass."""
    g = torch.Generator().manual_seed(3)
    n, t = 25024, 50
    sets = {k: torch.randn(n, t, 51, generator=g).cuda() for k in ("orig", "prior", "cross", "self", "flow")}
    sets["embed"] = torch.randn(n, 1024, generator=g).cuda()
    torch.manual_seed(3)
    out = _E().classifier_study(sets, bs=256, iterations=97)
    assert out["epochs"] == 1 and len(out["final"]) == 6
    for fin, cur in zip(out["final"], out["curves"]):
        assert set(fin) == {"Acc Prior", "Acc Cross", "Acc Self", "Acc Flow", "Loss_regressor", "DE"}
        for k, v in fin.items():
            assert np.isfinite(v), k
            if k.startswith("Acc"):
                assert 0.0 <= v <= 1.0, k
        for k, v in cur.items():
            assert v.shape == (97,) and np.isfinite(v).all(), k
