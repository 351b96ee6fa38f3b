"""GPU: the post-hoc pose-regressor probe (csrc/reg_probe.hip, reg_probe.RegProbeEngine, ``regressor_probe`` of both image
experiments, ``training.fused_regressor``) against the reference's trajectory (tests/golden/g17_reg_probe.npz) and the plain-torch
oracle (tests/reg_probe_ref.py)."""
import copy
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import reg_probe_ref as R
from conftest import ROOT, load_golden

pytestmark = pytest.mark.gpu

RTOL, ATOL = 2e-4, 2e-5       # the project's standing fp32 tolerance for the seq path
TRAJ_REL, TRAJ_ABS = 1e-4, 1e-6


def _module(cfg, sd=None):
    from behavior_driven_video_synthesis_amd.models.vunets import Regressor
    reg = Regressor(**R.model_kwargs(cfg))
    reg.load_state_dict(R.init_state(cfg) if sd is None else sd)
    return reg.cuda()


def _cuda(batch):
    means, tgt = batch
    return [m.cuda() for m in means], tgt.cuda()


def _traj_dev(got, want):
    """-> (max|got - want|, the worst deviation in units of the trajectory bound 1e-4 |want| + 1e-6)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    diff = np.abs(got - want)
    return float(diff.max()), float((diff / (TRAJ_REL * np.abs(want) + TRAJ_ABS)).max())


def _traj_close(got, want, what, allow=1.0):
    diff, worst = _traj_dev(got, want)
    print(f"{what}: max|diff| = {diff:.3e}, worst deviation = {worst:.3f} of the bound (allowed {allow:.3f})")
    assert worst <= allow, (what, worst, allow)


def _run_engine(tag, steps=R.STEPS):
    cfg = R.CASES[tag]
    reg = _module(cfg)
    eng = reg.probe_engine(n_steps=steps)
    for batch in R.inputs(tag, cfg, steps):
        eng.step(*_cuda(batch))
    eng.write_back()
    return reg, eng


# ---- 1. forward parity
def test_forward_matches_the_reference_and_the_oracle_small():
    meta, arr = load_golden("g17_reg_probe")
    cfg = R.CASES["small"]
    means, _ = R.inputs("small", cfg, 1)[0]
    pred = _module(cfg).probe_engine().forward([m.cuda() for m in means]).cpu()
    np.testing.assert_allclose(pred.numpy(), arr["small.pred1"], rtol=RTOL, atol=ATOL)
    sd64 = {k: v.double() for k, v in R.init_state(cfg).items()}
    ref, _ = R.forward(sd64, cfg, [m.double() for m in means])
    np.testing.assert_allclose(pred.numpy(), ref.numpy(), rtol=RTOL, atol=ATOL)


def test_forward_at_the_shipped_sizes_is_as_close_to_float64_as_the_float32_oracle():
    cfg = R.SHIPPED
    means, _ = R.inputs("shipped", cfg, 1)[0]
    sd = R.init_state(cfg)
    eng = _module(cfg, sd).probe_engine()
    assert all(lay.inplace for lay in eng.emb) and eng.lin[0].inplace     # the state-dict tensors are the kernels' operands
    pred = eng.forward([m.cuda() for m in means]).cpu()
    ref64, _ = R.forward({k: v.double() for k, v in sd.items()}, cfg, [m.double() for m in means])
    ref32, _ = R.forward(sd, cfg, means)
    np.testing.assert_allclose(pred.numpy(), ref64.numpy(), rtol=RTOL, atol=ATOL)
    err_hip, err_cpu = float((pred.double() - ref64).abs().max()), float((ref32.double() - ref64).abs().max())
    print(f"shipped sizes: max|hip - f64| = {err_hip:.3e}, max|cpu f32 - f64| = {err_cpu:.3e}")
    assert err_hip <= 2.0 * err_cpu, (err_hip, err_cpu)


# ---- 2. split-K edge shapes
@pytest.mark.parametrize("B", [1, 5, 16, 17, 64])
def test_split_k_edge_shapes(B):
    from behavior_driven_video_synthesis_amd import _lib
    from behavior_driven_video_synthesis_amd.reg_probe import split_k
    from synth import seeded_randn
    lib = _lib.lib()
    bp = (B + 15) // 16 * 16
    for K in (64, 192, 8192):
        for M in (16, 128):
            S = split_k(M, K)
            assert K % (64 * S) == 0 and (K, S) != (192, 1)
            x = torch.zeros(bp, K)
            x[:B] = seeded_randn(f"x.{B}.{K}", (B, K), 3)
            w = seeded_randn(f"w.{M}.{K}", (M, K), 3) * (1.5 / K) ** 0.5
            bias = 0.1 * seeded_randn(f"b.{M}", (M,), 3)
            ldy, off = M + 8, 4
            y = torch.zeros(bp, ldy)
            y[:, off:off + M] = 7.0                                       # stale values where the kernel must write
            xd, wd, bd, yd = x.cuda(), w.cuda(), bias.cuda(), y.cuda()
            part = torch.full((S * bp * M,), float("nan"), device="cuda")
            p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
            assert lib.vunet_reg_probe_embed(p(xd), p(wd), B, M, K, S, p(part), None) == 0
            assert lib.vunet_reg_probe_embed_finish(p(part), S, p(bd), B, M, p(yd), ldy, off, None) == 0
            got = yd.cpu()
            ref = torch.relu(x[:B].double() @ w.double().t() + bias.double())
            np.testing.assert_allclose(got[:B, off:off + M].numpy(), ref.numpy(), rtol=RTOL, atol=ATOL, err_msg=f"{B} {K} {M}")
            assert float(ref.max()) > 0.1
            assert torch.equal(got[B:], torch.zeros(bp - B, ldy)), (B, K, M)              # rows B .. Bp
            assert torch.equal(got[:, :off], torch.zeros(bp, off)) and torch.equal(got[:, off + M:], torch.zeros(bp, ldy - off - M))
    # arguments outside the contract are refused, not launched
    assert lib.vunet_reg_probe_embed(p(xd), p(wd), B, 16, 192, 2, p(part), None) != 0
    assert lib.vunet_reg_probe_embed(p(xd), p(wd), 65, 16, 64, 1, p(part), None) != 0


# ---- 3. the loss kernel
@pytest.mark.parametrize("B", [1, 5, 64])
def test_loss_kernel_value_gradient_and_padding(B):
    from behavior_driven_video_synthesis_amd import _lib
    from synth import seeded_randn
    lib = _lib.lib()
    n, ldp, bp = 34, 64, (B + 15) // 16 * 16
    pred = torch.zeros(bp, ldp)
    pred[:B, :n] = seeded_randn(f"pred.{B}", (B, n), 4)
    pred[:, n:] = 3.0                                                     # padded columns must not count
    pred[B:] = 5.0                                                        # nor padded rows
    tgt = seeded_randn(f"tgt.{B}", (B, n), 4)
    same = 2 if B > 2 else None
    if same is not None:
        tgt[same] = pred[same, :n]
    pd, td = pred.cuda(), tgt.cuda()
    dpred = torch.full((bp, ldp), float("nan"), device="cuda")
    last, losses, cursor = torch.zeros(1, device="cuda"), torch.zeros(2, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    for _ in range(3):                                                    # the third append is beyond the buffer: dropped
        assert lib.vunet_reg_probe_loss(p(pd), ldp, p(td), n, B, n, p(dpred), p(last), p(losses), 2, p(cursor), None) == 0
    pr = pred[:B, :n].clone().requires_grad_(True)
    ref = torch.norm(pr - tgt, dim=1).mean()
    ref.backward()
    got = dpred.cpu()
    assert torch.isfinite(last).all() and int(cursor.item()) == 3
    np.testing.assert_allclose(float(last), float(ref.detach()), rtol=1e-6)
    assert torch.equal(losses.cpu(), last.cpu().expand(2))
    np.testing.assert_allclose(got[:B, :n].numpy(), pr.grad.numpy(), rtol=1e-5, atol=1e-8)
    assert torch.equal(got[B:], torch.zeros(bp - B, ldp)) and torch.equal(got[:, n:], torch.zeros(bp, ldp - n))
    if same is not None:
        assert torch.equal(got[same], torch.zeros(ldp)) and torch.equal(pr.grad[same], torch.zeros(n))


# ---- 4. trajectory
@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_six_recorded_steps_reproduce_the_reference_trajectory(tag):
    """Step 1 is issued eagerly, step 2 records the hipGraph, steps 3-6 replay it.  Bound: 1e-4 relative with an absolute floor
    of 1e-6 (Adam's first steps divide by sqrt(v) ~ |g|: a tighter bound would test rounding)."""
    meta, arr = load_golden("g17_reg_probe")
    reg, eng = _run_engine(tag)
    assert eng.graph.enabled and len(eng.graph.graphs) == 1
    losses = eng.losses()
    assert losses.shape == (R.STEPS,)
    _traj_close(losses.numpy(), arr[f"{tag}.losses"], f"{tag} losses")
    for k, v in reg.state_dict().items():
        _traj_close(v.cpu().reshape(-1)[:meta["keep"]].numpy(), arr[f"{tag}.param.{k}"], f"{tag} {k}")


# ---- 5. graph replay equals eager
_CHILD = """
import sys
sys.path.insert(0, {tests!r}); sys.path.insert(0, {root!r})
import numpy as np
import test_hip_reg_probe as T
reg, eng = T._run_engine("small")
assert not eng.graph.enabled and not eng.graph.graphs
np.savez({out!r}, losses=eng.losses().numpy(), **{{k: v.cpu().numpy() for k, v in reg.state_dict().items()}})
"""


def test_graph_replay_is_bit_identical_to_eager(tmp_path):
    reg, eng = _run_engine("small")
    out = str(tmp_path / "eager.npz")
    code = _CHILD.format(tests=os.path.join(ROOT, "tests"), root=ROOT, out=out)
    env = dict(os.environ, VUNET_SEQ_GRAPH="0")
    r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, "-c", code], env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(out)
    assert np.array_equal(z["losses"], eng.losses().numpy())
    for k, v in reg.state_dict().items():
        assert np.array_equal(z[k], v.cpu().numpy()), k


# ---- 6. the experiments' regressor_probe, end to end
def _module_route(regressor, means_per_step, targets_per_step, lr=1e-3):
    """The module's existing route: ``Regressor.forward`` + autograd + torch.optim.Adam."""
    opt = torch.optim.Adam(regressor.parameters(), lr=lr)
    losses = []
    for means, tgt in zip(means_per_step, targets_per_step):
        loss = torch.norm(regressor(means) - tgt, dim=1).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    return torch.stack(losses).cpu()


def _probe_batches(spatial, n, n_channels_x=3):
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import synthetic_batch, synthetic_keypoints
    batches = []
    for i in range(n):
        b = synthetic_batch(2, spatial, "cuda:0", seed=100 + i, n_channels_x=n_channels_x)
        b["keypoints"] = synthetic_keypoints(2, spatial, seed=100 + i) / spatial
        batches.append(b)
    return batches


def _check_probe(tr, encode, batches, make_regressor, oracle_cfg=None):
    """``oracle_cfg``: the trajectory bound's second clause -- where 1e-4 is exceeded, measure the CPU float32 oracle's deviation
    from the float64 oracle on the same six steps and allow 4 x that."""
    from synth import seeded_randn
    with torch.no_grad():
        tr.vunet.eval()
        shapes = [tuple(m.shape) for m in encode(batches[0], None)]
    eps = [[seeded_randn(f"probe.eps.{i}.{s}", sh, 9).cuda() for s, sh in enumerate(shapes)] for i in range(len(batches))]
    before = {k: v.clone() for k, v in tr.vunet.state_dict().items()}
    torch.manual_seed(5)
    out = tr.regressor_probe(batches, n_epochs=2, eps=eps)
    for k, v in tr.vunet.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert out["loss"].shape == (6,) and out["loss"].device.type == "cpu" and torch.isfinite(out["loss"]).all()
    assert abs(out["running_mean_100"] - float(out["loss"].mean())) < 1e-6
    torch.manual_seed(5)
    ref = make_regressor()
    with torch.no_grad():
        means = [[m.clone() for m in encode(b, e)] for b, e in zip(batches, eps)] * 2
    tgts = [b["keypoints"].reshape(2, -1).cuda() for b in batches] * 2
    sd0 = {k: v.detach().cpu().clone() for k, v in ref.state_dict().items()}
    ref_losses = _module_route(ref, means, tgts)
    allow = 1.0
    if oracle_cfg is not None:
        cpu = [([m.cpu() for m in ms], t.cpu()) for ms, t in zip(means, tgts)]
        l32, _, sd32, _ = R.run(oracle_cfg, sd0, cpu, torch.float32)
        l64, _, sd64, _ = R.run(oracle_cfg, sd0, cpu, torch.float64)
        own = max([_traj_dev(l32.numpy(), l64.numpy())[1]] + [_traj_dev(sd32[k].numpy(), sd64[k].numpy())[1] for k in sd0])
        eng64 = max(_traj_dev(v.cpu().numpy(), sd64[k].numpy())[1] for k, v in out["regressor"].state_dict().items())
        mod64 = max(_traj_dev(v.detach().cpu().numpy(), sd64[k].numpy())[1] for k, v in ref.state_dict().items())
        print(f"float32 oracle vs float64 oracle: {own:.3f} of the bound; engine vs float64: {eng64:.3f}; module route vs float64: {mod64:.3f}")
        allow = max(1.0, 4.0 * own)
    _traj_close(out["loss"].numpy(), ref_losses.numpy(), "probe losses", allow)
    for (k, v), (_, w) in zip(out["regressor"].state_dict().items(), ref.state_dict().items()):
        _traj_close(v.cpu().numpy(), w.detach().cpu().numpy(), f"probe {k}", allow)


def _small_cfg(default, spatial=64):
    cfg = copy.deepcopy(default)
    cfg["data"]["spatial_size"] = spatial
    cfg["architecture"].update(nf_start=8, nf_max=16)
    cfg["training"].update(dropout_prob=0.0)
    return cfg


def test_shape_pose_net_regressor_probe_end_to_end():
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import DEFAULT_CONFIG, ShapePoseNet
    from behavior_driven_video_synthesis_amd.models.vunets import Regressor
    cfg = _small_cfg(DEFAULT_CONFIG)
    tr = ShapePoseNet(cfg, device="cuda:0", vgg_width_div=8, total_steps=50, vgg_synthetic=True)
    arch = cfg["architecture"]
    widths = [64 // (2 ** (tr.vunet.n_scales - i)) for i in range(arch["n_latent_scales"], 0, -1)]

    def encode(batch, e):
        return tr.vunet.ed(tr.vunet.eu(batch["pose_img"]), e)[1]
    _check_probe(tr, encode, _probe_batches(64, 3), lambda: Regressor(34, latent_widths=widths, **arch).cuda())


def test_vunet_regressor_probe_end_to_end():
    """Against the module route this case exceeds 1e-4 (floor 1e-6): measured 3.12 x the bound, max|diff| 6.4e-6, all of it in
    ``embedders.0.weight``.  Against the float64 oracle on the same means and steps the engine is at 0.92 x the bound, the CPU
    float32 oracle at 0.85 x (max|diff| 1.7e-6) and the module route at 2.19 x: the comparison partner carries most of the
    deviation (Adam divides by sqrt(v) ~ |g| on weights whose gradient is near zero).  So the bound's second clause applies:
    4 x the float32 oracle's own deviation from float64, measured here on the same six steps (3.4 x the bound when written)."""
    from behavior_driven_video_synthesis_amd.experiments.vunet import DEFAULT_CONFIG, Vunet
    from behavior_driven_video_synthesis_amd.models.vunets import Regressor
    cfg = _small_cfg(DEFAULT_CONFIG)
    tr = Vunet(cfg, device="cuda:0", n_channels_x=3, vgg_width_div=8, total_steps=50, vgg_synthetic=True)
    arch = dict(cfg["architecture"], linear_width_factor=1, n_linear=2)
    widths = [64 // (2 ** (tr.vunet.n_scales - i)) for i in range(arch["n_latent_scales"], 0, -1)]

    def encode(batch, e):
        return tr.vunet.ed(tr.vunet.eu(batch.get("pose_img_inplane", batch["pose_img"])), e)[1]
    oracle_cfg = dict(n_out=34, n_latent_scales=2, nf_max=16, latent_widths=tuple(widths), linear_width_factor=1, n_linear=2, B=2)
    _check_probe(tr, encode, _probe_batches(64, 3), lambda: Regressor(34, latent_widths=widths, **arch).cuda(), oracle_cfg)


# ---- 7. training.fused_regressor
def test_fused_regressor_side_loop_matches_the_module_route():
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import DEFAULT_CONFIG, ShapePoseNet, synthetic_batch
    from synth import seeded_randn
    runs = {}
    for fused in (False, True):
        cfg = _small_cfg(DEFAULT_CONFIG, 32)
        cfg["training"].update(train_regressor=True, reg_steps=2, fused_regressor=fused)
        tr = ShapePoseNet(cfg, device="cuda:0", vgg_width_div=8, total_steps=50, vgg_synthetic=True, hip_graph=False)
        assert tr.fused_regressor == fused
        log = []
        for it in range(3):
            batch = synthetic_batch(2, 32, "cuda:0", seed=200 + it, with_regressor=True, reg_steps=2)
            with torch.no_grad():
                shapes = [tuple(m.shape) for m in tr.vunet.ed(tr.vunet.eu(batch["pose_img"]), None)[1]]
            eps = [seeded_randn(f"fr.eps.{it}.{s}", sh, 11).cuda() for s, sh in enumerate(shapes)]
            reg_eps = [[seeded_randn(f"fr.reg.{it}.{j}.{s}", sh, 11).cuda() for s, sh in enumerate(shapes)] for j in range(2)]
            log.append(tr.train_fn(batch, eps=eps, reg_eps=reg_eps)["loss_reg"].reshape(1).clone())
        runs[fused] = (torch.cat(log).cpu(), {k: v.cpu() for k, v in tr.regressor.state_dict().items()},
                       {k: v.cpu() for k, v in tr.vunet.state_dict().items()})
        if fused:
            with pytest.raises(RuntimeError, match="fused_regressor"):
                tr.enable_hip_graph()
            ck = tr.state_dict()["regressor"]                              # the engine's moments, torch.optim.Adam's layout
            assert len(ck["optimizer"]["state"]) == 8 and int(ck["optimizer"]["state"][0]["step"]) == 6
            tr.load_state_dict({"model": tr.vunet.state_dict(), "regressor": ck})
            assert tr._regressor_engine().adam.step == 6
            back = tr._regressor_engine().optimizer_state_dict()["state"]
            assert all(torch.equal(back[i]["exp_avg_sq"], ck["optimizer"]["state"][i]["exp_avg_sq"]) for i in range(8))
    _traj_close(runs[True][0].numpy(), runs[False][0].numpy(), "loss_regressor log")
    for k, v in runs[False][1].items():
        _traj_close(runs[True][1][k].numpy(), v.numpy(), f"regressor {k}")
    for k, v in runs[False][2].items():
        assert torch.equal(runs[True][2][k], v), k                         # the side loop contributes no gradient to the generator


# ---- 8. optimiser state round trip
def test_adam_moments_continue_in_torch_optim_adam():
    cfg, tag = R.CASES["small"], "small"
    batches = R.inputs(tag, cfg, 4)
    reg, eng = _run_engine(tag, 3)
    osd = eng.optimizer_state_dict()
    assert list(osd["state"]) == list(range(8)) and int(osd["state"][0]["step"]) == 3
    assert [tuple(s["exp_avg"].shape) for s in osd["state"].values()] == [tuple(p.shape) for p in reg.parameters()]
    sd = {k: v.detach().cpu().clone() for k, v in reg.state_dict().items()}
    params = {k: torch.nn.Parameter(v.clone()) for k, v in sd.items()}
    opt = torch.optim.Adam(list(params.values()), lr=1e-3)
    # (copies: torch.optim.Adam keeps the ``step`` tensors it is handed and advances them in place)
    osd_cpu = {"state": {i: {k: (v.detach().cpu().clone() if torch.is_tensor(v) else v) for k, v in s.items()} for i, s in osd["state"].items()},
               "param_groups": copy.deepcopy(osd["param_groups"])}
    opt.load_state_dict(osd_cpu)
    means, tgt = batches[3]
    _, _, g = R.grads(sd, cfg, means, tgt)
    for k, p in params.items():
        p.grad = g[k]
    opt.step()
    eng.step(*_cuda(batches[3]))
    eng.write_back()
    for k, v in reg.state_dict().items():
        _traj_close(v.cpu().numpy(), params[k].detach().numpy(), f"continued {k}")
    # and back: a second engine that loads the state continues as the first does
    reg2 = _module(cfg, sd)
    eng2 = reg2.probe_engine()
    eng2.load_optimizer_state_dict(osd)
    eng2.step(*_cuda(batches[3]))
    eng2.write_back()
    for k, v in reg.state_dict().items():
        assert torch.equal(v, reg2.state_dict()[k]), k


def test_more_than_two_latent_scales_are_refused_with_the_sentence():
    from behavior_driven_video_synthesis_amd.models.vunets import Regressor
    from behavior_driven_video_synthesis_amd.reg_probe import TOO_MANY_SCALES
    reg = Regressor(34, n_latent_scales=3, nf_max=16, latent_widths=[8, 4, 2], linear_width_factor=1).cuda()
    with pytest.raises(NotImplementedError, match="at most two latent scales"):
        reg.probe_engine()
    assert "module route" in TOO_MANY_SCALES
