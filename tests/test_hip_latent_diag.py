"""The latent diagnostics on the GPU (csrc/seq_latent.hip, latent_diag.py, lib.losses.FlowLoss, BehaviorNet.evaluate(...,
latent_diagnostics=...)): the KS kernel and the FlowLoss kernel against the float64 restatement (tests/latent_diag_ref.py) and
against what scipy and the reference's FlowLoss recorded (tests/golden/g20_latent_diag.npz), and the evaluation end to end."""
import copy
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import latent_diag_ref as R
from conftest import load_golden
from synth import seeded_randn, synth_behavior_state

pytestmark = pytest.mark.gpu

# D, D+, D-: derived, not measured.  Every term is a difference of numbers in [0, 1]; the only rounding is the float64 erfc, a few
# ulp, so the error is about 1e-15: anything larger means a wrong rank or a wrong element.
D_TOL = dict(rtol=0, atol=1e-12)
P_RTOL = 1e-10                     # the series' exp calls, where p > 1e-200
FLOW_RTOL = 1e-12                  # float64 accumulation over fp32 inputs on both sides: only the summation order differs
REF_LOG_TOL = dict(rel=2e-4, abs=2e-4)     # what tests/test_hip_seq_train.py holds the entries to against the reference's fp32 log


def _L():
    from behavior_driven_video_synthesis_amd import latent_diag
    return latent_diag


def _np(t):
    return t.detach().cpu().numpy()


def _ks_dict(ks):
    return {"statistic": _np(ks.statistic), "d_plus": _np(ks.d_plus), "d_minus": _np(ks.d_minus), "p_asymptotic": _np(ks.p_asymptotic)}


def _padded(x, col_major, pad):
    """x [N, C] host fp32 -> a device view of it inside a larger buffer whose other elements are NaN: a read outside the extent
    shows as a NaN result."""
    x = torch.as_tensor(x)
    n, c = x.shape
    if col_major:
        buf = torch.full((c, n + pad), math.nan)
        buf[:, :n] = x.t()
        return buf.cuda()[:, :n]
    buf = torch.full((n, c + pad), math.nan)
    buf[:, :c] = x
    return buf.cuda()[:, :c]


def _hold_ks(got, want, msg=""):
    for k in ("statistic", "d_plus", "d_minus"):
        np.testing.assert_allclose(got[k], want[k], err_msg=f"{msg} {k}", equal_nan=True, **D_TOL)
    p, q = got["p_asymptotic"], want["p_asymptotic"]
    big = q > 1e-200
    np.testing.assert_allclose(p[big], q[big], rtol=P_RTOL, atol=0, err_msg=f"{msg} p")
    rest = ~big & ~np.isnan(q)
    assert (p[rest] <= 1e-199).all(), msg
    assert np.array_equal(np.isnan(p), np.isnan(q)), msg


@functools.lru_cache(maxsize=None)
def _case(n, c):
    x = (seeded_randn(f"ks.case.{n}.{c}", (n, c), 7) * (1.0 + 0.25 * torch.arange(c)) + 0.1 * torch.arange(c)).numpy()
    return x, R.ks_table(x)


KS_SHAPES = [(n, c) for n in (1, 2, 63, 64, 65, 1000, 4097) for c in (1, 5, 33)] + [(32768, 1), (32768, 5), (32768, 2)]


# ---- 1. the KS kernel
@pytest.mark.parametrize("col_major", [False, True])
@pytest.mark.parametrize("n,c", KS_SHAPES)
def test_ks_statistic_vs_the_restatement(n, c, col_major):
    x, want = _case(n, c)
    got = _ks_dict(_L().ks_normal(_padded(x, col_major, 3 if col_major else 5), col_major=col_major))
    _hold_ks(got, want, f"N={n} C={c}")


@pytest.mark.parametrize("n", [64, 65, 1000])
def test_ks_on_the_fixture_columns_vs_scipy(n):
    meta, arr = load_golden("g20_latent_diag")
    x = R.golden_columns(n, meta["seed"])
    ks = _L().ks_normal(torch.from_numpy(x).cuda())
    got = _ks_dict(ks)
    np.testing.assert_allclose(got["statistic"], arr[f"ks.{n}.statistic"], rtol=0, atol=1e-12)      # the all-equal and +inf columns too
    want_p = arr[f"ks.{n}.p_asymptotic"]
    big = want_p > 1e-200
    np.testing.assert_allclose(got["p_asymptotic"][big], want_p[big], rtol=P_RTOL, atol=0)
    _hold_ks(got, R.ks_table(x), f"fixture N={n}")
    assert ks.n == n
    np.testing.assert_array_equal(ks.pvalues("asymptotic"), got["p_asymptotic"])


def test_ks_nan_column_propagates_and_leaves_the_others():
    x, want = _case(65, 5)
    x = x.copy()
    x[17, 1] = math.nan
    x[0, 3] = -math.nan
    x[5, 4], x[6, 4], x[7, 0] = math.inf, -math.inf, -math.inf
    want = R.ks_table(x)
    for col_major in (False, True):
        got = _ks_dict(_L().ks_normal(_padded(x, col_major, 2), col_major=col_major))
        for k in got:
            assert np.isnan(got[k][[1, 3]]).all() and not np.isnan(got[k][[0, 2, 4]]).any(), k
        _hold_ks(got, want, "nan")


def test_ks_sorted_route_and_the_route_taken():
    L = _L()
    from behavior_driven_video_synthesis_amd.ops import _call, _p, _stream
    n, c = 33000, 3
    x, want = _case(n, c)
    xs = torch.sort(torch.from_numpy(x).cuda(), dim=0)[0].contiguous()
    stat = torch.empty(3, c, device="cuda", dtype=torch.float64)
    p = torch.empty(c, device="cuda", dtype=torch.float64)
    _call("vunet_seq_ks_norm", _p(xs), c, 0, n, c, 1, _p(stat), _p(p), None, _stream())
    got = {"statistic": _np(stat[0]), "d_plus": _np(stat[1]), "d_minus": _np(stat[2]), "p_asymptotic": _np(p)}
    _hold_ks(got, want, "sorted=1")
    before = dict(L.ks_routes)
    _hold_ks(_ks_dict(L.ks_normal(torch.from_numpy(x).cuda())), want, "torch.sort route")
    assert L.ks_routes["torch_sort"] == before["torch_sort"] + 1 and L.ks_routes["lds"] == before["lds"]
    _hold_ks(_ks_dict(L.ks_normal(torch.from_numpy(x.T.copy()).cuda(), col_major=True)), want, "torch.sort route, column-major")
    x2, want2 = _case(32768, 2)
    before = dict(L.ks_routes)
    _hold_ks(_ks_dict(L.ks_normal(torch.from_numpy(x2).cuda())), want2, "lds route")
    assert L.ks_routes["lds"] == before["lds"] + 1 and L.ks_routes["torch_sort"] == before["torch_sort"]


def test_ks_two_runs_are_bit_identical():
    L = _L()
    for n, c in ((1000, 33), (32768, 2)):
        x = torch.from_numpy(_case(n, c)[0]).cuda()
        a, b = _ks_dict(L.ks_normal(x)), _ks_dict(L.ks_normal(x))
        for k in a:
            assert np.array_equal(a[k], b[k]), (n, c, k)


def test_argument_errors_launch_nothing():
    from behavior_driven_video_synthesis_amd import _lib
    lib = _lib.lib()
    x = torch.zeros(8, 4, device="cuda")
    stat = torch.full((3, 4), 7.0, device="cuda", dtype=torch.float64)
    p = torch.full((4,), 7.0, device="cuda", dtype=torch.float64)
    P = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    ERR_ARG, ERR_UNSUPPORTED = -1, -3
    assert lib.vunet_seq_ks_norm(None, 4, 0, 8, 4, 0, P(stat), P(p), None, None) == ERR_ARG
    assert lib.vunet_seq_ks_norm(P(x), 4, 0, 8, 4, 0, None, P(p), None, None) == ERR_ARG
    assert lib.vunet_seq_ks_norm(P(x), 4, 0, 8, 4, 0, P(stat), None, None, None) == ERR_ARG
    assert lib.vunet_seq_ks_norm(P(x), 4, 0, 0, 4, 0, P(stat), P(p), None, None) == ERR_ARG
    assert lib.vunet_seq_ks_norm(P(x), 4, 0, 8, 0, 0, P(stat), P(p), None, None) == ERR_ARG
    assert lib.vunet_seq_ks_norm(P(x), 3, 0, 8, 4, 0, P(stat), P(p), None, None) == ERR_ARG          # row-major: ld < C
    assert lib.vunet_seq_ks_norm(P(x), 7, 1, 8, 4, 0, P(stat), P(p), None, None) == ERR_ARG          # column-major: ld < N
    assert lib.vunet_seq_ks_norm(P(x), 40000, 1, 32769, 4, 0, P(stat), P(p), None, None) == ERR_UNSUPPORTED
    pr, sc = torch.full((2, 8), 7.0, device="cuda", dtype=torch.float64), torch.full((4,), 7.0, device="cuda", dtype=torch.float64)
    ld = torch.zeros(8, device="cuda")
    assert lib.vunet_seq_latent_nll(None, 4, P(ld), None, 8, 4, P(pr), P(sc), None) == ERR_ARG
    assert lib.vunet_seq_latent_nll(P(x), 4, None, None, 8, 4, P(pr), P(sc), None) == ERR_ARG
    assert lib.vunet_seq_latent_nll(P(x), 4, P(ld), None, 8, 4, None, P(sc), None) == ERR_ARG
    assert lib.vunet_seq_latent_nll(P(x), 4, P(ld), None, 8, 4, P(pr), None, None) == ERR_ARG
    assert lib.vunet_seq_latent_nll(P(x), 4, P(ld), None, 0, 4, P(pr), P(sc), None) == ERR_ARG
    assert lib.vunet_seq_latent_nll(P(x), 4, P(ld), None, 8, 0, P(pr), P(sc), None) == ERR_ARG
    assert lib.vunet_seq_latent_nll(P(x), 3, P(ld), None, 8, 4, P(pr), P(sc), None) == ERR_ARG
    torch.cuda.synchronize()
    for t in (stat, p, pr, sc):
        assert bool((t == 7.0).all())


# ---- 2. the FlowLoss kernel
@pytest.mark.parametrize("with_noise", [False, True])
@pytest.mark.parametrize("b,c", [(b, c) for b in (1, 5, 64, 70, 1025) for c in (1, 51, 1024)])
def test_flow_nll_vs_float64_torch(b, c, with_noise):
    z = 0.9 * seeded_randn(f"nll.{b}.{c}.z", (b, c), 3) + 0.1
    logdet = 3.0 * seeded_randn(f"nll.{b}.{c}.ld", (b,), 3) - 7.0
    noise = seeded_randn(f"nll.{b}.{c}.noise", (b, c), 3) if with_noise else None
    buf = torch.full((b, c + 5), math.nan)
    buf[:, :c] = z
    zd = buf.cuda()[:, :c]                                       # a padded leading dimension, read in place
    assert zd.stride(0) == c + 5
    res = _L().flow_nll(zd, logdet.cuda(), None if noise is None else noise.cuda())
    scalars, nll, log_prob = R.flow_entries(z, logdet, noise)
    got = _np(res.scalars)
    assert res.scalars.dtype == res.nll.dtype == res.log_prob.dtype == torch.float64
    np.testing.assert_allclose(got[[0, 2, 3]], scalars[[0, 2, 3]], rtol=FLOW_RTOL, atol=0)
    if with_noise:
        np.testing.assert_allclose(got[1], scalars[1], rtol=FLOW_RTOL, atol=0)
    else:
        assert math.isnan(got[1])                                # NULL noise: NaN in slot 1
    np.testing.assert_allclose(_np(res.nll), nll, rtol=FLOW_RTOL, atol=0)
    np.testing.assert_allclose(_np(res.log_prob), log_prob, rtol=FLOW_RTOL, atol=0)
    assert list(res.log()) == ["flow_loss", "reference_nll_loss", "nlogdet_loss", "nll_loss"]
    again = _L().flow_nll(zd, logdet.cuda(), None if noise is None else noise.cuda())
    for u, v in ((res.scalars, again.scalars), (res.nll, again.nll), (res.log_prob, again.log_prob)):
        assert np.array_equal(_np(u), _np(v), equal_nan=True)    # two runs are bit-identical


def _flow_inputs(meta, b):
    c, seed = meta["C"], meta["seed"]
    return 0.9 * seeded_randn(f"flow.{b}.gauss", (b, c, 1, 1), seed) + 0.1, 3.0 * seeded_randn(f"flow.{b}.logdet", (b,), seed) - 7.0


@pytest.mark.parametrize("b", [5, 70])
def test_flow_nll_and_the_module_vs_the_reference_log(b):
    from behavior_driven_video_synthesis_amd.lib import losses
    meta, arr = load_golden("g20_latent_diag")
    gauss, logdet = _flow_inputs(meta, b)
    noise = torch.from_numpy(arr[f"flow.{b}.noise"])
    want = meta["flow"][str(b)]
    res = _L().flow_nll(gauss.cuda(), logdet.cuda(), noise.cuda())          # [B, C, 1, 1] input
    log = res.log()
    for k in want:
        assert log[k] == pytest.approx(want[k], **REF_LOG_TOL), k
    # the module without a gradient: flow_nll's numbers, a 0-dim fp32 device loss
    with torch.no_grad():
        loss, mlog = losses.FlowLoss()(gauss.cuda(), logdet.cuda(), noise=noise.cuda())
    assert mlog == log and loss.is_cuda and loss.dim() == 0 and loss.dtype == torch.float32
    assert float(loss) == float(res.scalars[0].to(torch.float32))
    loss2, mlog2 = losses.FlowLoss()(gauss.cuda(), logdet.cuda(), noise=noise.cuda())      # grad mode on, nothing requires grad
    assert mlog2 == log and not loss2.requires_grad
    # drawn noise: the reference entry is the mean of a chi-square's half, C / 2 in expectation
    _, drawn = losses.FlowLoss()(gauss.cuda(), logdet.cuda())
    assert drawn["flow_loss"] == log["flow_loss"] and abs(drawn["reference_nll_loss"] - meta["C"] / 2) < 6 * math.sqrt(meta["C"] / 2 / b)
    # with a gradient: the reference's torch expression, differentiable
    g = gauss.cuda().requires_grad_(True)
    ld = logdet.cuda().requires_grad_(True)
    loss3, mlog3 = losses.FlowLoss()(g, ld, noise=noise.cuda())
    ref_loss, ref_log = losses.flow_loss_expression(gauss.cuda(), logdet.cuda(), noise.cuda().reshape(gauss.shape))
    assert mlog3 == ref_log and float(loss3.detach()) == float(ref_loss)
    for k in want:
        assert mlog3[k] == pytest.approx(want[k], **REF_LOG_TOL), k
    loss3.backward()
    np.testing.assert_allclose(_np(g.grad), (gauss / b).numpy(), rtol=1e-6, atol=0)
    np.testing.assert_allclose(_np(ld.grad), np.full(b, -1.0 / b, dtype=np.float32), rtol=1e-6, atol=0)


# ---- 3. the collector
def test_collector_is_column_major_and_read_in_place():
    L = _L()
    col = L.LatentCollector({"b": 5, "gaussian_samples": 5}, 20, "cuda")
    parts = [seeded_randn(f"col.{i}", (8, 5), 1) for i in range(2)]
    for p in parts:
        col.add("gaussian_samples", p.cuda())
    col.add("actions", torch.arange(8).cuda())
    want = torch.cat(parts)
    assert torch.equal(col.get("gaussian_samples").cpu(), want) and tuple(col.columns("gaussian_samples").shape) == (5, 16)
    cols = col.columns("gaussian_samples")
    assert cols.stride() == (20, 1) and cols.data_ptr() == col.buf["gaussian_samples"].data_ptr()
    assert col.get("b").shape == (0, 5) and col.get("actions").tolist() == list(range(8))
    _hold_ks(_ks_dict(L.ks_normal(cols, col_major=True)), R.ks_table(want.numpy()), "collector")
    col.add("gaussian_samples", seeded_randn("col.2", (8, 5), 1).cuda())      # past the initial capacity: grows, keeps the rows
    assert torch.equal(col.get("gaussian_samples")[:16].cpu(), want) and col.rows["gaussian_samples"] == 24


# ---- 4. end to end
def _narrow_model():
    from behavior_driven_video_synthesis_amd.experiments.behavior_net import BehaviorNet, DEFAULT_CONFIG
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["architecture"].update(dim_hidden_b=32, n_flows=2, flow_mid_channels_factor=2, flow_hidden_depth=1)
    torch.manual_seed(9)
    bn = BehaviorNet(cfg, n_kps=51, device="cuda:0", hip_graph=True)
    for mod in (bn.latent_flow, bn.net):
        sd = mod.state_dict()
        mod.load_state_dict(synth_behavior_state({k: list(v.shape) for k, v in sd.items()}, 9,
                                                 {k: v.cpu() for k, v in sd.items() if k.endswith("_shuffle_idx")}))
    return bn


def test_evaluate_with_latent_diagnostics_end_to_end():
    from behavior_driven_video_synthesis_amd import behavior_eval as E
    L = _L()
    bn = _narrow_model()
    n, h, bsz, t, skip, s = 51, 32, 8, 6, 4, 4
    g = torch.Generator().manual_seed(9)
    dims = 96
    mean, std = (torch.randn(dims, generator=g) * 300).double().numpy(), (50 + 200 * torch.rand(dims, generator=g)).double().numpy()
    stats = E.PoseStats(mean, std, list(range(dims - n)), device="cuda")
    batches = [{"keypoints": (0.5 * seeded_randn(f"ld{i}.kps", (bsz, t + 1, n), 9)).cuda(),
                "future_keypoints": (0.5 * seeded_randn(f"ld{i}.fut", (bsz, t + 1, n), 9)).cuda(),
                "action_labels": torch.arange(bsz) + 10 * i} for i in range(3)]
    z = [seeded_randn(f"ld{i}.z", (s, bsz // skip, h), 9).cuda() for i in range(3)]
    eps = [seeded_randn(f"ld{i}.eps", (bsz, h), 9).cuda() for i in range(3)]
    noise = [{k: seeded_randn(f"ld{i}.{k}", (bsz, h), 9).cuda() for k in ("prior", "flow", "reference")} for i in range(3)]
    plain = bn.evaluate(batches, stats, n_samples=s, skip=skip, z=z, eps=eps)
    assert plain.latent is None
    ev = bn.evaluate(batches, stats, n_samples=s, skip=skip, z=z, eps=eps, latent_diagnostics={"n_max": 20, "ks_method": "asymptotic"},
                     latent_noise=noise)
    extra = {"self_recon_eval", "flow_loss", "reference_nll_loss", "nlogdet_loss", "nll_loss", "ks_p_mean"}
    summ, base = ev.summary(), plain.summary()
    assert set(summ) == set(base) | extra and not set(base) & extra
    assert {k: summ[k] for k in base} == base                           # key for key, value for value
    assert set(ev.lists()) == set(plain.lists())
    # the same quantities from the public net / flow calls and the restatement
    flows, recons, kept = [], [], {k: [] for k in L.SETS}
    for i, (b_, e_, nz) in enumerate(zip(batches, eps, noise)):
        x_s, target = b_["keypoints"][:, :-1].contiguous(), b_["keypoints"][:, 1:].contiguous()
        with torch.no_grad():
            pred, _, _, b, mu, _, pre = bn.net(x_s, x_s, t, eps=e_)
            prior = bn.net(x_s, x_s, t, sample=True, eps=nz["prior"])[3]
            gauss, logdet = bn.latent_flow(b)
            fsamp = bn.latent_flow.reverse(nz["flow"]).reshape(bsz, h)
        flows.append(R.flow_entries(gauss.cpu(), logdet.cpu(), nz["reference"].cpu())[0])
        recons.append(float(torch.mean((pred - target) ** 2)))
        if (i + 1) * bsz < 20:                                          # strict: batches 0 and 1 (8 < 20, 16 < 20, not 24)
            for k, v in (("b", b), ("mu", mu), ("pre", pre), ("prior_samples", prior), ("flow_samples", fsamp),
                         ("gaussian_samples", gauss.reshape(bsz, h))):
                kept[k].append(v.reshape(bsz, -1).cpu())
    lat = ev.latent
    assert isinstance(lat, L.LatentDiagnostics)
    for k in L.SETS:
        assert lat.collector.rows[k] == 16, k
        assert torch.equal(lat.collector.get(k).cpu(), torch.cat(kept[k])), k
    assert lat.collector.get("actions").tolist() == list(range(8)) + list(range(10, 18))
    want_flow = np.mean(np.stack(flows), axis=0)
    for j, k in enumerate(L.FLOW_KEYS):
        assert summ[k] == pytest.approx(want_flow[j], rel=1e-12), k
        assert getattr(lat, k) == summ[k]
    assert summ["self_recon_eval"] == pytest.approx(sum(recons) / 3, rel=1e-6)      # fp32 batch values, as the reference's MSELoss
    want_ks = R.ks_table(torch.cat(kept["gaussian_samples"]).numpy())
    _hold_ks(_ks_dict(lat.ks), want_ks, "evaluate ks")
    assert lat.ks.n == 16 and summ["ks_p_mean"] == pytest.approx(float(np.mean(want_ks["p_asymptotic"])), rel=P_RTOL)
    # without a flow: the flow and KS entries are absent, not NaN
    nf = bn.evaluate(batches, stats, n_samples=s, skip=skip, use_flow=False, z=z, eps=eps, latent_diagnostics=True, latent_noise=noise[0])
    s2 = nf.summary()
    assert set(s2) - set(base) == {"self_recon_eval"} and s2["self_recon_eval"] == summ["self_recon_eval"]
    assert nf.latent.ks is None and nf.latent.collector.rows["b"] == 24 and "gaussian_samples" not in nf.latent.collector.rows
