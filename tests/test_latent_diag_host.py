"""The latent diagnostics without a GPU: the float64 restatement (tests/latent_diag_ref.py) against what scipy and the
reference's FlowLoss recorded (tests/golden/g20_latent_diag.npz), the p-value methods of ``KSResult``, ``lib.losses.FlowLoss``'s
host-side contract, and that an evaluation without the flag adds no key."""
import math
import os
import re

import numpy as np
import pytest
import torch

import latent_diag_ref as R
from conftest import ROOT, load_golden
from synth import seeded_randn

KS_ROWS = (64, 65, 1000)


def _flow_inputs(meta, b):
    c, seed = meta["C"], meta["seed"]
    gauss = 0.9 * seeded_randn(f"flow.{b}.gauss", (b, c, 1, 1), seed) + 0.1
    logdet = 3.0 * seeded_randn(f"flow.{b}.logdet", (b,), seed) - 7.0
    return gauss, logdet


@pytest.mark.parametrize("n", KS_ROWS)
def test_restatement_matches_the_recorded_scipy_statistic_and_asymptotic_p(n):
    meta, arr = load_golden("g20_latent_diag")
    got = R.ks_table(R.golden_columns(n, meta["seed"]))
    np.testing.assert_allclose(got["statistic"], arr[f"ks.{n}.statistic"], rtol=0, atol=1e-13)
    want = arr[f"ks.{n}.p_asymptotic"]
    big = want > 1e-300
    assert big.sum() >= 5
    np.testing.assert_allclose(got["p_asymptotic"][big], want[big], rtol=1e-12, atol=0)
    assert (got["p_asymptotic"][~big] <= 1e-300).all()


def test_kolmogorov_series_small_and_large_arguments():
    assert R.kolmogorov_sf(0.0) == 1.0 and math.isnan(R.kolmogorov_sf(math.nan))
    assert R.kolmogorov_sf(0.05) == 1.0
    # the two forms agree where both are accurate (the switch at t = 0.2 is not a jump)
    assert abs(R.kolmogorov_sf(0.2 - 1e-12) - R.kolmogorov_sf(0.2)) < 1e-14
    # 2 exp(-2 t^2) alone once the second term is below rounding
    assert R.kolmogorov_sf(5.0) == pytest.approx(2.0 * math.exp(-50.0), rel=1e-14)
    from behavior_driven_video_synthesis_amd import latent_diag as L
    for t in (0.0, 0.05, 0.19, 0.2, 0.5, 1.0, 3.0, 30.0):
        assert L.kolmogorov_sf(t) == R.kolmogorov_sf(t)


def _ks_result(n, meta, arr):
    """A KSResult over the restatement's numbers (host tensors: ``pvalues`` only copies them)."""
    from behavior_driven_video_synthesis_amd import latent_diag as L
    got = R.ks_table(R.golden_columns(n, meta["seed"]))
    t = {k: torch.from_numpy(v) for k, v in got.items()}
    return L.KSResult(t["statistic"], t["d_plus"], t["d_minus"], t["p_asymptotic"], n)


def test_reference_rule_takes_both_branches_on_the_fixture():
    from behavior_driven_video_synthesis_amd import latent_diag as L
    meta, arr = load_golden("g20_latent_diag")
    taken = {}
    for n in KS_ROWS:
        p = arr[f"ks.{n}.p_asymptotic"]
        take = L.reference_rule_takes_asymptotic(n, p)
        assert take.tolist() == [R.reference_rule_takes_asymptotic(n, float(v)) for v in p]
        assert take.tolist() == (p > 0.80 - 0.0003 * n).tolist()
        taken[n] = bool(take[0])
    assert taken == {64: False, 65: True, 1000: True}      # the standard-normal column: ksone at 64, asymptotic at 65 and 1000
    assert L.reference_rule_takes_asymptotic(2667, np.array([0.0])).all()
    assert not L.reference_rule_takes_asymptotic(2666, np.array([0.0])).any()


def test_asymptotic_method_needs_no_scipy_and_large_n_neither(monkeypatch):
    import sys
    from behavior_driven_video_synthesis_amd import latent_diag as L
    meta, arr = load_golden("g20_latent_diag")
    monkeypatch.setitem(sys.modules, "scipy", None)          # any import of scipy raises
    ks = _ks_result(65, meta, arr)
    np.testing.assert_array_equal(ks.pvalues("asymptotic"), ks.p_asymptotic.numpy())
    big = L.KSResult(ks.statistic, ks.d_plus, ks.d_minus, ks.p_asymptotic, 2667)
    np.testing.assert_array_equal(big.pvalues("reference"), ks.p_asymptotic.numpy())
    assert big.p_mean() == float(np.mean(ks.p_asymptotic.numpy()))
    with pytest.raises(ValueError):
        ks.pvalues("approx")


@pytest.mark.parametrize("n", KS_ROWS)
def test_exact_and_reference_methods_against_scipy(n):
    pytest.importorskip("scipy")
    meta, arr = load_golden("g20_latent_diag")
    ks = _ks_result(n, meta, arr)
    want = arr[f"ks.{n}.pvalue"]
    # the same scipy function on a D that may differ from scipy's own by 1e-13 (above): |d ln p / dD| <= 4 N D <= 2800 here, so
    # 3e-10 relative at the most
    np.testing.assert_allclose(ks.pvalues("exact"), want, rtol=1e-9, atol=1e-300)
    ref = ks.pvalues()
    take = arr[f"ks.{n}.p_asymptotic"] > 0.80 - 0.0003 * n
    np.testing.assert_allclose(ref[take], arr[f"ks.{n}.p_asymptotic"][take], rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(ref[~take], arr[f"ks.{n}.two_ksone"][~take], rtol=1e-9, atol=1e-300)
    assert (ref <= 1.0).all()
    assert ks.p_mean() == float(np.mean(ref))


@pytest.mark.parametrize("b", [5, 70])
def test_flow_entries_restatement_and_the_torch_expression_against_the_reference_log(b):
    from behavior_driven_video_synthesis_amd.lib import losses
    meta, arr = load_golden("g20_latent_diag")
    gauss, logdet = _flow_inputs(meta, b)
    noise = torch.from_numpy(arr[f"flow.{b}.noise"])
    want = meta["flow"][str(b)]
    scalars, nll, log_prob = R.flow_entries(gauss, logdet, noise)
    keys = ("flow_loss", "reference_nll_loss", "nlogdet_loss", "nll_loss")
    assert tuple(want) == keys
    for j, k in enumerate(keys):
        assert scalars[j] == pytest.approx(want[k], rel=2e-4, abs=2e-4), k      # the reference's log is an fp32 computation
    np.testing.assert_allclose(log_prob, -nll + logdet.double().numpy() - 0.5 * meta["C"] * math.log(2 * math.pi), rtol=1e-15)
    assert math.isnan(R.flow_entries(gauss, logdet)[0][1])
    # the expression the grad path evaluates gives the reference's entries: both are fp32 sums of C = 24 squares per row and of
    # B <= 70 rows, so they agree to (24 + 70) x 2^-24 = 6e-6 relative at the worst
    g = gauss.clone().requires_grad_(True)
    loss, log = losses.flow_loss_expression(g, logdet, noise)
    assert tuple(log) == keys and all(isinstance(v, float) for v in log.values())
    for k in keys:
        assert log[k] == pytest.approx(want[k], rel=6e-6, abs=0), k
    assert float(loss.detach()) == log["flow_loss"] and loss.dtype == torch.float32
    loss.backward()
    np.testing.assert_allclose(g.grad.numpy(), (gauss / b).numpy(), rtol=1e-6)


def test_flow_loss_module_contract_on_the_host():
    from behavior_driven_video_synthesis_amd.lib import losses
    fl = losses.FlowLoss()
    assert isinstance(fl, torch.nn.Module) and not list(fl.parameters())
    with pytest.raises(AssertionError):
        fl(torch.zeros(3, 4, 1, 1), torch.zeros(3, 1))
    for grad in (False, True):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fl(torch.zeros(3, 4, 1, 1, requires_grad=grad), torch.zeros(3))
    from behavior_driven_video_synthesis_amd import latent_diag as L
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.flow_nll(torch.zeros(3, 4), torch.zeros(3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.ks_normal(torch.zeros(3, 4))


def test_evaluator_without_latent_diagnostics_adds_no_key():
    from behavior_driven_video_synthesis_amd import behavior_eval as E
    from behavior_driven_video_synthesis_amd import latent_diag as L
    ev = E.BehaviorEvaluator()
    ev.add({"APD": torch.tensor([1.0, 3.0]), "ASD": torch.tensor([2.0, 2.0]), "FSD": torch.tensor([0.5, 1.5]),
            "ADE": torch.tensor(4.0), "FDE": torch.tensor(5.0)})
    assert ev.latent is None
    assert ev.summary() == {"APD": 2.0, "ASD": 2.0, "FSD": 1.0, "ADE": 4.0, "FDE": 5.0}
    assert set(ev.lists()) == {"APD", "ASD", "FSD", "ADE", "FDE"}
    # with the flag: exactly the six additions (with a flow), one without; lists() unchanged
    lat = L.LatentDiagnostics(None, 20, "asymptotic", True)
    lat.recon += [torch.tensor(1.0), torch.tensor(2.0)]
    lat.flow_scalars += [torch.tensor([1.0, 2.0, 3.0, 4.0], dtype=torch.float64), torch.tensor([3.0, 4.0, 5.0, 6.0], dtype=torch.float64)]
    lat.ks = L.KSResult(*(torch.tensor([0.1, 0.2], dtype=torch.float64),) * 3, torch.tensor([0.25, 0.75], dtype=torch.float64), 10)
    ev.latent = lat
    s = ev.summary()
    assert set(s) - {"APD", "ASD", "FSD", "ADE", "FDE"} == {"self_recon_eval", "flow_loss", "reference_nll_loss", "nlogdet_loss",
                                                            "nll_loss", "ks_p_mean"}
    assert (s["self_recon_eval"], s["flow_loss"], s["nll_loss"], s["ks_p_mean"]) == (1.5, 2.0, 5.0, 0.5)
    assert lat.ks_p_mean == 0.5 and lat.flow_loss == 2.0
    assert set(ev.lists()) == {"APD", "ASD", "FSD", "ADE", "FDE"}
    no_flow = L.LatentDiagnostics(None, 20, "reference", False)
    no_flow.recon.append(torch.tensor(2.0))
    assert no_flow.summary() == {"self_recon_eval": 2.0}
    assert lat.admits(0, 8) and lat.admits(1, 8) and not lat.admits(2, 8) and not L.LatentDiagnostics(None, 16, "exact", True).admits(1, 8)


def test_header_declares_the_two_entry_points():
    from behavior_driven_video_synthesis_amd import _lib
    names = _lib.declared_symbols()
    assert "vunet_seq_latent_nll" in names and "vunet_seq_ks_norm" in names
    txt = open(os.path.join(ROOT, "include", "vunet_seq_latent.h")).read()
    assert re.search(r"#define\s+VUNET_SEQ_KS_MAX_LDS_N\s+32768", txt)
    from behavior_driven_video_synthesis_amd import latent_diag as L
    assert L.KS_MAX_LDS_N == 32768
    protos = _lib.declared_prototypes()
    assert len(protos["vunet_seq_latent_nll"]) == 9 and len(protos["vunet_seq_ks_norm"]) == 10
