"""The g12 fixture (tests/golden/make_golden_regressor.py) against a float64 CPU restatement of the regressor's inner loop:
step 0 of the shipped case rebuilt from the fixture's mu and indices with torch 1.3.1's ``.data`` Adam.  It must reproduce
L_1..5, the regressor's parameters and the adversarial gradient wrt mu -- and the variant that runs that gradient through the
weights before the fifth update (W^4) must miss it by far more than the GPU tests' tolerance."""
import numpy as np
import torch

from conftest import load_golden
from regressor_ref import KEYS, inner_steps, regressor_init, slice_of
from synth import seeded_randn


def _rel(a, b):
    a, b = torch.as_tensor(np.asarray(a)).double(), torch.as_tensor(np.asarray(b)).double()
    assert a.shape == b.shape, (a.shape, b.shape)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _step0():
    meta, arr = load_golden("g12_cvae_regressor")
    seed, case = meta["seed"], meta["cases"]["shipped"]
    bsz, t_len, n = meta["batch"], meta["seq_len"], meta["kw"]["n_kps"]
    kps = meta["kps_scale"][0] * seeded_randn("reg.kps0", (bsz, t_len + 1, n), seed)
    P0 = {k: v.double() for k, v in regressor_init(meta["reg_shapes"], seed).items()}
    mu = torch.as_tensor(arr["shipped.mu0"]).double()
    out = inner_steps(P0, mu, kps[:, :-1].double(), arr["idx"][0], case["w"], lr=meta["reg_lr"])
    return meta, arr, out


def test_fixture_shape_and_coverage():
    meta, arr = load_golden("g12_cvae_regressor")
    assert meta["seq_len"] == 50 and meta["kw"]["dim_hidden_b"] == 256 and meta["batch"] == 5 and meta["steps"] == 3
    assert set(meta["cases"]) == {"shipped", "w1", "cvae"}
    assert meta["cases"]["shipped"]["w"] == 0.01 and meta["cases"]["w1"]["w"] == 1.0 and meta["cases"]["cvae"]["cvae"]
    assert arr["idx"].shape == (3, 5) and arr["idx"].min() >= 0 and arr["idx"].max() < 50
    bands = {log["band"] for log in meta["cases"]["shipped"]["logs"]}
    assert {"<=0.45", "<=0.7"} <= bands, bands        # both clamp regimes of L_5 are exercised
    for tag, case in meta["cases"].items():
        assert case["reg_adam_step"] == 5 * meta["steps"]
        for log in case["logs"]:
            assert log["adv_w4_vs_w5"] > 1e-3, (tag, log["adv_w4_vs_w5"])   # W^4 vs W^5: far above the 3e-5 tolerance


def test_inner_loop_step0_reproduces_the_fixture():
    meta, arr, (ls, P, st, adv, adv4) = _step0()
    want = meta["cases"]["shipped"]["logs"][0]
    for got, ref in zip(ls, want["L"]):
        assert abs(got - ref) <= 2e-5 * abs(ref), (ls, want["L"])
    for k in KEYS:
        assert _rel(slice_of(P[k]), arr[f"shipped.reg0.{k}"]) <= 3e-5, k
        s, a = meta["reg_after_step0"][k]
        assert abs(float(P[k].abs().sum()) - a) <= 1e-5 * a, k
    assert all(s["step"] == 5 for s in st.values())
    assert _rel(adv, arr["shipped.adv0"]) <= 2e-5
    assert _rel(adv4, arr["shipped.adv4_0"]) <= 2e-5


def test_weights_before_the_fifth_update_miss_the_fixture():
    """The torch 1.3.1 semantics are observable: the W^4 answer is off by orders of magnitude more than the tolerance."""
    _, arr, (_, _, _, adv, adv4) = _step0()
    assert _rel(adv4, arr["shipped.adv0"]) > 100 * 2e-5
    assert _rel(adv, arr["shipped.adv0"]) <= 2e-5
