"""CPU: the plain-torch restatement of the pose-regressor probe (tests/reg_probe_ref.py) against the reference's own
``Regressor`` driven by ``torch.optim.Adam`` (tests/golden/g17_reg_probe.npz, written by make_golden_reg_probe.py)."""
import numpy as np
import pytest
import torch

import reg_probe_ref as R
from conftest import load_golden


@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_restatement_reproduces_the_reference_trajectory(tag):
    meta, arr = load_golden("g17_reg_probe")
    cfg = R.CASES[tag]
    assert meta["cases"][tag]["shapes"] == R.shapes(cfg) and meta["steps"] == R.STEPS
    losses, pred1, sd, _ = R.run(cfg, R.init_state(cfg), R.inputs(tag, cfg), torch.float32)
    np.testing.assert_allclose(losses.numpy(), arr[f"{tag}.losses"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(pred1.numpy(), arr[f"{tag}.pred1"], rtol=1e-5, atol=1e-6)
    for k, v in sd.items():
        np.testing.assert_allclose(v.reshape(-1)[:meta["keep"]].numpy(), arr[f"{tag}.param.{k}"], rtol=1e-5, atol=1e-6, err_msg=k)


@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_float64_run_agrees_with_float32_on_the_losses(tag):
    cfg = R.CASES[tag]
    l32, _, _, _ = R.run(cfg, R.init_state(cfg), R.inputs(tag, cfg), torch.float32)
    l64, _, _, _ = R.run(cfg, R.init_state(cfg), R.inputs(tag, cfg), torch.float64)
    rel = ((l32.double() - l64).abs() / l64.abs()).max()
    assert float(rel) < 1e-4, float(rel)


def test_a_row_that_matches_its_target_gets_zero_gradient():
    pred = torch.tensor([[1.0, 2.0], [3.0, 5.0]])
    tgt = torch.tensor([[1.0, 2.0], [0.0, 1.0]])
    loss, d = R.loss_and_dpred(pred, tgt)
    assert float(loss) == 2.5 and torch.equal(d[0], torch.zeros(2))
    p = pred.clone().requires_grad_(True)
    torch.norm(p - tgt, dim=1).mean().backward()
    assert torch.allclose(d, p.grad)
