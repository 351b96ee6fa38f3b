#!/usr/bin/env python3
"""Golden-vector generator for the post-hoc pose-regressor probe (g17).  Runs ONLY in the build container (needs the reference
checkout, as make_golden.py does, whose helpers it imports).

The reference's own ``models.vunets.Regressor`` in float32 on the CPU, driven for six steps the way ``run_inference`` drives it
(experiments/shape_and_pose_net.py:930, :971-977): ``Adam(regressor.parameters(), lr=0.001)`` on
``torch.mean(torch.norm(regressor(means) - reg_targets, dim=1))``.  Inputs and initial weights come from tests/reg_probe_ref.py
(``synth.seeded_randn``), so the fixture stores only results: the six losses, the predictions of step 1 and the first 512
values of every parameter after step 6.

    python tests/golden/make_golden_reg_probe.py      # regenerate tests/golden/g17_reg_probe.npz
"""
import os
import sys

import torch
from torch.optim import Adam

import make_golden  # noqa: F401  (puts the reference checkout on sys.path)
from make_golden import save

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import reg_probe_ref as R  # noqa: E402
from models.vunets import Regressor  # noqa: E402

KEEP = 512


def main():
    torch.set_num_threads(1)
    assert make_golden.REF
    meta, arrays = {"cases": {}, "steps": R.STEPS, "seed": R.SEED, "keep": KEEP}, {}
    for tag, cfg in R.CASES.items():
        regressor = Regressor(**R.model_kwargs(cfg))
        shapes = {k: list(v.shape) for k, v in regressor.state_dict().items()}
        assert shapes == R.shapes(cfg), (shapes, R.shapes(cfg))
        regressor.load_state_dict(R.init_state(cfg))
        optimizer_regressor = Adam(regressor.parameters(), lr=0.001)
        losses = []
        for t, (means, reg_targets) in enumerate(R.inputs(tag, cfg)):
            preds = regressor(means)
            loss_regressor = torch.mean(torch.norm(preds - reg_targets, dim=1))
            optimizer_regressor.zero_grad()
            loss_regressor.backward()
            optimizer_regressor.step()
            losses.append(loss_regressor.detach())
            if t == 0:
                arrays[f"{tag}.pred1"] = preds.detach().numpy().copy()
        arrays[f"{tag}.losses"] = torch.stack(losses).numpy()
        for k, v in regressor.state_dict().items():
            arrays[f"{tag}.param.{k}"] = v.detach().reshape(-1)[:KEEP].numpy().copy()
        meta["cases"][tag] = {"cfg": R.model_kwargs(cfg), "B": cfg["B"], "shapes": shapes}
    save("g17_reg_probe", meta, arrays)


if __name__ == "__main__":
    main()
