"""CPU checks of the real-vs-fake classifier study: the float64 restatement (tests/classifier_study_ref.py) against what the
reference's own Classifier / Regressor classes and inline loop produced in float32 (tests/golden/g14_classifier_study.npz)."""
import numpy as np
import pytest
import torch

import classifier_study_ref as R
from conftest import load_golden

# float32 against float64 over 30 SGD / Adam iterations through 12-step GRUs: the fixture's own rounding
TOL = dict(rtol=2e-4, atol=2e-5)


@pytest.mark.parametrize("tag", sorted(R.CASES))
def test_float64_restatement_reproduces_the_reference_study(tag):
    meta, arr = load_golden("g14_classifier_study")
    c = meta["cases"][tag]
    torch.set_num_threads(4)
    sets, init = R.inputs(tag)
    finals, curves = R.run(sets, init, c["times"], c["bs"], c["iterations"])
    for si in range(len(c["times"])):
        for k, v in curves[si].items():
            np.testing.assert_allclose(v, arr[f"{tag}.{si}.{k}"], err_msg=f"{si} {k}", **TOL)
        assert set(finals[si]) == set(c["final"][si])
        for k, v in finals[si].items():
            np.testing.assert_allclose(v, c["final"][si][k], err_msg=f"{si} {k}", **TOL)


def test_fixture_shape():
    meta, arr = load_golden("g14_classifier_study")
    for tag, c in meta["cases"].items():
        nit = c["iterations"] // (c["rows"] // c["bs"]) * (c["rows"] // c["bs"])
        keys = {"acc1", "loss1", "acc2", "loss2", "acc_self", "loss_regressor"} | ({"acc_flow", "loss_flow"} if c["flow"] else set())
        for si in range(len(c["times"])):
            assert {k.split(".", 2)[2] for k in arr if k.startswith(f"{tag}.{si}.")} == keys
            assert all(arr[f"{tag}.{si}.{k}"].shape == (nit,) for k in keys)
