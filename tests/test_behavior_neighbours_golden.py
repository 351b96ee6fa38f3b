"""tests/behavior_neighbours_ref.py (the float64 restatement the nearest-neighbour kernels are held to) against what the
reference's numpy expressions wrote into tests/golden/g16_behavior_neighbours.npz: the same indices in both spaces, the
pose-space minima at float64 rounding (the fixture keeps the reference's mean pelvis, which cancels), the code-space minima
within the rounding bound of numpy's float32 norm.  No GPU."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden

import behavior_neighbours_ref as R


@pytest.fixture(scope="module")
def g16():
    return load_golden("g16_behavior_neighbours")


@pytest.fixture(scope="module")
def restated(g16):
    meta, arr = g16
    codes = R.argmin_rows(R.code_distances(arr["bank.mu"], arr["q.mu"]))
    poses = R.argmin_rows(R.pose_distances(arr["bank.kps"], arr["q.xs"], arr["stats.mean"], arr["stats.std"], meta["root"]))
    return codes, poses


def test_restatement_reproduces_the_reference_indices(g16, restated):
    meta, arr = g16
    (ci, _, _), (pi, _, _) = restated
    assert np.array_equal(ci, arr["codes.argmin"]) and np.array_equal(pi, arr["poses.argmin"])
    assert list(ci[:len(meta["near"])]) == meta["near"]          # the perturbed training sequences find their originals


def test_pose_minima_match_at_float64_rounding(g16, restated):
    _, arr = g16
    assert arr["poses.min"].dtype == np.float64
    np.testing.assert_allclose(restated[1][1], arr["poses.min"], rtol=1e-12, atol=0)


def test_code_minima_match_within_the_float32_norm_bound(g16, restated):
    """The fixture's value is numpy's float32 norm of float32 differences: H squares and a sum of H terms in float32 (pairwise,
    at most H / 2 roundings deep in the worst case) and a root -- (H / 2 + 2) 2^-24 relative."""
    meta, arr = g16
    h = meta["net_kw"]["dim_hidden_b"]
    assert arr["codes.min"].dtype == np.float32
    want = arr["codes.min"].astype(np.float64)
    worst = float(np.max(np.abs(restated[0][1] - want) / want))
    print(f"code minima: worst {worst:.3e} of bound {(h / 2 + 2) * 2.0 ** -24:.3e}")
    assert worst <= (h / 2 + 2) * 2.0 ** -24


def test_no_query_of_the_fixture_is_ambiguous(g16, restated):
    """Every gap between best and second best exceeds twice the bound the kernels are held to (and, in code space, twice the
    float32 norm's own): the cap on ambiguous queries is zero."""
    meta, arr = g16
    h, k = meta["net_kw"]["dim_hidden_b"], meta["t1"] * meta["j"] + 3
    (_, _, cgap), (_, _, pgap) = restated
    np.testing.assert_allclose(cgap, arr["codes.gap"], rtol=1e-9)
    np.testing.assert_allclose(pgap, arr["poses.gap"], rtol=1e-9)
    assert np.all(arr["codes.gap"] > 2 * max(R.bound(h), (h / 2 + 2) * 2.0 ** -24))
    assert np.all(arr["poses.gap"] > 2 * R.bound(k))


def test_the_fixture_is_what_the_kernel_tests_expect(g16):
    meta, arr = g16
    n, t1, q, h = meta["n_bank"], meta["t1"], meta["n_q"], meta["net_kw"]["dim_hidden_b"]
    assert arr["bank.kps"].shape == (n, t1, 3 * meta["j"]) and arr["bank.mu"].shape == (n, h)
    assert arr["q.xs"].shape == arr["q.beh"].shape == arr["q.start"].shape == (q, t1, 3 * meta["j"]) and arr["q.mu"].shape == (q, h)
    assert np.array_equal(arr["q.xs"][:, 0], arr["q.start"][:, 0])           # the start pose in front of the roll-out
    assert arr["stats.mean"].dtype == arr["stats.std"].dtype == np.float64 and meta["ignore"] == []
    # (numpy's float32 exp and torch's differ in the last place: the generator asserts torch's bit for bit)
    np.testing.assert_allclose(arr["q.b"], arr["q.eps"] * np.exp(arr["q.logstd"]) + arr["q.mu"], rtol=1e-5, atol=1e-6)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g16_behavior_neighbours.npz")) < 700 * 1024


def test_selection_rule_is_numpys_argmin():
    nan = float("nan")
    d = np.array([[3.0, 1.0, 1.0, 2.0], [2.0, nan, 0.0, nan], [nan, nan, nan, nan], [5.0, 5.0, 5.0, 5.0]])
    idx, best, gap = R.argmin_rows(d)
    assert idx.tolist() == [1, 1, 0, 0]
    assert best[0] == 1.0 and np.isnan(best[1]) and np.isnan(best[2]) and best[3] == 5.0
    assert gap[0] == 0.0 and gap[3] == 0.0
    assert R.argmin_rows(np.array([[4.0]]))[2][0] == np.inf


def test_distances_on_small_cases():
    """Hand-checkable values, NaN rows, float32 statistics and the cancelling translation."""
    bank = np.array([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0], [float("nan"), 0.0, 0.0]], dtype=np.float32)
    d = R.code_distances(bank, np.zeros((1, 3), dtype=np.float32))
    assert d[0, 0] == 0.0 and d[0, 1] == 5.0 and np.isnan(d[0, 2])
    rng = np.random.RandomState(0)
    x, y = rng.randn(5, 4, 9).astype(np.float32), rng.randn(2, 4, 9).astype(np.float32)
    mean, std = rng.randn(9) * 100.0, 1.0 + rng.rand(9)
    for root in (0, 2):
        want = R.pose_distances(x, y, mean, std, root)
        # a translation of every joint of a frame cancels in the root-centring: float64 statistics, up to rounding
        shift = mean + np.tile([1000.0, -500.0, 250.0], 3)
        np.testing.assert_allclose(R.pose_distances(x, y, shift, std, root), want, rtol=1e-11)
        # the definition, written out with numpy's own norm
        cx, cy = R.centred(x, mean, std, root), R.centred(y, mean, std, root)
        direct = np.stack([np.sum(np.linalg.norm(cy[a][None] - cx, axis=-1), axis=(1, 2)) for a in range(2)])
        np.testing.assert_allclose(want, direct, rtol=1e-13)
    f32 = R.pose_distances(x, y, mean.astype(np.float32), std.astype(np.float32), 0)
    np.testing.assert_allclose(f32, R.pose_distances(x, y, mean, std, 0), rtol=1e-4)
    assert not np.array_equal(f32, R.pose_distances(x, y, mean, std, 0))


def test_python_constants_mirror_the_header():
    from behavior_driven_video_synthesis_amd import neighbours as NB
    txt = open(os.path.join(ROOT, "include", "vunet_seq_nn.h")).read()
    macro = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (VUNET_NN_[A-Z_]+) (\d+)", txt)}
    assert macro == {"VUNET_NN_QT_CODES": NB.QT_CODES, "VUNET_NN_QT_POSES": NB.QT_POSES, "VUNET_NN_CHUNK": NB.CHUNK,
                     "VUNET_NN_MAX_H": NB.MAX_H, "VUNET_NN_MAX_TN": NB.MAX_TN}
