"""tests/behavior_interp_ref.py (the float64 restatement the slerp kernel is held to) against what the reference's own
``slerp`` wrote (tests/golden/g15_behavior_interp.npz): the fixture's float64 column bit for bit, the reference's
float32-path column within the distance the fixture recorded between the two.  No GPU."""
import numpy as np
import pytest

from conftest import load_golden

import behavior_interp_ref as R


@pytest.fixture(scope="module")
def g15():
    return load_golden("g15_behavior_interp")


@pytest.mark.parametrize("h", [1, 3, 64, 130, 1024])
def test_restatement_reproduces_the_float64_column_exactly(g15, h):
    meta, arr = g15
    out, mag = R.slerp_codes(arr[f"bare{h}.b1"], arr[f"bare{h}.b2"], np.asarray(meta["steps"]))
    assert out.dtype == np.float64 and out.shape == arr[f"bare{h}.f64"].shape == (2, 3, 6, h)
    assert np.array_equal(out, arr[f"bare{h}.f64"])
    assert np.all(np.abs(out) <= mag * (1 + 1e-15))


@pytest.mark.parametrize("h", [1, 3, 64, 130, 1024])
def test_restatement_is_within_the_recorded_gap_of_the_reference_column(g15, h):
    meta, arr = g15
    b1, b2 = arr[f"bare{h}.b1"], arr[f"bare{h}.b2"]
    out, _ = R.slerp_codes(b1, b2, np.asarray(meta["steps"]))
    scale = max(float(np.abs(b1).max()), float(np.abs(b2).max()))
    gap = float(np.abs(arr[f"bare{h}.ref"].astype(np.float64) - out).max() / scale)
    assert gap <= meta["f64_gap"][str(h)]
    assert meta["f64_gap"][str(h)] < 1e-6        # (the float32 path's omega: a few float32 roundings of O(1) codes)


def test_the_cases_are_what_the_kernel_tests_expect(g15):
    """Gaussian, near-parallel and identical pairs; the identical pair returns the code at every step; the end points return
    the two codes; the interpolated codes of the net's pairs are the restatement's too."""
    meta, arr = g15
    assert meta["bare_h"] == [1, 3, 64, 130, 1024] and meta["bare_kinds"] == ["gauss", "near", "same"]
    assert np.array_equal(np.asarray(meta["steps"]), R.DEFAULT_STEPS)
    for h in meta["bare_h"]:
        b1, b2, f64 = arr[f"bare{h}.b1"], arr[f"bare{h}.b2"], arr[f"bare{h}.f64"]
        assert np.array_equal(b1[2], b2[2]) and not np.array_equal(b1[1], b2[1])
        tol = 1e-14 * max(float(np.abs(b1).max()), float(np.abs(b2).max()))
        assert np.abs(f64[:, 2] - b1[2].astype(np.float64)).max() <= tol
        assert np.abs(f64[0, :, 0] - b1).max() <= tol and np.abs(f64[0, :, -1] - b2).max() <= tol
        assert np.abs(f64[1, :, 0] - b2).max() <= tol and np.abs(f64[1, :, -1] - b1).max() <= tol
    out, _ = R.slerp_codes(arr["pair.mu1"], arr["pair.mu2"])
    scale = max(float(np.abs(arr["pair.mu1"]).max()), float(np.abs(arr["pair.mu2"]).max()))
    assert np.abs(out - arr["pair.slerp"]).max() <= 1e-6 * scale
    assert arr["pair.rollouts"].shape == (2, meta["pairs"], 6, meta["t"], meta["net_kw"]["n_kps"])


def test_a_zero_row_gives_nan_rows_and_antisymmetric_steps_are_not_mirrored():
    z, b = np.zeros((1, 5), dtype=np.float32), np.arange(1, 6, dtype=np.float32)[None]
    out, _ = R.slerp_codes(z, b, [0.0, 0.5])
    assert np.isnan(out).all()
    rng = np.random.RandomState(3)
    b1, b2 = rng.randn(2, 7).astype(np.float32), rng.randn(2, 7).astype(np.float32)
    steps = [0.0, 0.1, 0.9, 1.0]
    out, _ = R.slerp_codes(b1, b2, steps)
    for s, v in enumerate(steps):
        assert np.array_equal(out[1, :, s], np.stack([R.slerp(v, b2[p], b1[p]) for p in range(2)]))
    assert not np.allclose(out[1, :, 1], out[0, :, 1])
