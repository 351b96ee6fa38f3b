"""CPU checks of the behaviour model's sampling metrics: the float64 restatement (tests/behavior_eval_ref.py) against what the
reference's own classes and formulas produced (tests/golden/g13_behavior_eval.npz), its NaN and tie semantics, and the argument
checks of the public surface and the C ABI that run before any device work."""
import ctypes
import os

import numpy as np
import pytest
import torch

import behavior_eval_ref as R
from conftest import load_golden

CASES = ["flow_f64_s8", "flow_f32_s50", "prior_f64_s50", "prior_f32_s8", "tie_f64_s8"]


def _tol(meta, tag):
    # float64 statistics: the reference computes in float64 too; float32: its torch norms and numpy sums run in float32
    return dict(rtol=1e-12, atol=0) if meta["cases"][tag]["stats_dtype"] == "float64" else dict(rtol=1e-5, atol=0)


@pytest.mark.parametrize("tag", CASES)
def test_restatement_reproduces_the_reference_metrics(tag):
    meta, arr = load_golden("g13_behavior_eval")
    samples, future, mean, std, f32 = R.fixture_inputs(meta, arr, tag)
    c = meta["cases"][tag]
    assert samples.shape == (5, c["n_samples"], c["seq_len"], 51)
    got = R.metrics(samples, future, mean, std, f32)
    for k in ("APD", "ASD", "FSD", "minADE", "minFDE"):
        np.testing.assert_allclose(got[k], arr[f"{tag}.{k}"], err_msg=k, **_tol(meta, tag))
    for k in ("ADE", "FDE"):
        np.testing.assert_allclose(got[k], c[k], err_msg=k, **_tol(meta, tag))


@pytest.mark.parametrize("tag", ["flow_f64_s8", "prior_f32_s8"])
def test_unnormalisation_is_the_references(tag):
    """unNormalizeData with numpy's promotion: bit for bit, float32 statistics included."""
    meta, arr = load_golden("g13_behavior_eval")
    samples, future, mean, std, f32 = R.fixture_inputs(meta, arr, tag)
    u = R.unnormalise(samples, mean, std, f32).numpy()
    g = R.unnormalise(future[:, 1:], mean, std, f32).numpy()
    assert u.dtype == np.float64
    np.testing.assert_array_equal(u, arr[f"{tag}.reverted"].astype(np.float64))
    np.testing.assert_array_equal(g, arr[f"{tag}.reverted_gt"].astype(np.float64))


def test_the_tie_case_holds_two_identical_samples():
    meta, arr = load_golden("g13_behavior_eval")
    q, s = meta["cases"]["tie_f64_s8"]["tie"]
    x = arr["tie_f64_s8.samples"]
    np.testing.assert_array_equal(x[:, q], x[:, s])
    samples, future, mean, std, f32 = R.fixture_inputs(meta, arr, "tie_f64_s8")
    u = R.unnormalise(samples[0], mean, std, f32)
    a, f, *_ = R.pair_tables(u, u[0], f32)
    assert R.second(a.numpy())[q] == 0.0 and R.second(f.numpy())[s] == 0.0   # np.sort(...)[1] is the twin's 0, not the next


def _random(n_seq, s, t, n=51, seed=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n_seq, s, t, n, generator=g).numpy().astype(np.float32),
            torch.randn(n_seq, t + 1, n, generator=g).numpy().astype(np.float32),
            (torch.randn(n, generator=g) * 300).double().numpy(), (50 + 200 * torch.rand(n, generator=g)).double().numpy())


def test_nan_sample_semantics():
    """A NaN sample: its own row of A is all NaN (its ASD term is NaN, so is the sequence's ASD); in the other rows it sorts
    last and np.sort(...)[1] skips it; torch.min makes minADE NaN."""
    samples, future, mean, std = _random(2, 5, 4)
    samples[1, 3, 2, 7] = np.nan
    u = R.unnormalise(samples[1], mean, std, False)
    g = R.unnormalise(future[1, 1:], mean, std, False)
    a, f, p, ga, gf = R.pair_tables(u, g, False)
    a = a.numpy()
    assert np.isnan(a[3]).all() and np.isnan(a[:, 3]).all()
    sec = R.second(a)
    assert np.isnan(sec[3])
    for q in (0, 1, 2, 4):
        assert sec[q] == np.sort(np.delete(a[q], [q, 3]))[0]          # the nearest other sample, the NaN one ignored
    m = R.metrics(samples, future, mean, std, False)
    assert np.isnan(m["ASD"][1]) and np.isnan(m["APD"][1]) and np.isnan(m["minADE"][1])
    assert np.isfinite(m["ASD"][0]) and np.isfinite(m["minADE"][0]) and np.isnan(m["ADE"])
    # the NaN sits in frame 2 of 4: the final frame is clean, FSD and minFDE stay finite
    assert np.isfinite(m["FSD"][1]) and np.isfinite(m["minFDE"][1])


def test_ties_and_a_zero_distance_duplicate():
    samples, future, mean, std = _random(1, 6, 3, seed=1)
    samples[0, 4] = samples[0, 1]
    m = R.metrics(samples, future, mean, std, False)
    u = R.unnormalise(samples[0], mean, std, False)
    a, *_ = R.pair_tables(u, u[0], False)
    sec = R.second(a.numpy())
    assert sec[1] == 0.0 and sec[4] == 0.0 and (sec[[0, 2, 3, 5]] > 0).all()
    np.testing.assert_allclose(m["ASD"][0], sec.sum() / 6, rtol=1e-15)
    # only two samples, one NaN: fewer than two values that are not NaN in every row -> NaN
    two = samples[:, :2].copy()
    two[0, 1, 0, 0] = np.nan
    assert np.isnan(R.metrics(two, future, mean, std, False)["ASD"][0])


def test_fewer_than_two_samples_are_rejected():
    from behavior_driven_video_synthesis_amd import behavior_eval as E
    from behavior_driven_video_synthesis_amd import _lib
    samples, future, mean, std = _random(2, 2, 3)
    with pytest.raises(ValueError):
        R.metrics(samples[:, :1], future, mean, std, False)
    with pytest.raises(ValueError, match="n_samples"):
        E.sample_behaviors(None, None, torch.zeros(2, 3, 51), 1, 5)
    stats = E.PoseStats(np.zeros(96), np.ones(96), list(range(45)), device="cpu")
    assert stats.n_use == 51 and stats.f32_math == 0 and stats.mean.dtype == torch.float64
    with pytest.raises(ValueError, match="n_samples"):
        E.sample_metrics(torch.zeros(2, 1, 3, 51), torch.zeros(2, 4, 51), stats)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        E.sample_metrics(torch.zeros(2, 2, 3, 51), torch.zeros(2, 4, 51), stats)
    # the C ABI checks its arguments before any launch: these calls return without touching a device (the pointers are
    # never dereferenced)
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib, fake = _lib.lib(), ctypes.c_void_p(256)
    assert lib.vunet_seq_eval_pairs(fake, fake, fake, fake, 0, 2, 1, 3, 51, fake, None) == -1        # S < 2
    assert lib.vunet_seq_eval_pairs(fake, fake, fake, fake, 0, 2, 2, 0, 51, fake, None) == -1        # T < 1
    assert lib.vunet_seq_eval_pairs(None, fake, fake, fake, 0, 2, 2, 3, 51, fake, None) == -1        # NULL
    assert lib.vunet_seq_eval_pairs(fake, fake, fake, fake, 0, 2, 2, 200, 51, fake, None) == -3      # T n > 8192
    assert lib.vunet_seq_eval_select(fake, 2, 1, fake, fake, None) == -1
    assert lib.vunet_seq_eval_select(fake, 2, 2, None, fake, None) == -1
