"""Host tests (no GPU) of the FID restatements (tests/fid_ref.py) against tests/golden/g21_fid.npz, the reference's own
``_calculate_fid`` on the same seeded feature sets, and of the new header's prototypes."""
import ctypes

import numpy as np
import pytest

import fid_ref as R


@pytest.fixture(scope="module")
def g21(golden):
    return golden("g21_fid")[0]


def _bar(g21, case):
    return R.group_bar(g21, R.FULL_RANK if case in R.FULL_RANK else R.RANK_DEFICIENT)


def test_fixture_covers_every_case_and_both_groups_have_a_bar(g21):
    assert set(g21["cases"]) == set(R.CASES) and g21["seed"] == R.SEED
    for case, shape in R.CASES.items():
        assert tuple(g21["cases"][case]["shape"]) == shape
        assert max(g21["cases"][case]["iters"]) < 100
    # the bars come from the fixture: float64 round-off where the covariances have full rank, the conditioning of a square root
    # at zero (about the square root of round-off) where they do not
    assert 0.0 < R.group_bar(g21, R.FULL_RANK) < 1e-9
    assert R.group_bar(g21, R.FULL_RANK) < R.group_bar(g21, R.RANK_DEFICIENT) < 1e-5


def test_feature_sets_are_fp32_relu_with_dead_columns():
    x = R.feature_set("d256_dead", 0)
    assert x.dtype == np.float32 and x.shape == (1000, 256) and float(x.min()) == 0.0
    assert not x[:, :5].any() and x[:, 5:].any(axis=0).all()
    assert R.feature_set("d96_n17", 1).shape == (23, 96)
    assert np.array_equal(x, R.feature_set("d256_dead", 0))


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_restatements_agree_with_the_fixture(g21, case):
    """Recomputed here (this machine's BLAS / LAPACK) against the stored values and the stored reference: within the group's bar,
    which is what another summation order may move them by."""
    c, bar = g21["cases"][case], _bar(g21, case)
    gt, gen = R.feature_set(case, 0), R.feature_set(case, 1)
    sym = R.fid_sym(gt, gen)
    polar, iters, ok = R.fid_polar(gt, gen)
    assert ok and max(iters) < 100
    for got in (sym, polar):
        assert abs(got - c["fid_ref"]) <= bar * abs(c["fid_ref"]), (got, c)
    assert abs(sym - c["fid_sym"]) <= bar * abs(c["fid_ref"]) and abs(polar - c["fid_polar"]) <= bar * abs(c["fid_ref"])


def test_package_host_route_agrees_with_the_fixture(g21):
    from behavior_driven_video_synthesis_amd.lib.metrics import fid_from_features
    c = g21["cases"]["d64"]
    got = fid_from_features(R.feature_set("d64", 0), R.feature_set("d64", 1))
    assert abs(got - c["fid_ref"]) <= R.group_bar(g21, R.FULL_RANK) * abs(c["fid_ref"])


def test_polar_trace_is_the_nuclear_norm_and_the_square_root():
    b = R.feature_set("d50_odd", 0).astype(np.float64)[:, :20]
    t, h, iters, ok = R.polar_trace(b, want_h=True)
    s = np.linalg.svd(b, compute_uv=False)
    assert ok and abs(t - s.sum()) <= 1e-12 * s.sum()
    assert np.abs(h @ h - b.T @ b).max() <= 1e-11 * np.abs(b.T @ b).max()
    tw, _, _, okw = R.polar_trace(b.T.copy())          # fewer rows than columns: the other branch, same norm
    assert okw and abs(tw - s.sum()) <= 1e-12 * s.sum()
    assert R.polar_trace(np.zeros((3, 5)))[0] == 0.0


def test_prototypes_parse_from_the_header():
    from behavior_driven_video_synthesis_amd import _lib
    protos = _lib.declared_prototypes()
    vp, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_double
    assert protos["vunet_f64_gemm"] == [vp, i64, vp, i64, vp, i64, i32, i32, i32, i32, i32, f64, f64, vp]
    assert protos["vunet_fid_center"] == [vp, i32, i32, vp, vp, vp] == protos["vunet_fid_center_f64"]
    assert protos["vunet_f64_dot"] == [vp, vp, i64, vp, vp, vp]
    assert protos["vunet_f64_scale"] == [vp, i64, f64, vp, vp]
    assert protos["vunet_f64_symmetrize"] == [vp, i32, i64, vp]
    lib = _lib.lib()
    for name in ("vunet_f64_gemm", "vunet_fid_center", "vunet_fid_center_f64", "vunet_f64_dot", "vunet_f64_scale", "vunet_f64_symmetrize"):
        assert getattr(lib, name).argtypes == protos[name]
    assert lib.vunet_abi_version() == 12


def test_save_metric_ckpt_writes_the_fid_names(tmp_path):
    import os
    import torch
    from behavior_driven_video_synthesis_amd.experiments.checkpoint import save_metric_ckpt

    class Tr:
        def state_dict(self):
            return {"model": {"w": torch.ones(2)}, "optimizer": {"state": {}, "param_groups": []}}
    ssim, fid, is_rec = 0.7998303726877782, 31.489000461195474, 3.25
    paths = save_metric_ckpt(str(tmp_path), Tr(), 23, ssim, is_rec, fid=fid)
    d = os.path.join(str(tmp_path), "epoch_ckpts")
    assert paths == (os.path.join(d, f"model@e23@ssim={ssim}-fid={fid}.pth"), os.path.join(d, f"opt@e23@ssim={ssim}-fid={fid}.pth"))
    assert sorted(os.listdir(d)) == sorted(os.path.basename(p) for p in paths)
    assert torch.equal(torch.load(paths[0])["w"], torch.ones(2))
    paths = save_metric_ckpt(str(tmp_path / "plain"), Tr(), 23, ssim, is_rec)
    assert os.path.basename(paths[0]) == f"model@e23@ssim={ssim}-is={is_rec}.pth"
