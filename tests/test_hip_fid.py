"""-m gpu: the FID statistic on the device (csrc/fid.hip, fid_device.py) -- the float64 MFMA GEMM's lane map on exact integer
data, its rounding against np.longdouble under the plain summation bound, the moments, ``fid_device`` on every case of
tests/golden/g21_fid.npz under bars taken from the fixture's own host methods, the degenerate inputs, and the routes through
``compute_fid(on_device=True)``, ``ShapePoseNet.evaluate(fid_extractor=...)`` and ``save_metric_ckpt(fid=...)``."""
import copy
import math
import os
import warnings

import numpy as np
import pytest
import torch

import fid_ref as R
from synth import seeded_randn

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
FORMS = {"NN": (False, False), "TN": (True, False), "NT": (False, True), "TT": (True, True)}
SHAPES = [(16, 16, 4), (33, 17, 5), (50, 131, 77)]          # (M, N, K)
BIG = (256, 256, 1000)


@pytest.fixture(scope="module")
def g21(golden):
    return golden("g21_fid")[0]


@pytest.fixture(scope="module")
def bars(g21):
    return {"full": R.group_bar(g21, R.FULL_RANK), "deficient": R.group_bar(g21, R.RANK_DEFICIENT)}


def _stored(a, b, form):
    """The logical operands op(a) [M, K], op(b) [K, N] as the form stores them, on the device."""
    ta, tb = FORMS[form]
    return (torch.from_numpy(np.ascontiguousarray(a.T if ta else a)).cuda(), torch.from_numpy(np.ascontiguousarray(b.T if tb else b)).cuda(),
            ta, tb)


_REALS = {}


def _reals(shape):
    """Seeded real operands of a shape and their np.longdouble product, computed once and shared by the forms."""
    if shape not in _REALS:
        m, n, k = shape
        a = seeded_randn(f"fid.gemm.a.{shape}", (m, k), 21).double().numpy()
        b = seeded_randn(f"fid.gemm.b.{shape}", (k, n), 21).double().numpy()
        _REALS[shape] = (a, b) + R.gemm_longdouble(a, b, False, False)
    return _REALS[shape]


# ---------------------------------------------------------------------------------------------------------------- 1. lane map
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("shape", SHAPES)
def test_gemm_is_exact_on_small_integers(shape, form):
    """Integer operands in [-8, 8]: every product and partial sum is an integer far below 2^53, so any summation order gives the
    int64 result bit for bit -- and a wrong lane map does not (the f32 row formula would misplace 3 rows of every 4)."""
    from behavior_driven_video_synthesis_amd.fid_device import gemm_f64
    m, n, k = shape
    a = torch.round(seeded_randn(f"fid.int.a.{shape}", (m, k), 3) * 4).clamp(-8, 8).double().numpy()
    b = torch.round(seeded_randn(f"fid.int.b.{shape}", (k, n), 3) * 4).clamp(-8, 8).double().numpy()
    # make the operand distinguish every (row, k) and (k, column): a rank-one ramp on top of the noise
    a += np.arange(m)[:, None] * 16.0 + np.arange(k)[None, :]
    b += np.arange(n)[None, :] * 32.0 - np.arange(k)[:, None]
    da, db, ta, tb = _stored(a, b, form)
    for alpha, diag in ((1, 0), (-3, 7)):
        got = gemm_f64(da, db, ta, tb, alpha=alpha, diag=diag).cpu().numpy()
        want = R.gemm_exact_int(a, b, False, False, alpha, diag)
        assert got.shape == want.shape and np.array_equal(got, want.astype(np.float64)), (shape, form, alpha, diag)


# ---------------------------------------------------------------------------------------------------------------- 2. rounding
@pytest.mark.parametrize("form", sorted(FORMS))
@pytest.mark.parametrize("shape", SHAPES + [BIG])
def test_gemm_rounding_padding_and_repeatability(shape, form):
    """|C - exact| <= (K + 2) 2^-53 sum_k |a_k b_k| per element: the bound of plain recursive summation of K products (K - 1
    additions and one rounding per product, any order), with room for the exact reference's own rounding to float64.  C is a
    window of a larger sentinel-filled buffer (ldc > N): nothing outside the window is written.  Two runs agree bit for bit."""
    from behavior_driven_video_synthesis_amd.fid_device import gemm_f64
    m, n, k = shape
    a, b, exact, mag = _reals(shape)
    da, db, ta, tb = _stored(a, b, form)
    sentinel = -1234.5
    buf = torch.full((m + 2, n + 3), sentinel, device="cuda", dtype=torch.float64)
    out = buf[1:m + 1, 2:n + 2]
    gemm_f64(da, db, ta, tb, out=out)
    host = buf.cpu().numpy()
    got = host[1:m + 1, 2:n + 2].copy()
    err = np.abs(got.astype(np.longdouble) - exact)
    bound = (k + 2) * U * mag
    print(f"gemm {form} {shape}: max err / bound = {float((err / bound).max()):.3e}")
    assert (err <= bound).all()
    host[1:m + 1, 2:n + 2] = sentinel
    assert (host == sentinel).all()
    again = gemm_f64(da, db, ta, tb)
    assert torch.equal(again, out)
    # alpha and diag on real data: v = alpha acc, then + diag on the diagonal (two more roundings)
    c2 = gemm_f64(da, db, ta, tb, alpha=-0.5, diag=1.5).cpu().numpy()
    want2 = -0.5 * got
    want2[np.arange(min(m, n)), np.arange(min(m, n))] += 1.5
    assert np.array_equal(c2, want2)


@pytest.mark.parametrize("rows,cols", [(77, 50), (1000, 256), (5, 131)])
def test_gram_matrix_is_bit_symmetric(rows, cols):
    from behavior_driven_video_synthesis_amd.fid_device import gemm_f64
    x = seeded_randn(f"fid.gram.{rows}.{cols}", (rows, cols), 5).double().cuda()
    g = gemm_f64(x, x, trans_a=True)
    assert g.shape == (cols, cols) and torch.equal(g, g.t())
    g = gemm_f64(x, x, trans_b=True, alpha=-0.5, diag=1.5)
    assert g.shape == (rows, rows) and torch.equal(g, g.t())


def test_gemm_rejects_what_it_cannot_run():
    from behavior_driven_video_synthesis_amd.fid_device import gemm_f64
    x = torch.zeros(4, 3, device="cuda", dtype=torch.float64)
    with pytest.raises(ValueError):
        gemm_f64(x, x)
    with pytest.raises(ValueError):
        gemm_f64(x.float(), x.float(), trans_a=True)
    with pytest.raises(RuntimeError):
        gemm_f64(x.cpu(), x.cpu(), trans_a=True)


# ---------------------------------------------------------------------------------------------------------------- 3. moments
@pytest.mark.parametrize("case,which", [("d50_odd", 0), ("d50_odd", 1), ("d256_dead", 0), ("d96_n17", 1), ("d48_n2", 0)])
def test_feature_moments(case, which):
    """Mean: e = (N + 2) 2^-53 sum |x| per column (N - 1 additions, the division, the reference's own rounding).  Covariance, the
    GEMM bound carried through the centring: with y = (x - mu) / sqrt(N - 1) exact, the device's y is off by the mean's error
    e_j / sqrt(N - 1) and by three roundings (subtraction, square root, division); a product of two is off by 6 * 2^-53 and the
    GEMM adds (N + 2) 2^-53, in all (N + 8) 2^-53 sum_n |y_ni y_nj|, and np.cov carries as much: (2 N + 16) 2^-53 sum_n |y_ni y_nj|.
    The mean's error enters through sum_n y_ni e_j / sqrt(N - 1), bounded by s_i e_j with s_i = sum_n |y_ni| / sqrt(N - 1)."""
    from behavior_driven_video_synthesis_amd.fid_device import feature_moments
    x = R.feature_set(case, which)
    n = x.shape[0]
    mu, cov = feature_moments(torch.from_numpy(x).cuda())
    assert mu.dtype == torch.float64 and cov.dtype == torch.float64 and torch.equal(cov, cov.t())
    xd = x.astype(np.float64)
    want_mu, want_cov = np.mean(xd, axis=0), np.atleast_2d(np.cov(xd, rowvar=False))
    e = (n + 2) * U * np.abs(xd).sum(axis=0)
    err_mu = np.abs(mu.cpu().numpy() - want_mu)
    assert (err_mu <= e).all()
    y = np.abs(xd - want_mu) / math.sqrt(n - 1)
    s = y.sum(axis=0) / math.sqrt(n - 1)
    bound = (2 * n + 16) * U * (y.T @ y) + np.outer(e, s) + np.outer(s, e)
    err = np.abs(cov.cpu().numpy() - want_cov)
    print(f"moments {case}[{which}]: mean err / bound {float((err_mu / np.maximum(e, 1e-300)).max()):.3e}, "
          f"cov err / bound {float((err / np.maximum(bound, 1e-300)).max()):.3e}")
    assert (err <= bound).all()
    # float64 features take the same route
    mu64, cov64 = feature_moments(torch.from_numpy(xd).cuda())
    assert torch.equal(mu64, mu) and torch.equal(cov64, cov)


# ---------------------------------------------------------------------------------------------------------------- 4. the statistic
@pytest.mark.parametrize("case", sorted(R.CASES))
def test_fid_device_on_the_fixture(case, g21, bars):
    from behavior_driven_video_synthesis_amd.fid_device import fid_device
    c = g21["cases"][case]
    bar = bars["full" if case in R.FULL_RANK else "deficient"]
    gt, gen = torch.from_numpy(R.feature_set(case, 0)).cuda(), torch.from_numpy(R.feature_set(case, 1)).cuda()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = fid_device(gt, gen)
    dist = abs(res.fid - c["fid_ref"]) / abs(c["fid_ref"])
    print(f"fid_device {case}: fid {res.fid!r} ref {c['fid_ref']!r} distance {dist:.3e} bar {bar:.3e} iters {res.iters} "
          f"(numpy {c['iters']}); host methods: sym {abs(c['fid_sym'] - c['fid_ref']) / abs(c['fid_ref']):.3e} "
          f"polar {abs(c['fid_polar'] - c['fid_ref']) / abs(c['fid_ref']):.3e}")
    assert res.converged and 0 <= min(res.iters) and max(res.iters) < 100
    assert dist <= bar
    assert res.trace_gt > 0 and res.trace_gen > 0 and 0 < res.trace_sqrt <= math.sqrt(res.trace_gt * res.trace_gen) * (1 + 1e-12)


def test_polar_trace_square_root_and_both_branches():
    from behavior_driven_video_synthesis_amd.fid_device import gemm_f64, polar_trace
    b = R.feature_set("d50_odd", 0).astype(np.float64)[:, :20]
    s = np.linalg.svd(b, compute_uv=False).sum()
    t, h, iters, ok = polar_trace(torch.from_numpy(b).cuda(), 1e-14, 100, True)
    assert ok and 0 < iters < 100 and abs(t - s) <= 1e-12 * s
    btb = b.T @ b
    assert torch.equal(h, h.t()) and np.abs(gemm_f64(h, h).cpu().numpy() - btb).max() <= 1e-11 * np.abs(btb).max()
    tw, hw, _, okw = polar_trace(torch.from_numpy(b.T.copy()).cuda(), 1e-14, 100, False)
    assert okw and hw is None and abs(tw - s) <= 1e-12 * s
    t0, h0, it0, ok0 = polar_trace(torch.zeros(7, 5, device="cuda", dtype=torch.float64), 1e-14, 100, True)
    assert t0 == 0.0 and ok0 and it0 == 0 and not h0.any()


# ---------------------------------------------------------------------------------------------------------------- 5. degenerate inputs
def test_degenerate_inputs(g21, bars):
    from behavior_driven_video_synthesis_amd.fid_device import fid_device
    from behavior_driven_video_synthesis_amd.lib.metrics import fid_from_features, fid_from_features_device
    x = torch.from_numpy(R.feature_set("d64", 0)).cuda()
    same = fid_device(x, x.clone())
    print(f"identical sets: fid {same.fid!r}, tr S1 + tr S2 = {same.trace_gt + same.trace_gen!r}")
    assert same.converged and abs(same.fid) <= bars["full"] * (same.trace_gt + same.trace_gen)
    # all rows equal: zero covariance
    const = x[:1].repeat(9, 1)
    res = fid_device(const, x)
    assert math.isfinite(res.fid) and res.fid > 0 and res.trace_gt <= 1e-24 * res.trace_gen
    # the cap: warns and returns the host route's value
    gt, gen = R.feature_set("d128_illcond", 0), R.feature_set("d128_illcond", 1)
    with pytest.warns(RuntimeWarning):
        capped = fid_device(torch.from_numpy(gt).cuda(), torch.from_numpy(gen).cuda(), max_iter=3)
    want = fid_from_features(gt, gen)
    assert not capped.converged and capped.iters == (3, 3) and abs(capped.fid - want) <= bars["full"] * abs(want)
    # a NaN feature: nan at once
    bad = x.clone()
    bad[3, 5] = float("nan")
    res = fid_device(bad, x)
    assert math.isnan(res.fid) and not res.converged and max(res.iters) <= 1
    res = fid_device(x, bad)
    assert math.isnan(res.fid) and max(res.iters) <= 1
    # two runs, and host arrays in place of device tensors
    y = torch.from_numpy(R.feature_set("d64", 1)).cuda()
    a, b = fid_device(x, y), fid_device(x, y)
    assert a == b and fid_from_features_device(x.cpu().numpy(), y.cpu().numpy()) == a.fid
    with pytest.raises(ValueError):
        fid_device(x[:1], y)
    with pytest.raises(ValueError):
        fid_device(x, y[:, :10])


# ---------------------------------------------------------------------------------------------------------------- 6. compute_fid
class _Seeded:
    """Hands every batch out behind torch.manual_seed(its index): the models draw latent noise from torch's generator."""

    def __init__(self, batches):
        self.batches = batches

    def __iter__(self):
        for i, b in enumerate(self.batches):
            torch.manual_seed(i)
            yield b


def _extractor():
    w = seeded_randn("fid.w", (3 * 4 * 4, 12), 5).cuda()
    return lambda x: torch.nn.functional.adaptive_avg_pool2d(x.float(), 4).flatten(1) @ w


def test_compute_fid_on_device_agrees_with_the_host_route(bars):
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import synthetic_batch
    from behavior_driven_video_synthesis_amd.lib import metrics
    from behavior_driven_video_synthesis_amd.models.vunets import VunetAlter
    net = VunetAlter(spatial_size=32, bottleneck_factor=2, box_factor=2, n_scales=0, n_latent_scales=2,
                     conv_layer_type="l1", nf_start=8, nf_max=16, subpixel_upsampling=True).cuda()
    batches = [synthetic_batch(8, 32, "cuda:0", seed=s) for s in range(6)]
    extractor = _extractor()
    net.train()
    want = metrics.compute_fid(net, _Seeded(batches), extractor)
    got = metrics.compute_fid(net, _Seeded(batches), extractor, on_device=True)
    assert net.training
    print(f"compute_fid: host {want!r} device {got!r} distance {abs(got - want) / abs(want):.3e}")
    assert abs(got - want) <= bars["full"] * abs(want)
    with torch.no_grad():
        gt = np.concatenate([extractor(b["pose_img"]).double().cpu().numpy() for b in batches])
    want_gt = metrics.compute_fid(net, _Seeded(batches), extractor, gt_features=gt)
    got_gt = metrics.compute_fid(net, _Seeded(batches), extractor, gt_features=gt, on_device=True)
    assert abs(got_gt - want_gt) <= bars["full"] * abs(want_gt)


# ---------------------------------------------------------------------------------------------------------------- 7. evaluate
def test_evaluate_returns_the_device_fid_and_the_checkpoint_is_named_by_it(tmp_path):
    from behavior_driven_video_synthesis_amd.experiments.checkpoint import save_metric_ckpt
    from behavior_driven_video_synthesis_amd.experiments.shape_and_pose_net import DEFAULT_CONFIG, ShapePoseNet, synthetic_batch
    from behavior_driven_video_synthesis_amd.lib import metrics
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["data"]["spatial_size"] = 32
    cfg["architecture"].update(nf_start=8, nf_max=16)
    trainer = ShapePoseNet(cfg, device="cuda:0", vgg_width_div=8, total_steps=50, vgg_synthetic=True)
    batches = [synthetic_batch(8, 32, "cuda:0", seed=60 + s) for s in range(3)]
    wc = seeded_randn("fid.cls", (3 * 4 * 4, 10), 5).cuda()

    def classifier(x):   # any callable mapping a 299 x 299 batch to logits
        return torch.nn.functional.adaptive_avg_pool2d(x.float(), 4).flatten(1) @ wc
    extractor = _extractor()
    plain = trainer.evaluate(_Seeded(batches), classifier)
    assert set(plain) == {"ssim", "is_recon", "std_is_recon", "is_transfer", "std_is_transfer", "n", "n_without_box"}
    got = trainer.evaluate(_Seeded(batches), classifier, fid_extractor=extractor)
    assert set(got) == set(plain) | {"fid"} and {k: v for k, v in got.items() if k != "fid"} == plain
    want = metrics.compute_fid(trainer.vunet, _Seeded(batches), extractor, on_device=True)
    assert got["fid"] == want and math.isfinite(want) and want > 0
    with torch.no_grad():
        gt = torch.cat([extractor(b["pose_img"]) for b in batches]).cpu().numpy() + 0.25
    got_gt = trainer.evaluate(_Seeded(batches), classifier, fid_extractor=extractor, gt_features=gt)
    assert got_gt["fid"] == metrics.compute_fid(trainer.vunet, _Seeded(batches), extractor, gt_features=gt, on_device=True) != want
    model_path, opt_path = save_metric_ckpt(str(tmp_path), trainer, 4, got["ssim"], got["is_recon"], fid=got["fid"])
    assert os.path.basename(model_path) == f"model@e4@ssim={got['ssim']}-fid={got['fid']}.pth"
    assert os.path.basename(opt_path) == f"opt@e4@ssim={got['ssim']}-fid={got['fid']}.pth"
    assert os.path.isfile(model_path) and os.path.isfile(opt_path)
    model_path, _ = save_metric_ckpt(str(tmp_path), trainer, 4, got["ssim"], got["is_recon"])
    assert os.path.basename(model_path) == f"model@e4@ssim={got['ssim']}-is={got['is_recon']}.pth"
