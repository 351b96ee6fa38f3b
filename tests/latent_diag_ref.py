"""Float64 restatement of the latent diagnostics (csrc/seq_latent.hip, latent_diag.py), free of scipy: the one-sample two-sided
Kolmogorov-Smirnov statistic against N(0, 1) with ``math.erfc``, the Kolmogorov series of the asymptotic p-value, and the
four ``FlowLoss`` entries and ``log_prob`` in float64 torch (lib/losses.py:295-311, :330-331)."""
import math

import numpy as np
import torch


GOLDEN_COLUMNS = ("normal", "scaled_shifted", "uniform", "half_tied", "all_equal", "one_inf")


def golden_columns(n, seed):
    """The fixture's six column types (tests/golden/make_golden_latent_diag.py) as fp32 [n, 6], rebuilt from the seed: N(0, 1);
    1.5 N(0, 1) + 0.3; uniform on [-1, 1); N(0, 1) with its first half set to one value; all equal; N(0, 1) with one +inf."""
    from synth import seeded_rand, seeded_randn
    cols = [seeded_randn(f"ks.{n}.c{j}", (n,), seed) for j in range(6)]
    cols[1] = 1.5 * cols[1] + 0.3
    cols[2] = seeded_rand(f"ks.{n}.c2", (n,), seed) * 2.0 - 1.0
    cols[3][:n // 2] = 0.25
    cols[4] = torch.full((n,), 0.5)
    cols[5][n // 3] = math.inf
    return torch.stack(cols, dim=1).numpy()


def ks_column(col):
    """-> (D, D+, D-) of one column of fp32 values (NaN: all NaN): sorted ascending, F_i = 0.5 erfc(-x_(i) / sqrt 2) on the value
    widened to float64, D+ = max_i (i / N - F_i), D- = max_i (F_i - (i - 1) / N), i = 1 .. N."""
    col = np.asarray(col, dtype=np.float32)
    if np.isnan(col).any():
        return (math.nan,) * 3
    x = np.sort(col).astype(np.float64)
    n = x.size
    dp = dm = -math.inf
    for i, v in enumerate(x.tolist()):
        f = 0.5 * math.erfc(-v / math.sqrt(2.0))
        dp = max(dp, (i + 1) / n - f)
        dm = max(dm, f - i / n)
    return max(dp, dm), dp, dm


def kolmogorov_sf(t):
    """2 sum_{k >= 1} (-1)^(k-1) exp(-2 k^2 t^2) until a term is below 1e-17, clamped to [0, 1]; for t < 0.2 the theta-function
    form 1 - sqrt(2 pi) / t sum_{k >= 1} exp(-(2k - 1)^2 pi^2 / (8 t^2))."""
    if t != t:
        return math.nan
    if not t > 0.0:
        return 1.0
    if t < 0.2:
        w, s = math.pi * math.pi / (8.0 * t * t), 0.0
        for k in range(1, 257):
            m = float(2 * k - 1)
            term = math.exp(-m * m * w)
            s += term
            if term < 1e-17:
                break
        p = 1.0 - math.sqrt(2.0 * math.pi) / t * s
    else:
        s, sign = 0.0, 1.0
        for k in range(1, 257):
            term = math.exp(-2.0 * float(k) * float(k) * t * t)
            s += sign * term
            sign = -sign
            if term < 1e-17:
                break
        p = 2.0 * s
    return min(max(p, 0.0), 1.0)


def ks_table(x):
    """x [N, C] -> dict of float64 [C] arrays: statistic, d_plus, d_minus, p_asymptotic."""
    x = np.asarray(x, dtype=np.float32)
    n = x.shape[0]
    rows = [ks_column(x[:, c]) for c in range(x.shape[1])]
    d = np.array([r[0] for r in rows])
    return {"statistic": d, "d_plus": np.array([r[1] for r in rows]), "d_minus": np.array([r[2] for r in rows]),
            "p_asymptotic": np.array([kolmogorov_sf(v * math.sqrt(n)) for v in d.tolist()])}


def reference_rule_takes_asymptotic(n, p_asym):
    """scipy 1.3.3 ``kstest(mode='approx')``: the asymptotic value when N > 2666 or p_asym > 0.80 - 0.0003 N."""
    return n > 2666 or p_asym > 0.80 - n * 0.3 / 1000.0


def flow_entries(gauss, logdet, noise=None):
    """-> (scalars [4] float64 numpy: flow_loss, reference_nll_loss, nlogdet_loss, nll_loss; nll [B]; log_prob [B])."""
    z = torch.as_tensor(gauss).double().reshape(len(gauss), -1)
    ld = torch.as_tensor(logdet).double()
    nll = 0.5 * (z * z).sum(1)
    nll_loss, nlogdet = nll.mean(), -ld.mean()
    ref = math.nan if noise is None else float((0.5 * (torch.as_tensor(noise).double().reshape(z.shape) ** 2).sum(1)).mean())
    log_prob = -nll + ld - 0.5 * z.shape[1] * math.log(2.0 * math.pi)
    return np.array([float(nll_loss + nlogdet), ref, float(nlogdet), float(nll_loss)]), nll.numpy(), log_prob.numpy()
