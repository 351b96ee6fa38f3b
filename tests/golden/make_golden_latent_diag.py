#!/usr/bin/env python3
"""Golden-vector generator for the latent diagnostics (g20).  Runs ONLY in the build container (needs the reference checkout,
as make_golden.py does, whose helpers it imports, and scipy).

* The reference's own ``lib.losses.FlowLoss()(gauss, logdet)`` (lib/losses.py:295-311) for B = 5 and B = 70 rows of C = 24: its
  log, and the ``torch.randn_like`` draw behind ``reference_nll_loss`` -- torch's generator is seeded before the call and the
  draw repeated from the same seed afterwards.
* ``scipy.stats.kstest(column, "norm")`` -- what lib/logging.py:2553 calls -- on six column types (tests/latent_diag_ref.py:
  ``golden_columns``) of N = 64, 65 and 1000 rows: statistic and p-value of the installed scipy, and ``kstwobign.sf(D sqrt N)``,
  the asymptotic value.  The rule of scipy 1.3.3's ``mode='approx'`` (the reference's pinned version) must take both of its
  branches on the standard-normal columns of what is written: asserted below.

    python tests/golden/make_golden_latent_diag.py      # regenerate tests/golden/g20_latent_diag.npz
"""
import os
import sys

import numpy as np
import torch

import make_golden as G
from make_golden import save, seeded_randn

sys.path.insert(0, os.path.dirname(G.HERE))
import latent_diag_ref as R  # noqa: E402

SEED = 213
C = 24
FLOW_ROWS = (5, 70)
KS_ROWS = (64, 65, 1000)


def g20_latent_diag():
    import scipy
    from scipy import stats
    arrays, meta = {}, {"seed": SEED, "C": C, "flow_rows": list(FLOW_ROWS), "ks_rows": list(KS_ROWS), "columns": list(R.GOLDEN_COLUMNS),
                        "scipy": scipy.__version__, "flow": {}}
    for b in FLOW_ROWS:
        gauss = (0.9 * seeded_randn(f"flow.{b}.gauss", (b, C, 1, 1), SEED) + 0.1)
        logdet = 3.0 * seeded_randn(f"flow.{b}.logdet", (b,), SEED) - 7.0
        torch.manual_seed(SEED + b)
        with torch.no_grad():
            loss, log = G.rl.FlowLoss()(gauss, logdet)
        torch.manual_seed(SEED + b)
        noise = torch.randn_like(gauss)
        assert abs(float(torch.mean(G.rl.nll(noise))) - log["reference_nll_loss"]) == 0.0      # the draw is the one it used
        assert float(loss) == log["flow_loss"]
        meta["flow"][str(b)] = log
        arrays[f"flow.{b}.noise"] = noise.reshape(b, C).numpy()
        print(b, log)
    branches = set()
    for n in KS_ROWS:
        x = R.golden_columns(n, SEED)
        res = [stats.kstest(x[:, j], "norm") for j in range(x.shape[1])]
        d = np.array([r[0] for r in res], dtype=np.float64)
        arrays[f"ks.{n}.statistic"] = d
        arrays[f"ks.{n}.pvalue"] = np.array([r[1] for r in res], dtype=np.float64)
        arrays[f"ks.{n}.p_asymptotic"] = stats.kstwobign.sf(d * np.sqrt(n))
        arrays[f"ks.{n}.two_ksone"] = np.minimum(2.0 * stats.ksone.sf(d, n), 1.0)
        take = R.reference_rule_takes_asymptotic(n, float(arrays[f"ks.{n}.p_asymptotic"][0]))
        branches.add(bool(take))
        print(n, "D", d, "p_asym", arrays[f"ks.{n}.p_asymptotic"], "asymptotic branch on the normal column:", take)
    assert branches == {True, False}, branches
    save("g20_latent_diag", meta, arrays)


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(4)
    assert G.REF
    g20_latent_diag()
