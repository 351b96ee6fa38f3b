#!/usr/bin/env python3
"""Generator of tests/golden/g21_fid.npz.  Runs ONLY where the upstream reference is checked out (VUNET_REFERENCE).

Per case of tests/fid_ref.py (seeded feature sets, rebuilt bit for bit by the tests) it records three float64 values of the FID:
``fid_ref``, the reference's own ``lib.metrics._calculate_fid`` on ``np.mean`` / ``np.cov``; ``fid_sym``, the symmetric-eigenvalue
restatement; ``fid_polar``, the polar iteration in numpy with its step counts.  The fixture holds these numbers only.

    python tests/golden/make_golden_fid.py
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
REF = os.environ.get("VUNET_REFERENCE", "/root/reference")

import fid_ref as R  # noqa: E402


def _install_stubs():
    """Absent third-party packages that the reference's lib/metrics.py imports at module import time only (the list of
    make_golden.py and of its g7_metrics)."""
    class _Any(types.ModuleType):
        def __getattr__(self, k):
            if k.startswith("__"):
                raise AttributeError(k)
            return type(k, (), {"__init__": lambda self, *a, **kw: None})

    for name in ["cv2", "kornia", "ignite", "ignite.engine", "ignite.handlers", "ignite.metrics", "ignite.contrib",
                 "ignite.contrib.handlers", "torch.utils.tensorboard", "torchvision", "torchvision.utils", "torchvision.models",
                 "torchvision.transforms", "wandb", "tqdm.autonotebook", "matplotlib.backends.backend_agg", "skimage",
                 "skimage.metrics", "h5py", "imagesize", "umap"]:
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                sys.modules[name] = _Any(name)


def main():
    _install_stubs()
    sys.path.insert(0, REF)
    from lib import metrics as rmet
    meta = {"seed": R.SEED, "cases": {}}
    for case in R.CASES:
        gt, gen = R.feature_set(case, 0), R.feature_set(case, 1)
        (mu1, s1), (mu2, s2) = R.moments(gt), R.moments(gen)
        ref = float(rmet._calculate_fid(mu1, s1, mu2, s2))
        assert np.isfinite(ref), (case, ref)
        polar, iters, ok = R.fid_polar(gt, gen, tol=1e-14, max_iter=100)
        assert ok and max(iters) < 100, (case, iters)
        meta["cases"][case] = {"shape": list(R.CASES[case]), "fid_ref": ref, "fid_sym": R.fid_sym(gt, gen), "fid_polar": polar,
                               "iters": list(iters)}
        print(case, meta["cases"][case])
    path = os.path.join(HERE, "g21_fid.npz")
    np.savez_compressed(path, __meta__=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8))
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
