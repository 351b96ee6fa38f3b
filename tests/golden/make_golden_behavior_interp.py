#!/usr/bin/env python3
"""Golden-vector generator for behaviour transfer and latent interpolation (g15).  Runs ONLY in the build container (needs the
reference checkout, as make_golden.py does, whose helpers it imports).

The two per-epoch video hooks of experiments/behavior_net.py:851-890 up to their pose arrays, driven as the reference drives
them, on the reference's own ``ResidualBehaviorNet`` (``behavior_state`` weights, stored as arrays) and its own ``slerp``
(lib/utils.py:920-925):

* ``latent_interpolate`` (lib/logging.py:983-1022): the codes of both sequences of a pair, ``slerp`` between them at
  ``np.linspace(0, 1, 6)`` in both directions, and one batch-1 ``generate_seq(code, data, T, start_frame=0)`` per step and
  direction.  The codes are the posterior means (``mu`` of ``infer_b(., False)``): the reference interpolates the first return
  value, which carries a fresh noise draw per call; the mean is what is reproducible.  ``infer_b``'s ``b`` and ``logstd`` are
  stored with the noise that produced them (``FixedNoise``).
* ``visualize_transfer3d`` (lib/logging.py:207-212, :331-342): ``generate_seq(mu2, data1, ...)`` and
  ``generate_seq(mu1, data2, ...)`` at ``start_frame`` 0 and 3, and the same from the sampled code ``b``.

``slerp`` returns float64 under this container's numpy (a float64 scalar times a float32 array); ``torch.tensor`` of it would
hand the float32 LSTM a float64 code, so it is rounded to float32 first, which is also what older numpy returned.

Bare cases, codes only: H in {1, 3, 64, 130, 1024}, three pairs each -- independent Gaussian, near-parallel
(b2 = b1 + 1e-3 noise), identical.  No antiparallel pairs: there sin(omega) of the float32 path is a rounding residue of pi
and the reference's own output is noise (the two coefficients are ~1e7 with opposite signs), so nothing can be held to it.
For H = 1 two rows are either parallel or antiparallel, so the Gaussian pair's second row takes the first one's sign.
Per case: the reference's float32-path result, a float64 evaluation of the same formula from the same float32 inputs
(tests/behavior_interp_ref.py's arithmetic, checked here against the reference's function on float64 copies of the inputs),
and ``f64_gap``: the largest distance between the two columns relative to max|b|.

    python tests/golden/make_golden_behavior_interp.py      # regenerate tests/golden/g15_behavior_interp.npz
"""
import os
import sys
import types

import numpy as np
import torch

import make_golden as G
from make_golden import FixedNoise, behavior_state, save, seeded_randn

sys.path.insert(0, os.path.dirname(G.HERE))
import behavior_interp_ref as R  # noqa: E402

SEED = 151
N_KPS, HID, PAIRS, T = 51, 64, 2, 6
STEPS = np.linspace(0, 1, 6)
BARE_H = (1, 3, 64, 130, 1024)
BARE_KINDS = ("gauss", "near", "same")
START_FRAMES = (0, 3)


def bare_pairs(h):
    b1 = seeded_randn(f"bare{h}.b1", (3, h), SEED).numpy()
    b2 = seeded_randn(f"bare{h}.b2", (3, h), SEED).numpy()
    if h == 1:
        b2[0] = np.abs(b2[0]) * np.sign(b1[0])
    b2[1] = b1[1] + np.float32(1e-3) * b2[1]
    b2[2] = b1[2]
    cos = float(np.dot(b1[0].astype(np.float64), b2[0].astype(np.float64)) / (np.linalg.norm(b1[0].astype(np.float64))
                                                                               * np.linalg.norm(b2[0].astype(np.float64))))
    assert cos > -0.9, (h, cos)
    return b1, b2


def ref_slerp_codes(slerp, b1, b2):
    """The reference's function, row by row as lib/logging.py:997-1012 calls it -> float32 [2, P, S, H]."""
    out = np.empty((2, b1.shape[0], len(STEPS), b1.shape[1]), dtype=np.float32)
    for d, (lo, hi) in enumerate(((b1, b2), (b2, b1))):
        for p in range(b1.shape[0]):
            for s, v in enumerate(STEPS):
                out[d, p, s] = np.asarray(slerp(v, lo[p], hi[p])).astype(np.float32)
    return out


def g15_behavior_interp():
    for name in ["h5py", "imagesize", "skimage", "skimage.metrics", "natsort", "kornia.geometry", "umap"]:
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                sys.modules[name] = types.ModuleType(name)
                sys.modules[name].__getattr__ = lambda k: type(k, (), {"__init__": lambda self, *a, **kw: None})
    from lib import utils as ru
    from models import pose_behavior_rnn as rb
    torch.manual_seed(SEED)
    net_kw = dict(n_kps=N_KPS, information_bottleneck=True, decoder_arch="lstm", linear_in_decoder=False, dim_hidden_b=HID)
    net = rb.ResidualBehaviorNet(**net_kw)
    nsd = behavior_state(net, SEED)
    net.eval()
    net.b_enc.init_hidden = lambda bs, device: rb.BEncoder.init_hidden(net.b_enc, bs, "cpu")   # get_device() is -1 on CPU
    arrays = {f"net.sd.{k}": v.numpy() for k, v in nsd.items()}
    meta = {"seed": SEED, "net_kw": net_kw, "pairs": PAIRS, "t": T, "steps": STEPS.tolist(), "start_frames": list(START_FRAMES),
            "bare_h": list(BARE_H), "bare_kinds": list(BARE_KINDS), "f64_gap": {}}
    # (keypoints -> prepare_input, lib/utils.py:914-917: data = kps[:, :-1])
    data1 = 0.5 * seeded_randn("pair.data1", (PAIRS, T, N_KPS), SEED)
    data2 = 0.5 * seeded_randn("pair.data2", (PAIRS, T, N_KPS), SEED)
    with torch.no_grad():
        with FixedNoise("pair.enc", SEED) as fn:
            b1, mu1, logstd1, _ = net.infer_b(data1, False)
            b2, mu2, logstd2, _ = net.infer_b(data2, False)
        eps1, eps2 = seeded_randn("pair.enc.eps0", (PAIRS, HID), SEED), seeded_randn("pair.enc.eps1", (PAIRS, HID), SEED)
        assert fn.shapes == [[PAIRS, HID]] * 2 and torch.equal(b1, eps1 * torch.exp(logstd1) + mu1)
        codes = ref_slerp_codes(ru.slerp, mu1.numpy(), mu2.numpy())
        rolls = np.empty((2, PAIRS, len(STEPS), T, N_KPS), dtype=np.float32)
        for d, data in enumerate((data1, data2)):
            for p in range(PAIRS):
                for s in range(len(STEPS)):          # one batch-1 roll-out per step, as :1017-1022
                    xs, *_ = net.generate_seq(torch.tensor(codes[d, p, s]).unsqueeze(dim=0), data[p:p + 1], T, start_frame=0)
                    rolls[d, p, s] = xs[0].numpy()
        for sf in START_FRAMES:
            arrays[f"xfer.x1_mu2.s{sf}"] = net.generate_seq(mu2, data1, len=T, start_frame=sf)[0].numpy()
            arrays[f"xfer.x2_mu1.s{sf}"] = net.generate_seq(mu1, data2, len=T, start_frame=sf)[0].numpy()
        arrays["xfer.x1_b2.s0"] = net.generate_seq(b2, data1, len=T, start_frame=0)[0].numpy()
    for name, v in dict(data1=data1, data2=data2, b1=b1, b2=b2, mu1=mu1, mu2=mu2, logstd1=logstd1, logstd2=logstd2, eps1=eps1,
                        eps2=eps2).items():
        arrays[f"pair.{name}"] = v.numpy()
    arrays["pair.slerp"], arrays["pair.rollouts"] = codes, rolls
    for h in BARE_H:
        b1, b2 = bare_pairs(h)
        ref = ref_slerp_codes(ru.slerp, b1, b2)
        f64, _ = R.slerp_codes(b1, b2, STEPS)
        scale = max(float(np.abs(b1).max()), float(np.abs(b2).max()))
        # the restated float64 arithmetic against the reference's own function on float64 copies of the inputs
        own = np.stack([np.stack([np.stack([ru.slerp(v, lo[p].astype(np.float64), hi[p].astype(np.float64)) for v in STEPS])
                                  for p in range(3)]) for lo, hi in ((b1, b2), (b2, b1))])
        assert float(np.abs(own - f64).max()) <= 1e-12 * scale, (h, float(np.abs(own - f64).max()))
        gap = float(np.abs(ref.astype(np.float64) - f64).max() / scale)
        meta["f64_gap"][str(h)] = gap
        arrays[f"bare{h}.b1"], arrays[f"bare{h}.b2"], arrays[f"bare{h}.ref"], arrays[f"bare{h}.f64"] = b1, b2, ref, f64
        print(f"H = {h}: f64_gap {gap:.3e} of max|b| = {scale:.3f}")
    save("g15_behavior_interp", meta, arrays)


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(4)
    assert G.REF
    g15_behavior_interp()
