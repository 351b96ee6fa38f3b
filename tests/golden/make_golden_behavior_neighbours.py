#!/usr/bin/env python3
"""Golden-vector generator for the nearest training-set neighbours of generated behaviour (g16).  Runs ONLY in the build
container (needs the reference checkout, as make_golden.py does, whose helpers it imports).

The reference's ``nearest_neighbours`` (lib/figures.py:23-455) cannot be imported as it stands: it builds the datasets and
needs cv2.  What it computes between loading the data and drawing is driven here on synthetic sequences with the reference's
own ``ResidualBehaviorNet`` (``behavior_state`` weights, stored as arrays), and its four numpy expressions are evaluated on those
arrays, written afresh:

* the bank's codes: ``mu`` of ``net.infer_b(poses_in, False)`` on ``poses_in = keypoints[:, :-1]`` (:85-101, ``prepare_input``);
* per query ``xs, _, _, b, mu, logstd, pre = net(poses_b, poses_in, len=seq_len)`` with the start pose put in front (:212, :235-240),
  the noise recorded (``FixedNoise``);
* code space (:258-262): ``np.argmin(np.linalg.norm(betas_train - mu, axis=1))`` in float32, as numpy does it;
* pose space (:146-164, :242-253, :268-277): both sides un-normalised (``x * std + mean`` with float64 statistics, every dimension
  used), ``mean_pelvis`` of the bank's first frames added and the pelvis subtracted, then
  ``np.argmin(np.sum(np.linalg.norm(xs_aligned - seqs_aligned, axis=-1), axis=(1, 2)))`` in float64.

Stored: the inputs, the reference's argmins and minima, and per query the relative gap between the best and the second best
distance (from the float64 restatement, tests/behavior_neighbours_ref.py).  Every gap must exceed twice the bound the kernels are
held to -- and in code space twice the float32 norm's own rounding bound (H / 2 + 2) 2^-24 -- so no query is ambiguous and the
reference's indices are the only right answer; asserted here.

    python tests/golden/make_golden_behavior_neighbours.py      # regenerate tests/golden/g16_behavior_neighbours.npz
"""
import os
import sys
import types

import numpy as np
import torch

import make_golden as G
from make_golden import FixedNoise, behavior_state, save, seeded_randn

sys.path.insert(0, os.path.dirname(G.HERE))
import behavior_neighbours_ref as R  # noqa: E402

SEED = 161
N_KPS, J, HID, N_BANK, T1, N_Q, ROOT = 51, 17, 64, 160, 7, 8, 0


def g16_behavior_neighbours():
    for name in ["h5py", "imagesize", "skimage", "skimage.metrics", "natsort", "kornia.geometry", "umap"]:
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                sys.modules[name] = types.ModuleType(name)
                sys.modules[name].__getattr__ = lambda k: type(k, (), {"__init__": lambda self, *a, **kw: None})
    from models import pose_behavior_rnn as rb
    torch.manual_seed(SEED)
    net_kw = dict(n_kps=N_KPS, information_bottleneck=True, decoder_arch="lstm", linear_in_decoder=False, dim_hidden_b=HID)
    net = rb.ResidualBehaviorNet(**net_kw)
    nsd = behavior_state(net, SEED)
    net.eval()
    net.b_enc.init_hidden = lambda bs, device: rb.BEncoder.init_hidden(net.b_enc, bs, "cpu")   # get_device() is -1 on CPU
    arrays = {f"net.sd.{k}": v.numpy() for k, v in nsd.items()}

    bank = 0.5 * seeded_randn("bank.kps", (N_BANK, T1, N_KPS), SEED)
    # half of the behaviour sequences are perturbed training sequences (a near neighbour exists), half are unrelated
    beh = 0.5 * seeded_randn("q.beh", (N_Q, T1, N_KPS), SEED)
    near = [3, 157, 64, 128]
    for a, j in enumerate(near):
        beh[a] = bank[j] + 0.05 * seeded_randn(f"q.near{a}", (T1, N_KPS), SEED)
    start = 0.5 * seeded_randn("q.start", (N_Q, T1, N_KPS), SEED)
    rng = np.random.RandomState(SEED)
    mean = rng.randn(N_KPS) * 250.0                       # float64 statistics: the un-normalisation is float64
    std = 40.0 + 40.0 * rng.rand(N_KPS)

    with torch.no_grad():
        betas_train = np.concatenate([net.infer_b(bank[s:s + 64, :-1], False)[1].numpy() for s in range(0, N_BANK, 64)], axis=0)
        poses_b, poses_in = beh[:, :-1], start[:, :-1]
        seq_len = poses_b.shape[1]
        with FixedNoise("q.enc", SEED) as fn:
            xs, _, _, b, mu, logstd, _ = net(poses_b, poses_in, len=seq_len)
        eps = seeded_randn("q.enc.eps0", (N_Q, HID), SEED)
        assert fn.shapes == [[N_Q, HID]] and torch.equal(b, eps * torch.exp(logstd) + mu)
        xs = torch.cat([poses_in[:, 0].unsqueeze(dim=1), xs], dim=1)
    assert betas_train.dtype == np.float32 and tuple(xs.shape) == (N_Q, T1, N_KPS)

    # ---- code space, lib/figures.py:258-262, one query at a time as the reference's loop
    mu_np = mu.numpy()
    code_norms = np.stack([np.linalg.norm(betas_train - mu_np[a], axis=1) for a in range(N_Q)])
    assert code_norms.dtype == np.float32
    code_arg, code_min = np.argmin(code_norms, axis=1), code_norms.min(axis=1)

    # ---- pose space, :121-164 and :242-277
    seqs_train = (bank.numpy() * std + mean).reshape(N_BANK, T1, J, 3)
    assert seqs_train.dtype == np.float64
    kp_id = ROOT
    mean_pelvis = np.expand_dims(np.expand_dims(np.mean(seqs_train[:, 0, kp_id], axis=0, keepdims=True), axis=1), axis=1)
    seqs_aligned = seqs_train + mean_pelvis - np.expand_dims(seqs_train[:, :, kp_id], axis=2)
    pose_sums = np.empty((N_Q, N_BANK))
    for a in range(N_Q):
        x = (xs[a].numpy() * std + mean).reshape(T1, J, 3)
        xs_aligned = np.expand_dims(x, axis=0) + mean_pelvis - np.expand_dims(np.expand_dims(x[:, kp_id], axis=1), axis=0)
        pose_sums[a] = np.sum(np.linalg.norm(xs_aligned - seqs_aligned, axis=-1), axis=(1, 2))
    pose_arg, pose_min = np.argmin(pose_sums, axis=1), pose_sums.min(axis=1)

    # ---- the float64 restatement: same winners, and no ambiguous query
    ci, cd, cgap = R.argmin_rows(R.code_distances(betas_train, mu_np))
    pi, pd, pgap = R.argmin_rows(R.pose_distances(bank.numpy(), xs.numpy(), mean, std, ROOT))
    f32_bound = (HID / 2 + 2) * 2.0 ** -24
    assert np.array_equal(ci, code_arg) and np.array_equal(pi, pose_arg)
    assert np.all(np.abs(cd - code_min) <= f32_bound * cd) and np.all(np.abs(pd - pose_min) <= 1e-12 * pd)
    assert np.all(cgap > 2 * max(R.bound(HID), f32_bound)), cgap
    assert np.all(pgap > 2 * R.bound(T1 * J + 3)), pgap
    assert list(code_arg[:len(near)]) == near, code_arg
    print(f"code space: argmin {code_arg.tolist()}, smallest gap {cgap.min():.3e}")
    print(f"pose space: argmin {pose_arg.tolist()}, smallest gap {pgap.min():.3e}")

    meta = {"seed": SEED, "net_kw": net_kw, "n_bank": N_BANK, "t1": T1, "n_q": N_Q, "j": J, "root": ROOT, "ignore": [], "near": near}
    arrays.update({"bank.kps": bank.numpy(), "bank.mu": betas_train, "q.beh": beh.numpy(), "q.start": start.numpy(), "q.eps": eps.numpy(),
                   "q.mu": mu_np, "q.logstd": logstd.numpy(), "q.b": b.numpy(), "q.xs": xs.numpy(), "stats.mean": mean, "stats.std": std,
                   "codes.argmin": code_arg.astype(np.int64), "codes.min": code_min, "codes.gap": cgap,
                   "poses.argmin": pose_arg.astype(np.int64), "poses.min": pose_min, "poses.gap": pgap})
    save("g16_behavior_neighbours", meta, arrays)


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(4)
    assert G.REF
    g16_behavior_neighbours()
