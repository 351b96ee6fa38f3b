#!/usr/bin/env python3
"""Golden-vector generator for the behaviour model's sampling metrics (g13).  Runs ONLY in the build container (needs the
reference checkout, as make_golden.py does, whose helpers it imports).

``run_inference`` (experiments/behavior_net.py:1112-1301) driven the way it scores a test batch: the reference's own
``UnsupervisedTransformer2`` and ``ResidualBehaviorNet`` (``behavior_state`` weights, ``FixedNoise`` for every
``randn_like``) through the sampling loop of :1182-1217 -- S samples one after another, each a ``flow.reverse`` of fresh noise
and a roll-out on the rows [::skip], or ``net(..., sample=True)`` without a flow -- and the reference's own
``revert_output_format`` (data/data_conversions_3d.py:178-211, behind the stubs g9b_projection uses).  The metric formulas
are inline code in the reference and cannot be imported: ``metrics`` below restates them (:1238-1255; APD from
lib/logging.py:2079-2093) in the reference's precision.

    python tests/golden/make_golden_behavior_eval.py      # regenerate tests/golden/g13_behavior_eval.npz
"""
import sys
import types

import numpy as np
import torch

import make_golden as G
from make_golden import FixedNoise, behavior_state, save, seeded_randn

SEED = 131
N_KPS, HID, BSZ, SKIP = 51, 64, 17, 4
FLOW_KW = dict(flow_in_channels=HID, flow_mid_channels=128, flow_hidden_depth=2, n_flows=3)
DIMS, N_IGNORE = 96, 45
# tag: (with the flow, statistics dtype, samples, seq_len, (q, s): sample s draws the noise of sample q -- two identical samples)
CASES = {"flow_f64_s8": (True, "float64", 8, 6, None), "flow_f32_s50": (True, "float32", 50, 6, None),
         "prior_f64_s50": (False, "float64", 50, 6, None), "prior_f32_s8": (False, "float32", 8, 9, None),
         "tie_f64_s8": (True, "float64", 8, 7, (2, 5))}
TRANSFER_CASE = "flow_f64_s8"
REVERTED = ("flow_f64_s8", "prior_f32_s8")     # the cases whose reverted arrays are stored as well (one per statistics dtype)


def stats(stats_dtype):
    """g9b_projection's recipe of the H3.6M-like statistics: 96 dimensions, 45 of them ignored."""
    rng = np.random.RandomState(17 + DIMS)
    ignore = sorted(rng.choice(DIMS, size=N_IGNORE, replace=False).tolist())
    mean = (rng.randn(DIMS) * 300.0).astype(stats_dtype)
    std = (50.0 + 200.0 * rng.rand(DIMS)).astype(stats_dtype)
    return mean, std, ignore


def metrics(seq_samples, seq_gt, n_samples, seq_len):
    """The reference's formulas, in its precision (the reverted arrays' dtype).  seq_samples [N, S, T, D]; seq_gt [N, 1, T, D]
    (already without frame 0, :1235).  Per sequence: for each sample q the row of distances to every sample s --
    mean over frames of the per-frame norm (:1241), the final frame's norm (:1243), the whole sequence's norm (APD,
    lib/logging.py:2083) -- then element [1] of np.sort of the first two rows (:1242, :1244) and the row sum over (S - 1) of
    the third, each accumulated over q and divided by S (:1246-1247, lib/logging.py:2091).  Per batch: the mean over sequences
    of the minimum over samples of the mean-over-frames / final-frame error against the ground truth (:1250-1254)."""
    apd, asd, fsd = [], [], []
    for samples in seq_samples:
        acc_a = acc_s = acc_f = 0
        for x_q in samples:
            diff = x_q - samples
            acc_a += torch.sum(torch.norm(diff.reshape(n_samples, -1), dim=1)) / (n_samples - 1)
            acc_s += np.sort(torch.mean(torch.norm(diff.reshape(n_samples, seq_len, -1), dim=2), dim=1).numpy())[1]
            acc_f += np.sort(torch.norm(diff[:, -1].reshape(n_samples, -1), dim=1).numpy())[1]
        apd.append(acc_a.item() / n_samples)
        asd.append(acc_s.item() / n_samples)
        fsd.append(acc_f.item() / n_samples)
    n_seq = seq_gt.shape[0]
    err = torch.norm((seq_samples - seq_gt).reshape(n_seq, n_samples, seq_len, -1), dim=3)
    min_ade = torch.min(torch.mean(err, dim=2), dim=1)[0]
    min_fde = torch.min(torch.norm((seq_samples[:, :, -1] - seq_gt[:, :, -1]).reshape(n_seq, n_samples, -1), dim=2), dim=1)[0]
    return dict(APD=np.array(apd), ASD=np.array(asd), FSD=np.array(fsd), minADE=min_ade.double().numpy(),
                minFDE=min_fde.double().numpy(), ADE=float(torch.mean(min_ade)), FDE=float(torch.mean(min_fde)))


class TieNoise(FixedNoise):
    """FixedNoise whose call ``s`` returns what call ``q`` returned: samples q and s of every sequence are identical."""

    def __init__(self, tag, seed, tie):
        super().__init__(tag, seed)
        self.tie = tie

    def __enter__(self):
        super().__enter__()
        fake = torch.randn_like

        def tied(t, **kw):
            if self.tie is not None and self.i == self.tie[1]:
                e = seeded_randn(f"{self.tag}.eps{self.tie[0]}", tuple(t.shape), self.seed)
                self.shapes.append(list(t.shape))
                self.i += 1
                return e
            return fake(t, **kw)
        torch.randn_like = tied
        return self


def g13_behavior_eval():
    for name in ["h5py", "imagesize", "skimage", "skimage.metrics", "natsort", "kornia.geometry", "umap"]:
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                sys.modules[name] = types.ModuleType(name)
                sys.modules[name].__getattr__ = lambda k: type(k, (), {"__init__": lambda self, *a, **kw: None})
    from data import data_conversions_3d as dc
    from models import pose_behavior_rnn as rb
    from models.flow import simple_flow as rf
    torch.manual_seed(SEED)
    flow = rf.UnsupervisedTransformer2(**FLOW_KW)
    fsd = behavior_state(flow, SEED)
    flow.eval()
    net_kw = dict(n_kps=N_KPS, information_bottleneck=True, decoder_arch="lstm", linear_in_decoder=False, dim_hidden_b=HID)
    net = rb.ResidualBehaviorNet(**net_kw)
    nsd = behavior_state(net, SEED)
    net.eval()
    net.b_enc.init_hidden = lambda bs, device: rb.BEncoder.init_hidden(net.b_enc, bs, "cpu")   # get_device() is -1 on CPU
    arrays, meta = {}, {"seed": SEED, "batch": BSZ, "skip": SKIP, "flow_kw": FLOW_KW, "net_kw": net_kw, "dims": DIMS,
                        "n_ignore": N_IGNORE, "flow_shapes": {k: list(v.shape) for k, v in fsd.items()},
                        "net_shapes": {k: list(v.shape) for k, v in nsd.items()}, "cases": {}}
    for k, v in fsd.items():
        if k.endswith("_shuffle_idx"):
            arrays[f"flow.sd.{k}"] = v.numpy()
    for tag, (use_flow, sdt, n_samples, seq_len, tie) in CASES.items():
        mean, std, ignore = stats(sdt)
        # keypoints -> prepare_input (lib/utils.py:914-917); the future sequences stand in for _get_keypoints (:1162-1179)
        kps = 0.5 * seeded_randn(f"{tag}.kps", (BSZ, seq_len + 1, N_KPS), SEED)
        future = 0.5 * seeded_randn(f"{tag}.future", (BSZ, seq_len + 1, N_KPS), SEED)
        x_s, target_s = kps[:, :-1], kps[:, 1:]
        future_seqs = future[::SKIP]
        b = torch.zeros(BSZ, HID)                                                          # (only its shape is used: randn_like(b[::skip]))
        seq_samples, normalised = [], []
        with torch.no_grad(), TieNoise(f"{tag}.z", SEED, tie) as fn:
            for _ in range(n_samples):                                                     # :1182-1217
                if use_flow:
                    b_fs1 = flow.reverse(torch.randn_like(b[::SKIP])).squeeze(dim=-1).squeeze(dim=-1)
                    seq_s, *_ = net.generate_seq(b_fs1, target_s[::SKIP], len=seq_len, start_frame=target_s.shape[1] - 1)
                else:
                    seq_s, *_ = net(x_s[::SKIP, :seq_len], target_s[::SKIP], seq_len, sample=True, start_frame=target_s.shape[1] - 1)
                normalised.append(seq_s)
                seq_samples.append(torch.stack([torch.tensor(dc.revert_output_format(s.cpu().numpy(), mean, std, ignore))
                                                for s in seq_s], dim=0))
        seq_samples = torch.stack(seq_samples, dim=1)
        seq_gt = torch.stack([torch.tensor(dc.revert_output_format(s.cpu().numpy(), mean, std, ignore)) for s in future_seqs],
                             dim=0).unsqueeze(1)[:, :, 1:]
        m = metrics(seq_samples, seq_gt, n_samples, seq_len)
        use = [d for d in range(DIMS) if d not in set(ignore)]
        meta["cases"][tag] = {"flow": use_flow, "stats_dtype": sdt, "n_samples": n_samples, "seq_len": seq_len, "tie": tie,
                              "ignore": ignore, "noise_shapes": fn.shapes, "sample_dtype": str(seq_samples.dtype),
                              "ADE": m["ADE"], "FDE": m["FDE"]}
        arrays[f"{tag}.mean"], arrays[f"{tag}.std"] = mean, std
        arrays[f"{tag}.samples"] = torch.stack(normalised, dim=1).numpy()                 # [N, S, T, n] as the net returned them
        if tag in REVERTED:
            arrays[f"{tag}.reverted"] = seq_samples[..., use].numpy()                     # the used dimensions
            arrays[f"{tag}.reverted_gt"] = seq_gt[:, 0][..., use].numpy()
            assert torch.equal(seq_samples[..., ignore], torch.from_numpy(mean[ignore]).expand_as(seq_samples[..., ignore]))
        for k in ("APD", "ASD", "FSD", "minADE", "minFDE"):
            arrays[f"{tag}.{k}"] = m[k]
        print(tag, {k: (round(float(np.mean(v)), 3) if isinstance(v, np.ndarray) else round(v, 3)) for k, v in m.items()})
        if tag == TRANSFER_CASE:                                                           # :1262-1278
            kps2 = 0.5 * seeded_randn(f"{tag}.paired", (BSZ, seq_len + 1, N_KPS), SEED)
            kps3 = 0.5 * seeded_randn(f"{tag}.matched", (BSZ, seq_len + 1, N_KPS), SEED)
            x_t, x_related = kps2[:, :-1], kps3[:, :-1]
            with torch.no_grad(), FixedNoise(f"{tag}.xfer", SEED):
                seq_cross, _, _, _, mu, *_ = net(x_s, x_t, seq_len, sample=False)
                _, _, _, _, mu2, *_ = net(seq_cross, x_t, seq_len, sample=False)
                _, _, _, _, mu3, *_ = net(x_related, x_t, seq_len, sample=False)
            r, d = torch.norm(mu - mu2, dim=1), torch.norm(mu - mu3, dim=1)
            meta["transfer"] = {"case": tag, "ADE_c": float(torch.mean(torch.norm(seq_cross - x_s, dim=2))),
                                "FDE_c": float(torch.mean(torch.norm(seq_cross[:, -1] - x_s[:, -1], dim=1))),
                                "recon_mu": float(torch.mean(r)), "recon_std": float(torch.std(r)),
                                "distance_mu": float(torch.mean(d)), "distance_std": float(torch.std(d))}
            print("transfer", meta["transfer"])
    save("g13_behavior_eval", meta, arrays)


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(4)
    assert G.REF
    g13_behavior_eval()
