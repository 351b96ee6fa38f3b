"""Float64 CPU restatement of the behaviour model's sampling metrics (experiments/behavior_net.py:1238-1255, APD from
lib/logging.py:2079-2093) on normalised pose vectors, with the un-normalisation of data/data_conversions_3d.py:178-211 in the
statistics' precision.  Used by tests/test_behavior_eval_golden.py (CPU) and tests/test_hip_behavior_eval.py (GPU)."""
import numpy as np
import torch

from synth import seeded_randn


def unnormalise(x, mean, std, f32_math):
    """x [..., n] normalised (used dimensions) -> float64 values: x std + mean in float32 (two roundings, as numpy) or float64."""
    x = torch.as_tensor(np.asarray(x))
    mean, std = torch.as_tensor(np.asarray(mean)), torch.as_tensor(np.asarray(std))
    if f32_math:
        return (x.float() * std.float() + mean.float()).double()
    return x.float().double() * std.double() + mean.double()


def _diff(a, b, f32_math):
    return (a.float() - b.float()).double() if f32_math else a - b


def pair_tables(u, g, f32_math):
    """One sequence: u [S, T, D] un-normalised samples, g [T, D] un-normalised ground truth -> A, F, P [S, S] and G, GF [S]."""
    e = _diff(u[:, None], u[None, :], f32_math)                     # [q, s, T, D]
    sq = (e * e).sum(-1)
    d = sq.sqrt()
    eg = _diff(u, g[None], f32_math)
    dg = (eg * eg).sum(-1).sqrt()                                    # [S, T]
    return d.mean(-1), d[..., -1], sq.sum(-1).sqrt(), dg.mean(-1), dg[:, -1]


def second(rows):
    """np.sort(row)[1] of every row (NaN sorts last)."""
    return np.sort(np.asarray(rows), axis=-1)[..., 1]


def metrics(samples, future, mean, std, f32_math):
    """samples [N, S, T, n], future [N, T + 1, n] normalised; mean / std [n] of the used dimensions.  -> dict of float64 arrays:
    APD, ASD, FSD, minADE, minFDE [N] and the batch's ADE, FDE."""
    samples = torch.as_tensor(np.asarray(samples))
    future = torch.as_tensor(np.asarray(future))
    n_seq, s = samples.shape[0], samples.shape[1]
    if s < 2:
        raise ValueError("n_samples must be >= 2")
    out = {k: np.zeros(n_seq) for k in ("APD", "ASD", "FSD", "minADE", "minFDE")}
    for i in range(n_seq):
        u = unnormalise(samples[i], mean, std, f32_math)
        g = unnormalise(future[i, 1:], mean, std, f32_math)
        a, f, p, ga, gf = pair_tables(u, g, f32_math)
        out["ASD"][i] = second(a.numpy()).sum() / s
        out["FSD"][i] = second(f.numpy()).sum() / s
        out["APD"][i] = (p.sum(-1) / (s - 1)).sum().item() / s
        out["minADE"][i] = np.min(ga.numpy())                        # NaN propagates, as torch.min does
        out["minFDE"][i] = np.min(gf.numpy())
    out["ADE"], out["FDE"] = float(np.mean(out["minADE"])), float(np.mean(out["minFDE"]))
    return out


def fixture_inputs(meta, arr, tag):
    """The inputs of one g13 case: (samples [N, S, T, n] float32, future [N, T + 1, n] float32, mean, std of the used dims, f32)."""
    c = meta["cases"][tag]
    seed, bsz, skip, t = meta["seed"], meta["batch"], meta["skip"], c["seq_len"]
    n = arr[f"{tag}.samples"].shape[-1]
    future = (0.5 * seeded_randn(f"{tag}.future", (bsz, t + 1, n), seed))[::skip].contiguous()
    use = [d for d in range(meta["dims"]) if d not in set(c["ignore"])]
    mean, std = arr[f"{tag}.mean"], arr[f"{tag}.std"]
    return arr[f"{tag}.samples"], future.numpy(), mean[use], std[use], c["stats_dtype"] == "float32"
