"""CPU restatement of the image experiments' post-hoc pose-regressor probe, in plain torch without autograd: forward, loss,
backward and Adam of one step, in float32 or float64.  The oracle of tests/test_reg_probe_golden.py (against the reference's own
``Regressor`` + ``torch.optim.Adam``: tests/golden/g17_reg_probe.npz) and of tests/test_hip_reg_probe.py (against the kernels).

Inputs and initial weights come from ``synth`` by name, so fixtures store results only.
"""
from __future__ import annotations

import math
import os
import sys
from typing import Dict, List, Sequence

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from synth import seeded_randn, synth_state_dict  # noqa: E402

SEED = 17
STEPS = 6
CASES = {
    # linears 32 -> 32 -> 34, embedder K = 16 * 4 * 4 = 256 and 16 * 2 * 2 = 64
    "small": dict(n_out=34, n_latent_scales=2, nf_max=16, latent_widths=(4, 2), linear_width_factor=1, n_linear=2, B=5),
    "one_scale": dict(n_out=34, n_latent_scales=1, nf_max=16, latent_widths=(4,), linear_width_factor=1, n_linear=2, B=2),
}
SHIPPED = dict(n_out=34, n_latent_scales=2, nf_max=128, latent_widths=(8, 4), linear_width_factor=1, n_linear=2, B=8)


def model_kwargs(cfg: dict) -> dict:
    return {k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items() if k != "B"}


def shapes(cfg: dict) -> Dict[str, List[int]]:
    """State-dict keys, order and shapes of ``Regressor.__init__`` (models/vunets.py:788-807)."""
    n_out, n_st, nf, f, n_lin = cfg["n_out"], cfg["n_latent_scales"], cfg["nf_max"], cfg["linear_width_factor"], cfg["n_linear"]
    lw = n_st * nf * f                                                              # :793
    out: Dict[str, List[int]] = {}
    for i in range(n_st):                                                           # :798-799
        k = cfg["latent_widths"][i]
        out[f"embedders.{i}.weight"], out[f"embedders.{i}.bias"] = [f * nf, nf, k, k], [f * nf]
    for i in range(n_lin):                                                          # :801-807
        arg_in = 2 if lw // 2 ** (n_lin - i) > n_out else 1
        arg_out = 2 if lw // 2 ** (n_lin - i - 1) > n_out else 1
        fan_out = n_out if i == n_lin - 1 else lw // arg_out ** (i + 1)
        out[f"linears.{i}.weight"], out[f"linears.{i}.bias"] = [fan_out, lw // arg_in ** i], [fan_out]
    return out


def init_state(cfg: dict, seed: int = SEED) -> Dict[str, torch.Tensor]:
    return synth_state_dict(shapes(cfg), seed)


def inputs(tag: str, cfg: dict, steps: int = STEPS, seed: int = SEED):
    """-> per step (means, targets): ``means`` in the order the VUnet's bottleneck returns them (coarsest first -- the regressor
    reads them reversed, models/vunets.py:813), targets [B, n_out]."""
    B, nf = cfg["B"], cfg["nf_max"]
    widths = list(reversed(cfg["latent_widths"]))
    out = []
    for t in range(steps):
        means = [seeded_randn(f"{tag}.means.{s}.{t}", (B, nf, w, w), seed) for s, w in enumerate(widths)]
        out.append((means, seeded_randn(f"{tag}.tgt.{t}", (B, cfg["n_out"]), seed)))
    return out


def forward(sd: Dict[str, torch.Tensor], cfg: dict, means: Sequence[torch.Tensor]):
    """``Regressor.forward`` (models/vunets.py:811-824): a full-window valid convolution is the product of the flattened latent
    with ``weight.reshape(out, -1)``.  -> (pred, saved activations)."""
    xs, feats = [], []
    for i, e in enumerate(reversed(list(means))):                                   # :813
        x = e.reshape(e.shape[0], -1)
        w = sd[f"embedders.{i}.weight"]
        feats.append(torch.relu(x @ w.reshape(w.shape[0], -1).t() + sd[f"embedders.{i}.bias"]))   # :814
        xs.append(x)
    h = torch.cat(feats, dim=-1)                                                    # :816
    acts = [h]
    for i in range(cfg["n_linear"]):                                                # :818-822
        h = h @ sd[f"linears.{i}.weight"].t() + sd[f"linears.{i}.bias"]
        if i < cfg["n_linear"] - 1:
            h = torch.relu(h)
        acts.append(h)
    return h, (xs, acts)


def loss_and_dpred(pred: torch.Tensor, tgt: torch.Tensor):
    """``torch.mean(torch.norm(preds - reg_targets, dim=1))`` (experiments/shape_and_pose_net.py:972-974) and its gradient;
    a row of norm 0 gets gradient 0, as torch's norm backward gives."""
    r = pred - tgt
    nrm = r.square().sum(dim=1).sqrt()
    scale = torch.where(nrm > 0, (1.0 / r.shape[0]) / nrm, torch.zeros_like(nrm))
    return nrm.mean(), r * scale[:, None]


def grads(sd: Dict[str, torch.Tensor], cfg: dict, means, tgt):
    """What ``loss_regressor.backward()`` (experiments/shape_and_pose_net.py:976) leaves in ``.grad``.  -> (loss, pred, grads)."""
    pred, (xs, acts) = forward(sd, cfg, means)
    loss, dz = loss_and_dpred(pred, tgt)
    g: Dict[str, torch.Tensor] = {}
    for i in range(cfg["n_linear"] - 1, -1, -1):
        g[f"linears.{i}.weight"], g[f"linears.{i}.bias"] = dz.t() @ acts[i], dz.sum(dim=0)
        dz = (dz @ sd[f"linears.{i}.weight"]) * (acts[i] > 0).to(dz.dtype)         # ReLU' read off the saved output
    off = 0
    for i, x in enumerate(xs):
        w = sd[f"embedders.{i}.weight"]
        d = dz[:, off:off + w.shape[0]]
        g[f"embedders.{i}.weight"], g[f"embedders.{i}.bias"] = (d.t() @ x).reshape(w.shape), d.sum(dim=0)
        off += w.shape[0]
    return loss, pred, g


def adam_step(sd, g, state, t: int, lr: float = 1e-3, b1: float = 0.9, b2: float = 0.999, eps: float = 1e-8):
    """torch.optim.Adam (experiments/shape_and_pose_net.py:930: ``Adam(regressor.parameters(), lr=0.001)``), torch/optim/adam.py
    ``_single_tensor_adam``: bias corrections as host doubles."""
    step_size = lr / (1.0 - b1 ** t)
    bc2_sqrt = math.sqrt(1.0 - b2 ** t)
    for k, p in sd.items():
        m, v = state.setdefault(k, (torch.zeros_like(p), torch.zeros_like(p)))
        m.mul_(b1).add_(g[k], alpha=1.0 - b1)
        v.mul_(b2).addcmul_(g[k], g[k], value=1.0 - b2)
        p.addcdiv_(m, (v.sqrt() / bc2_sqrt).add_(eps), value=-step_size)


def run(cfg: dict, sd: Dict[str, torch.Tensor], batches, dtype=torch.float32, lr: float = 1e-3, state=None, t0: int = 0):
    """Drive ``len(batches)`` steps.  -> (losses, pred of the first step, final state dict, Adam state)."""
    sd = {k: v.detach().clone().to(dtype) for k, v in sd.items()}
    state = {} if state is None else {k: (m.clone().to(dtype), v.clone().to(dtype)) for k, (m, v) in state.items()}
    losses, pred1 = [], None
    for t, (means, tgt) in enumerate(batches, start=1):
        loss, pred, g = grads(sd, cfg, [m.to(dtype) for m in means], tgt.to(dtype))
        if pred1 is None:
            pred1 = pred.clone()
        adam_step(sd, g, state, t0 + t, lr)
        losses.append(loss)
    return torch.stack(losses), pred1, sd, state
