"""Float64 CPU restatement of the cVAE's adversarial pose regressor (experiments/behavior_net.py:627-648,
models/pose_behavior_rnn.py:47-62) with torch 1.3.1's Adam, which updates through ``p.data``: the adversarial term's
gradient wrt mu then runs through the weights after the fifth inner update with the fifth forward's ReLU masks.
Used by tests/test_regressor_golden.py (CPU) and tests/test_hip_seq_regressor.py (GPU)."""
import math

import torch

from synth import seeded_randn

KEYS = [f"fc{i}.{s}" for i in range(1, 6) for s in ("weight", "bias")]


def regressor_init(shapes, seed):
    """The fixture's starting weights (tests/golden/make_golden_regressor.py: ``regressor_state``)."""
    return {k: seeded_randn(f"reg.{k}", tuple(s), seed) * ((1.0 / s[1]) ** 0.5 if len(s) == 2 else 0.1) for k, s in shapes.items()}


def slice_of(v):
    """The part of a tensor the fixture stores (make_golden_regressor.py: ``slice_of``)."""
    return v.reshape(-1)[:512]


def forward(P, mu, idx):
    """Regressor_fly(mu, one_hot(idx)): fc4 of the one-hot written as the product it is."""
    relu = torch.relu
    h = relu(relu(relu(mu @ P["fc1.weight"].T + P["fc1.bias"]) @ P["fc2.weight"].T + P["fc2.bias"]) @ P["fc3.weight"].T + P["fc3.bias"])
    oh = torch.zeros(mu.shape[0], 50, dtype=mu.dtype)
    oh[:, idx] = 1.0
    c = relu(oh @ P["fc4.weight"].T + P["fc4.bias"])
    return torch.cat((h, c), dim=1) @ P["fc5.weight"].T + P["fc5.bias"]


def inner_steps(P0, mu, seq_b, idx, w, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, state=None):
    """The five inner steps from parameters ``P0`` on ``mu`` [B, H] and ``seq_b`` [B, T, n] (dtype of the inputs).
    -> (L_1..5, parameters after, Adam state, the adversarial gradient wrt mu (W^5), the same with W^4)."""
    P = {k: v.clone().requires_grad_(True) for k, v in P0.items()}
    st = state if state is not None else {k: dict(step=0, m=torch.zeros_like(v), v=torch.zeros_like(v)) for k, v in P0.items()}
    mu = mu.detach().clone().requires_grad_(True)
    ls, w4, loss = [], None, None
    for k in range(5):
        if k == 4:
            w4 = {n: p.detach().clone() for n, p in P.items()}
        loss = torch.mean((forward(P, mu, int(idx[k])) - seq_b[:, int(idx[k])]) ** 2)
        for p in P.values():
            p.grad = None
        loss.backward(retain_graph=True)
        b1, b2 = betas
        for n, p in P.items():   # torch 1.3.1 Adam.step: writes through p.data
            s, g = st[n], p.grad.data
            s["step"] += 1
            s["m"].mul_(b1).add_(g, alpha=1 - b1)
            s["v"].mul_(b2).addcmul_(g, g, value=1 - b2)
            denom = (s["v"].sqrt() / math.sqrt(1 - b2 ** s["step"])).add_(eps)
            p.data.addcdiv_(s["m"], denom, value=-lr / (1 - b1 ** s["step"]))
        ls.append(float(loss.detach()))

    def term(l):
        return -(torch.clamp(l, max=0.45) * w + torch.clamp(l, max=0.7) * w)
    adv, = torch.autograd.grad(term(loss), mu, retain_graph=True)
    l4 = torch.mean((forward(w4, mu, int(idx[4])) - seq_b[:, int(idx[4])]) ** 2)
    adv4, = torch.autograd.grad(term(l4), mu)
    return ls, {n: p.detach() for n, p in P.items()}, st, adv, adv4
