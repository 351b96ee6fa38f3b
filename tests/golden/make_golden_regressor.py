#!/usr/bin/env python3
"""Golden-vector generator for the cVAE's adversarial pose regressor (g12).  Runs ONLY in the build container (needs the
reference checkout, as make_golden.py does, whose helpers it imports).

BASELINE config 4, first stage with ``use_regressor`` (experiments/behavior_net.py:591-660, models/pose_behavior_rnn.py:47-62):
the reference's own ``ResidualBehaviorNet``, ``Regressor_fly`` and ``kl_loss`` driven for three steps as ``train_fn`` drives
them -- the cVAE loss, five inner regressor steps (``Adam(lr=1e-4)``), ``loss -= w clamp(L_5, max=0.45) + w clamp(L_5,
max=0.7)``, the net's backward / ``torch.optim.Adam`` step / gamma update.  The regressor's Adam is torch 1.3.1's (the
reference's pinned torch), which writes through ``p.data``: the adversarial term's backward then runs through the weights
after the fifth inner update with the fifth forward's ReLU masks.  Torch >= 1.5's own Adam bumps the version counter and
refuses that backward; a ``.data`` write does not, so the pinned semantics are reproduced here exactly.

    python tests/golden/make_golden_regressor.py      # regenerate tests/golden/g12_cvae_regressor.npz
"""
import math

import torch

import make_golden as G
from make_golden import FixedNoise, behavior_state, save, seeded_randn
from lib import losses as rl  # noqa: E402  (the reference's, on make_golden's path)

SEED = 121
N_KPS, HID, BSZ, T_LEN, STEPS = 51, 256, 5, 50, 3
W_RECON, GAMMA, GAMMA_STEP, IMAX, LR, REG_LR = 2.5, 0.05, 1e-3, 5.0, 1e-3, 1e-4
KPS_SCALE = (0.62, 0.8, 0.74)    # per step: L_5 below 0.45 in some steps, between 0.45 and 0.7 in others
CASES = {"shipped": dict(w=0.01, cvae=False), "w1": dict(w=1.0, cvae=False), "cvae": dict(w=0.01, cvae=True)}


class Adam131:
    """torch 1.3.1's ``torch.optim.Adam.step`` (amsgrad False, no weight decay): the update goes through ``p.data``."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8):
        self.params, self.lr, self.betas, self.eps = list(params), lr, betas, eps
        self.state = [dict(step=0, exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p)) for p in self.params]

    def zero_grad(self):
        for p in self.params:
            if p.grad is not None:
                p.grad.detach_()
                p.grad.zero_()

    def step(self):
        b1, b2 = self.betas
        for p, st in zip(self.params, self.state):
            g = p.grad.data
            st["step"] += 1
            st["exp_avg"].mul_(b1).add_(g, alpha=1 - b1)
            st["exp_avg_sq"].mul_(b2).addcmul_(g, g, value=1 - b2)
            denom = (st["exp_avg_sq"].sqrt() / math.sqrt(1 - b2 ** st["step"])).add_(self.eps)
            p.data.addcdiv_(st["exp_avg"], denom, value=-self.lr / (1 - b1 ** st["step"]))


def regressor_state(shapes, seed):
    """The regressor's starting weights: fan-in scaled normals, small biases (the tests rebuild them from this recipe)."""
    return {k: seeded_randn(f"reg.{k}", tuple(s), seed) * ((1.0 / s[1]) ** 0.5 if len(s) == 2 else 0.1) for k, s in shapes.items()}


def slice_of(v):
    """The first 512 values (flattened) of a larger tensor, else the whole tensor; the float64 checksums cover the rest."""
    return v.reshape(-1)[:512]


def g12_cvae_regressor():
    from models import pose_behavior_rnn as rb
    arrays = {}
    meta = {"seed": SEED, "steps": STEPS, "batch": BSZ, "seq_len": T_LEN, "recon_loss_weight": W_RECON, "gamma_init": GAMMA,
            "gamma_step": GAMMA_STEP, "imax": IMAX, "lr": LR, "reg_lr": REG_LR, "kps_scale": list(KPS_SCALE),
            "kw": dict(n_kps=N_KPS, information_bottleneck=True, decoder_arch="lstm", linear_in_decoder=False, dim_hidden_b=HID),
            "cases": {}}
    gen = torch.Generator().manual_seed(SEED)
    idx_all = torch.randint(0, T_LEN, (STEPS, 5), generator=gen)
    arrays["idx"] = idx_all.numpy().astype("int32")
    for tag, c in CASES.items():
        torch.manual_seed(SEED)
        net = rb.ResidualBehaviorNet(**meta["kw"])
        sd = behavior_state(net, SEED)
        net.train()
        net.b_enc.init_hidden = lambda bs, device, net=net: rb.BEncoder.init_hidden(net.b_enc, bs, "cpu")
        reg = rb.Regressor_fly(HID, N_KPS)
        rsd = regressor_state({k: list(v.shape) for k, v in reg.state_dict().items()}, SEED)
        reg.load_state_dict(rsd)
        meta["shapes"], meta["reg_shapes"] = {k: list(v.shape) for k, v in sd.items()}, {k: list(v.shape) for k, v in rsd.items()}
        opt = torch.optim.Adam([{"params": net.b_enc.parameters(), "name": "z_enc"}, {"params": net.decoder.parameters(), "name": "dec"}],
                               lr=LR)
        ropt = Adam131(reg.parameters(), REG_LR)
        rec_loss = torch.nn.MSELoss(reduction="none")
        gamma, logs = GAMMA, []
        for it in range(STEPS):
            kps = KPS_SCALE[it] * seeded_randn(f"reg.kps{it}", (BSZ, T_LEN + 1, N_KPS), SEED)
            seq_b, target = kps[:, :-1], kps[:, 1:]
            with FixedNoise(f"reg.s{it}", SEED):
                xs, cs, _, bs, mu, logstd, pre = net(seq_b, seq_b, T_LEN)
            r = rec_loss(xs, target)
            recon = torch.mean(r)
            kl = rl.kl_loss(mu, logstd)
            tuning = 1.0 if c["cvae"] else gamma
            loss = W_RECON * recon + tuning * kl
            ls, w4 = [], None
            for k in range(5):
                idx = idx_all[it, k:k + 1]
                oh = torch.nn.functional.one_hot(idx.repeat(mu.size(0)), num_classes=T_LEN)
                if k == 4:
                    w4 = {n: p.detach().clone() for n, p in reg.named_parameters()}
                loss_regressor = torch.mean((reg(mu, oh.float()) - seq_b[:, idx].squeeze()) ** 2)
                ropt.zero_grad()
                loss_regressor.backward(retain_graph=True)
                ropt.step()
                ls.append(float(loss_regressor.detach()))
            term = torch.clamp(loss_regressor, max=0.45) * c["w"] + torch.clamp(loss_regressor, max=0.7) * c["w"]
            adv, = torch.autograd.grad(-term, mu, retain_graph=True)      # through W^5 (the .data writes) and forward 5's masks
            # the same with the weights before the fifth update (what torch >= 1.5 semantics would give)
            f = torch.func.functional_call(reg, w4, (mu, oh.float()))
            l4 = torch.mean((f - seq_b[:, idx].squeeze()) ** 2)
            adv4, = torch.autograd.grad(-(torch.clamp(l4, max=0.45) * c["w"] + torch.clamp(l4, max=0.7) * c["w"]), mu, retain_graph=True)
            loss = loss - torch.clamp(loss_regressor, max=0.45) * c["w"]
            loss = loss - torch.clamp(loss_regressor, max=0.7) * c["w"]
            opt.zero_grad()
            loss.backward()
            opt.step()
            used = gamma
            gamma = max(gamma - GAMMA_STEP * (IMAX - float(kl)), 0)
            l5 = ls[-1]
            logs.append({"loss": float(loss), "loss_recon": float(recon), "kl_loss": float(kl), "gamma_used": used, "gamma": gamma,
                         "mu_s": float(torch.mean(mu)), "logstd_s": float(torch.mean(logstd)), "loss_regressor": l5, "L": ls,
                         "band": "<=0.45" if l5 <= 0.45 else ("<=0.7" if l5 <= 0.7 else ">0.7"),
                         "adv_w4_vs_w5": float((adv4 - adv).abs().max() / adv.abs().max()) if float(adv.abs().max()) else 0.0})
            arrays[f"{tag}.mu{it}"] = mu.detach().numpy()
            arrays[f"{tag}.adv{it}"] = adv.numpy()
            if it == 0 and tag == "shipped":
                fin0 = reg.state_dict()
                meta["reg_after_step0"] = {k: [float(v.double().sum()), float(v.double().abs().sum())] for k, v in fin0.items()}
                for k, v in fin0.items():
                    arrays[f"{tag}.reg0.{k}"] = slice_of(v).clone().numpy()   # (state_dict() shares the live parameters)
                arrays[f"{tag}.adv4_0"] = adv4.numpy()
        fin = net.state_dict()
        rfin = reg.state_dict()
        case = {"logs": logs, "w": c["w"], "cvae": c["cvae"], "adam_step": int(opt.state_dict()["state"][0]["step"]),
                "reg_adam_step": ropt.state[0]["step"],
                "checksums": {k: [float(v.double().sum()), float(v.double().abs().sum())] for k, v in fin.items()},
                "reg_checksums": {k: [float(v.double().sum()), float(v.double().abs().sum())] for k, v in rfin.items()}}
        for k, v in fin.items():
            arrays[f"{tag}.final.{k}"] = slice_of(v).numpy()
        for k, v in rfin.items():
            arrays[f"{tag}.reg.{k}"] = slice_of(v).numpy()
        names = [n for n, _ in net.named_parameters()]
        st = opt.state_dict()["state"]
        for n in ("decoder.rnn.weight_hh", "b_enc.mu_fn.conv.weight_v", "decoder.n_out.bias"):
            arrays[f"{tag}.exp_avg.{n}"] = slice_of(st[names.index(n)]["exp_avg"]).numpy()
        for (n, _), s in zip(reg.named_parameters(), ropt.state):
            arrays[f"{tag}.reg_exp_avg.{n}"] = slice_of(s["exp_avg"]).numpy()
            arrays[f"{tag}.reg_exp_avg_sq.{n}"] = slice_of(s["exp_avg_sq"]).numpy()
        meta["cases"][tag] = case
        print(tag, [(round(l["loss_regressor"], 4), l["band"], f"{l['adv_w4_vs_w5']:.1e}") for l in logs])
    save("g12_cvae_regressor", meta, arrays)


if __name__ == "__main__":
    torch.manual_seed(0)
    torch.set_num_threads(4)
    assert G.REF
    g12_cvae_regressor()
