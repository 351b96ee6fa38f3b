#!/usr/bin/env python3
"""Golden-vector generator for one whole iteration of the cVAE stage (g18).  Runs ONLY in the build container (needs the reference
checkout, as make_golden.py does, whose helpers it imports).

``make_golden.py::g11_cvae_training`` drives the reference's ``ResidualBehaviorNet`` through the part of ``train_fn`` that forms
the loss.  This one drives it, in float32 on the CPU, through everything ``train_fn`` (experiments/behavior_net.py:611-686) does
with the net per iteration -- THREE calls of one shape, all under ``enable_grad`` --, for K = 3 iterations, in its order:

    pass 1   net(seq_b, seq_b, seq_len)                         :616   recon loss (:621), kl_loss (:623)
    pass 2   net(seq_2, seq_b, seq_len)                         :627   none of its outputs is used
             loss = recon_loss_weight * recon + gamma * kl      :633
             zero_grad, loss.backward(), Adam(lr).step()        :657-659
             gamma update                                       :661, :111-116
    pass 3   net(seq_b, seq_b, seq_len) -> mu_s                 :681   on the stepped weights
             CrossEntropyLoss(classifier_beta(mu_s), labels)    :682-683
             zero_grad of the classifier's optimiser ONLY, backward (it runs back through the net's encoder: the net's
             ``.grad`` now hold pass 1's + pass 3's), Adam(lr=0.001).step() of the classifier            :684-686

with recorded reparametrisation noise for each of the three passes.  ``use_regressor`` is off (g11 records why) and the two
classifiers on the raw poses (:664-678) are left out: they never touch the net.  Sizes as in g11: 51 pose dimensions, hidden
width 64, 5 rows, T = 6; 4 action classes, fixed labels.

    python tests/golden/make_golden_cvae_iteration.py      # regenerate tests/golden/g18_cvae_iteration.npz
"""
import torch

import make_golden  # noqa: F401  (puts the reference checkout on sys.path)
from make_golden import FixedNoise, behavior_state, save
from synth import seeded_randn

from lib import losses as rl  # noqa: E402
from models import pose_behavior_rnn as rb  # noqa: E402

SEED = 118
N_KPS, HID, BSZ, T_LEN, N_CLASSES = 51, 64, 5, 6, 4
LABELS = [0, 3, 1, 2, 1]
W_RECON, GAMMA, GAMMA_STEP, IMAX, LR, LR_CLS = 2.5, 0.05, 1e-3, 5.0, 1e-3, 0.001


def main():
    torch.manual_seed(SEED)
    torch.set_num_threads(1)
    kw = dict(n_kps=N_KPS, information_bottleneck=True, decoder_arch="lstm", linear_in_decoder=False, dim_hidden_b=HID)
    net = rb.ResidualBehaviorNet(**kw)
    sd = behavior_state(net, SEED)
    net.train()
    net.b_enc.init_hidden = lambda bs, device: rb.BEncoder.init_hidden(net.b_enc, bs, "cpu")   # get_device() is -1 on CPU
    classifier_beta = rb.Classifier_action_beta(HID, N_CLASSES)
    with torch.no_grad():
        classifier_beta.fc1.weight.copy_(0.1 * seeded_randn("cvit.cls.weight", (N_CLASSES, HID), SEED))
        classifier_beta.fc1.bias.copy_(0.1 * seeded_randn("cvit.cls.bias", (N_CLASSES,), SEED))
    optimizer = torch.optim.Adam([{"params": net.b_enc.parameters(), "name": "z_enc"},
                                  {"params": net.decoder.parameters(), "name": "dec"}], lr=LR)                    # :324-336
    optimizer_classifier_beta = torch.optim.Adam(classifier_beta.parameters(), lr=LR_CLS)                          # :302
    labels = torch.tensor(LABELS)
    rec_loss = torch.nn.MSELoss(reduction="none")
    gamma = GAMMA
    meta = {"seed": SEED, "steps": 3, "kw": kw, "batch": BSZ, "seq_len": T_LEN, "n_classes": N_CLASSES, "labels": LABELS,
            "recon_loss_weight": W_RECON, "gamma_init": GAMMA, "gamma_step": GAMMA_STEP, "imax": IMAX, "lr": LR, "lr_classifier": LR_CLS,
            "shapes": {k: list(v.shape) for k, v in sd.items()}, "logs": [], "noise_shapes": []}
    arrays = {}
    named = dict(net.named_parameters())
    for it in range(meta["steps"]):
        kps = 0.5 * seeded_randn(f"cvit.kps{it}", (BSZ, T_LEN + 1, N_KPS), SEED)
        kps_cross = 0.5 * seeded_randn(f"cvit.kpsx{it}", (BSZ, T_LEN + 1, N_KPS), SEED)
        seq_b, target_self = kps[:, :-1], kps[:, 1:]                      # prepare_input (lib/utils.py:914-917)
        seq_2 = kps_cross[:, :-1]
        with torch.enable_grad():
            with FixedNoise(f"cvit.s{it}.p1", SEED) as fn1:
                xs, cs, _, bs, mu_s, logstd_s, pre_s = net(seq_b, seq_b, T_LEN)
            r = rec_loss(xs, target_self)
            recon_loss = torch.mean(r)
            kl_loss_avg = rl.kl_loss(mu_s, logstd_s)
            with FixedNoise(f"cvit.s{it}.p2", SEED) as fn2:
                xt, ct, _, bt, mu_t, logstd_t, pre_t = net(seq_2, seq_b, T_LEN)
            loss = W_RECON * recon_loss + gamma * kl_loss_avg
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            used = gamma
            gamma = max(gamma - GAMMA_STEP * (IMAX - float(kl_loss_avg.detach())), 0)
            log = {"loss": float(loss.detach()), "loss_recon": float(recon_loss.detach()), "kl_loss": float(kl_loss_avg.detach()),
                   "gamma_used": used, "gamma": gamma, "mu_s": float(torch.mean(mu_s.detach())),
                   "logstd_s": float(torch.mean(logstd_s.detach()))}
            dec_grad_before = named["decoder.rnn.weight_hh"].grad.clone()
            enc_grad_before = named["b_enc.rnn.weight_hh_l0"].grad.clone()
            with FixedNoise(f"cvit.s{it}.p3", SEED) as fn3:
                _, _, _, _, mu_s, *_ = net(seq_b, seq_b, T_LEN)
            predict = classifier_beta(mu_s)
            loss_classifier_action_beta = torch.nn.CrossEntropyLoss()(predict, labels)
            optimizer_classifier_beta.zero_grad()
            loss_classifier_action_beta.backward()
            optimizer_classifier_beta.step()
        log["loss_classifier_action_beta"] = float(loss_classifier_action_beta.detach())
        meta["logs"].append(log)
        meta["noise_shapes"].append([fn1.shapes, fn2.shapes, fn3.shapes])
        assert fn1.shapes == fn2.shapes == fn3.shapes == [[BSZ, HID]], (fn1.shapes, fn2.shapes, fn3.shapes)
        # pass 3 reaches the encoder and the heads only: the decoder's gradients are pass 1's, the encoder's the sum of both
        assert torch.equal(named["decoder.rnn.weight_hh"].grad, dec_grad_before)
        assert not torch.equal(named["b_enc.rnn.weight_hh_l0"].grad, enc_grad_before)
        if it == 0:
            arrays["grad0.b_enc.rnn.weight_hh_l0"] = named["b_enc.rnn.weight_hh_l0"].grad.numpy().copy()
            arrays["grad0.decoder.rnn.weight_hh"] = named["decoder.rnn.weight_hh"].grad.numpy().copy()
            arrays["mu3_0"] = mu_s.detach().numpy().copy()       # pass 3's mu of iteration 0 (on the weights after the first step)
    fin = net.state_dict()
    meta["checksums"] = {k: [float(v.double().sum()), float(v.double().abs().sum())] for k, v in fin.items()}
    for k, v in fin.items():
        arrays[f"final.{k}"] = (v[:24] if v.dim() == 2 and v.shape[0] > 64 else v).numpy().copy()
    for k, v in classifier_beta.state_dict().items():
        arrays[f"classifier_beta.{k}"] = v.numpy().copy()
    meta["adam_step"] = int(optimizer.state_dict()["state"][0]["step"])
    save("g18_cvae_iteration", meta, arrays)


if __name__ == "__main__":
    main()
