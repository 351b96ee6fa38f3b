#!/usr/bin/env python3
"""Golden-vector generator for the real-vs-fake classifier study (g14).  Runs ONLY in the build container (needs the reference
checkout, as make_golden.py does, whose helpers it imports).

The reference's own ``Classifier`` and ``Regressor`` (models/pose_behavior_rnn.py:6-17, :33-44), in float32 on the CPU, driven
by the inline loop of ``run_inference`` (experiments/behavior_net.py:1315-1521), restated below with ``bs``, ``iterations`` and
``times`` as parameters -- including ``class_real_self``'s optimiser over ``class_real2``'s parameters.  Inputs and initial
weights come from tests/classifier_study_ref.py (``synth.seeded_randn``), so the fixture stores only results.

    python tests/golden/make_golden_classifier_study.py      # regenerate tests/golden/g14_classifier_study.npz
"""
import os
import sys

import numpy as np
import torch
from torch import nn
from torch.optim import SGD, Adam

import make_golden  # noqa: F401  (puts the reference checkout on sys.path)
from make_golden import save

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import classifier_study_ref as R  # noqa: E402
from models.pose_behavior_rnn import Classifier, Regressor  # noqa: E402


def study(sets, init, times, bs, iterations):
    flow = "flow" in sets
    X_orig, X_prior, X_cross, X_self, X_embed = (sets[k] for k in ("orig", "prior", "cross", "self", "embed"))
    X_flow = sets.get("flow")
    num_samples = X_orig.shape[0]
    epochs = iterations // (num_samples // bs)
    finals, curves = [], []
    for si, start in enumerate(times):
        loss1, loss2, loss_regressor, acc1, acc2, acc_flow, acc_self, loss_self, loss_flow = ([] for _ in range(9))
        class_real1 = Classifier(51, 1)
        class_real1.load_state_dict(init[si]["prior"])
        optimizer_classifier_real1 = SGD(class_real1.parameters(), lr=0.001, momentum=0.9)
        class_real2 = Classifier(51, 1)
        class_real2.load_state_dict(init[si]["cross"])
        optimizer_classifier_real2 = SGD(class_real2.parameters(), lr=0.001, momentum=0.9)
        if flow:
            class_flow = Classifier(51, 1)
            class_flow.load_state_dict(init[si]["flow"])
            optimizer_classifier_flow = SGD(class_flow.parameters(), lr=0.001, momentum=0.9)
        regressor = Regressor(X_embed.shape[1], 51)
        regressor.load_state_dict(init[si]["regressor"])
        optimizer_regressor = Adam(regressor.parameters(), lr=0.001)
        class_real_self = Classifier(51, 1)
        class_real_self.load_state_dict(init[si]["self"])
        optimizer_classifier_real_self = SGD(class_real2.parameters(), lr=0.001, momentum=0.9)
        cls_loss = nn.BCEWithLogitsLoss(reduction="mean")

        def pair(model, opt, x_fake, x_true, accs, losses):
            predict = model(x_fake)
            loss_gen = cls_loss(predict, torch.zeros_like(predict))
            accs.append(torch.mean(nn.Sigmoid()(predict)).item())
            predict = model(x_true)
            loss = loss_gen + cls_loss(predict, torch.ones_like(predict))
            losses.append(loss.item())
            opt.zero_grad()
            loss.backward()
            opt.step()

        for _ in range(epochs):
            for i in range(num_samples // bs):
                sl = slice(i * bs, (i + 1) * bs)
                x_true, x_mu, x_start = X_orig[sl], X_embed[sl], X_orig[sl, start]
                pair(class_real1, optimizer_classifier_real1, X_prior[sl], x_true, acc1, loss1)
                pair(class_real2, optimizer_classifier_real2, X_cross[sl], x_true, acc2, loss2)
                pair(class_real_self, optimizer_classifier_real_self, X_self[sl], x_true, acc_self, loss_self)
                if flow:
                    pair(class_flow, optimizer_classifier_flow, X_flow[sl], x_true, acc_flow, loss_flow)
                predict = regressor(x_mu)
                loss_regressor_ = torch.mean(torch.norm(predict - x_start, dim=1))
                optimizer_regressor.zero_grad()
                loss_regressor_.backward()
                optimizer_regressor.step()
                loss_regressor.append(loss_regressor_.item())
        cur = {"acc1": acc1, "loss1": loss1, "acc2": acc2, "loss2": loss2, "acc_self": acc_self, "loss_regressor": loss_regressor}
        if flow:
            cur.update(acc_flow=acc_flow, loss_flow=loss_flow)
        f = {k: [] for k in ("Acc Prior", "Acc Cross", "Acc Self", "Acc Flow", "Loss_regressor", "DE")}
        for i in range(num_samples // bs):
            sl = slice(i * bs, (i + 1) * bs)
            x_start = X_orig[sl, start]
            f["DE"].append(torch.mean(torch.norm(X_cross[sl][:, start] - x_start, dim=1)).item())
            f["Acc Prior"].append(torch.mean(nn.Sigmoid()(class_real1(X_prior[sl]))).item())
            f["Acc Cross"].append(torch.mean(nn.Sigmoid()(class_real2(X_cross[sl]))).item())
            f["Acc Self"].append(torch.mean(nn.Sigmoid()(class_real_self(X_self[sl]))).item())
            if flow:
                f["Acc Flow"].append(torch.mean(nn.Sigmoid()(class_flow(X_flow[sl]))).item())
            predict = regressor(X_embed[sl])
            loss_regressor_ = torch.mean(torch.norm(predict - x_start, dim=1))
            optimizer_regressor.zero_grad()
            loss_regressor_.backward()
            optimizer_regressor.step()
            f["Loss_regressor"].append(loss_regressor_.item())
        finals.append({k: float(np.mean(v)) for k, v in f.items() if v})
        curves.append({k: np.asarray(v, dtype=np.float64) for k, v in cur.items()})
    return finals, curves


def main():
    torch.set_num_threads(1)
    meta, arrays = {"cases": {}}, {}
    for tag, (flow, n, t, h, bs, iters, times) in R.CASES.items():
        sets, init = R.inputs(tag)
        finals, curves = study(sets, init, list(times), bs, iters)
        meta["cases"][tag] = {"flow": flow, "rows": n, "T": t, "H": h, "bs": bs, "iterations": iters, "times": list(times),
                              "final": finals}
        for si, c in enumerate(curves):
            for k, v in c.items():
                arrays[f"{tag}.{si}.{k}"] = v
    save("g14_classifier_study", meta, arrays)


if __name__ == "__main__":
    main()
