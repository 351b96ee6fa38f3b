#!/usr/bin/env python3
"""Time the real-vs-fake classifier study (behavior_eval.classifier_study) at the reference sizes: 25 024 synthetic rows,
T = 50, bs 256, 2000 iterations (1 940 trained + 97 final-pass), six start times, with a flow, H = 1024 -- and the same loop
structure on torch.nn.GRU + torch.optim.SGD / Adam on the same GPU (the project's restatement of
experiments/behavior_net.py:1315-1521 with torch modules, one start time timed over --torch-iters iterations and scaled to
1 940 x 6).  Prints one JSON line; --out writes it too.

    python tools/time_classifier_study.py --out profiles/classifier_study_time.json
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/time_classifier_study.py --iterations 200   # device time per kernel
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from behavior_driven_video_synthesis_amd import behavior_eval as E  # noqa: E402


def torch_loop(sets, start, bs, iters):
    """One start time of :1315-1456 with torch modules (prior, cross, self, flow classifiers, regressor), ``iters`` iterations."""
    dev = sets["orig"].device
    cls = {k: E._Classifier().to(dev) for k in ("prior", "cross", "flow")}
    selfc = E._Classifier().to(dev)
    reg = E._Regressor(sets["embed"].shape[1]).to(dev)
    opt = {k: torch.optim.SGD(m.parameters(), lr=1e-3, momentum=0.9) for k, m in cls.items()}
    ropt = torch.optim.Adam(reg.parameters(), lr=1e-3)
    bce = torch.nn.BCEWithLogitsLoss()

    def fwd(m, x):
        _, h = m.GRU(x)
        return m.fc1(h.reshape(x.shape[0], -1))

    nb = sets["orig"].shape[0] // bs
    log = []
    for it in range(iters):
        i = it % nb
        sl = slice(i * bs, (i + 1) * bs)
        for k, m in cls.items():
            p = fwd(m, sets[k][sl])
            log.append(torch.mean(torch.sigmoid(p)).item())
            loss = bce(p, torch.zeros_like(p)) + bce(fwd(m, sets["orig"][sl]), torch.ones_like(p))
            log.append(loss.item())
            opt[k].zero_grad()
            loss.backward()
            opt[k].step()
        with torch.no_grad():
            log.append(torch.mean(torch.sigmoid(fwd(selfc, sets["self"][sl]))).item())
        pred = reg.fc3(torch.relu(reg.fc2(torch.relu(reg.fc1(sets["embed"][sl])))))
        loss = torch.mean(torch.norm(pred - sets["orig"][sl, start], dim=1))
        ropt.zero_grad()
        loss.backward()
        ropt.step()
        log.append(loss.item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=25024)
    ap.add_argument("--iterations", type=int, default=2000)
    ap.add_argument("--torch-iters", type=int, default=60)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    g = torch.Generator().manual_seed(0)
    n, t, bs = a.rows, 50, 256
    sets = {k: torch.randn(n, t, 51, generator=g).cuda() for k in ("orig", "prior", "cross", "self", "flow")}
    sets["embed"] = torch.randn(n, 1024, generator=g).cuda()
    torch.manual_seed(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = E.classifier_study(sets, bs=bs, iterations=a.iterations)
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    nb = n // bs
    n_it = out["epochs"] * nb + nb
    res = {"rows": n, "T": t, "bs": bs, "iterations": a.iterations, "epochs": out["epochs"], "replayed_iterations": n_it,
           "start_times": 6, "flow": True, "hip_total_s": round(total, 3), "hip_ms_per_iteration": round(1e3 * total / n_it, 3),
           "final": out["final"]}
    if not a.no_torch:
        torch_loop(sets, 0, bs, 3)                     # warm-up (MIOpen kernel selection)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch_loop(sets, 0, bs, a.torch_iters)
        torch.cuda.synchronize()
        per = (time.perf_counter() - t0) / a.torch_iters
        res.update(torch_ms_per_iteration_one_start=round(1e3 * per, 3), torch_iters_timed=a.torch_iters,
                   torch_total_s_scaled=round(per * (out["epochs"] * nb) * 6, 1),
                   torch_note="one start time timed over torch_iters iterations, scaled to the trained iterations x 6 start times")
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
