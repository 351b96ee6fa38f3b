#!/usr/bin/env python3
"""Time what an unchanged reference ``train_fn`` costs on the cVAE stage through the drop-in, at config/behavior_net.yaml's sizes
(64 rows, 50 frames, dim_hidden_b 1024, 51 pose dimensions): eager launches under autograd, ``torch.optim.Adam``.

    three   the reference's iteration (experiments/behavior_net.py:611-686): pass 1 and its losses, the dead pass 2, zero_grad /
            backward / Adam step, pass 3 on the stepped weights, CrossEntropyLoss(classifier_beta(mu_s)), its backward (back
            through the encoder) and the classifier's own Adam step
    single  one pass, its losses, zero_grad / backward / Adam step -- all that a tree without pass slots can run

Both are timed in one process, their windows alternated (device events around ``--reps`` iterations; the median window counts).

    python tools/time_dropin_cvae.py [--reps 20] [--windows 7] [--single-only] [--root TREE]
    python tools/time_dropin_cvae.py --against PARENT_TREE [--runs 3] [--out profiles/dropin_cvae_time.txt]

``--root TREE`` imports the package from another tree (an export of another revision with its built library beside it).
``--against PARENT_TREE`` is the comparison with another revision: fresh child processes, alternated -- PARENT_TREE (single only),
this tree, PARENT_TREE, this tree, ... ``--runs`` times each.  The spread of PARENT_TREE's single-pass time against itself (the
largest difference between two of its runs' medians) is the yardstick: this tree's single-pass time (median of its runs) must not
be slower than the parent's median by more than that spread, or the exit status is 1.  Everything is written to ``--out``.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
ROWS, FRAMES, HIDDEN, N_KPS, N_CLASSES = 64, 50, 1024, 51, 13


def measure(args):
    sys.path.insert(0, os.path.abspath(args.root) if args.root else ROOT)
    import torch
    from behavior_driven_video_synthesis_amd.models.pose_behavior_rnn import ResidualBehaviorNet
    torch.manual_seed(0)
    net = ResidualBehaviorNet(N_KPS, information_bottleneck=True, decoder_arch="lstm", dim_hidden_b=HIDDEN)
    net.decoder.n_out.weight.data.mul_(0.05)
    net = net.cuda().train()
    classifier_beta = torch.nn.Linear(HIDDEN, N_CLASSES).cuda()
    optimizer = torch.optim.Adam([{"params": net.b_enc.parameters(), "name": "z_enc"}, {"params": net.decoder.parameters(), "name": "dec"}],
                                 lr=1e-4)
    optimizer_classifier_beta = torch.optim.Adam(classifier_beta.parameters(), lr=0.001)
    kps = 0.5 * torch.randn(ROWS, FRAMES + 1, N_KPS, device="cuda")
    seq_b, target = kps[:, :-1].contiguous(), kps[:, 1:].contiguous()
    seq_2 = (0.5 * torch.randn(ROWS, FRAMES, N_KPS, device="cuda"))
    labels = torch.randint(0, N_CLASSES, (ROWS,), device="cuda")
    gamma, w_recon = 0.01, 2.5

    def first_pass_and_step():
        xs, cs, _, bs, mu_s, logstd_s, pre_s = net(seq_b, seq_b, FRAMES)
        recon = torch.mean(torch.nn.functional.mse_loss(xs, target, reduction="none"))
        kl = (torch.sum(-logstd_s + 0.5 * (torch.exp(logstd_s) ** 2 + mu_s ** 2), dim=-1) - 0.5 * HIDDEN).mean()
        return w_recon * recon + gamma * kl

    def single():
        loss = first_pass_and_step()
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()

    def three():
        loss = first_pass_and_step()
        dead = net(seq_2, seq_b, FRAMES)       # noqa: F841  (held, as the reference's locals hold it, until the function returns)
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        _, _, _, _, mu_s, *_ = net(seq_b, seq_b, FRAMES)
        loss_cls = torch.nn.CrossEntropyLoss()(classifier_beta(mu_s), labels)
        optimizer_classifier_beta.zero_grad()
        loss_cls.backward()
        optimizer_classifier_beta.step()

    modes = {"single": single} if args.single_only else {"single": single, "three": three}
    for fn in modes.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {m: [] for m in modes}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.windows):
        for m, fn in modes.items():
            a.record()
            for _ in range(args.reps):
                fn()
            b.record()
            torch.cuda.synchronize()
            times[m].append(a.elapsed_time(b) / args.reps)
    res = {"tree": "other" if args.root else "this", "rows": ROWS, "frames": FRAMES, "hidden": HIDDEN, "reps": args.reps}
    for m, ts in times.items():
        res[m + "_ms"] = round(statistics.median(ts), 4)
        res[m + "_windows_ms"] = [round(t, 4) for t in ts]
    print(json.dumps(res), flush=True)


def child(args, root, single_only):
    cmd = [sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--windows", str(args.windows)]
    if root:
        cmd += ["--root", root]
    if single_only:
        cmd += ["--single-only"]
    env = dict(os.environ)
    if root:    # the other tree's own build of the library, not this one's
        env["VUNET_HIP_LIB"] = os.path.join(os.path.abspath(root), "behavior_driven_video_synthesis_amd", "libvunet_hip.so")
    else:
        env.pop("VUNET_HIP_LIB", None)
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=args.child_timeout)
    if out.returncode != 0:
        raise SystemExit(f"{' '.join(cmd)} exited with {out.returncode}:\n{out.stderr[-2000:]}")
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(json.dumps(res), flush=True)
    return res


def against(args):
    parent, mine = [], []
    for _ in range(args.runs):
        parent.append(child(args, args.against, True))
        mine.append(child(args, None, False))
    p = [r["single_ms"] for r in parent]
    s = [r["single_ms"] for r in mine]
    t = [r["three_ms"] for r in mine]
    spread = max(p) - min(p)
    p_med, s_med, t_med = statistics.median(p), statistics.median(s), statistics.median(t)
    ok = s_med <= p_med + spread
    lines = [
        f"cVAE stage through the drop-in, eager launches under autograd + torch.optim.Adam: {ROWS} rows x {FRAMES} frames, hidden {HIDDEN}",
        f"(tools/time_dropin_cvae.py --against <parent tree> --runs {args.runs} --reps {args.reps} --windows {args.windows}; one MI355X; child",
        "processes alternated parent / this tree; per process the median of its windows, windows of the two loops alternated)",
        "",
        f"single pass + backward + step, parent tree   : runs {p} ms  median {p_med:.4f} ms",
        f"  spread of the parent against itself        : {spread:.4f} ms (largest difference between two runs)",
        f"single pass + backward + step, this tree     : runs {s} ms  median {s_med:.4f} ms",
        f"  difference to the parent's median          : {s_med - p_med:+.4f} ms  -> {'within' if ok else 'OUTSIDE'} the parent's own spread",
        f"three-pass iteration (:611-686), this tree   : runs {t} ms  median {t_med:.4f} ms  (the parent cannot run it)",
        f"  = {t_med / s_med:.2f} x the single pass's time",
        "",
        "raw:",
    ] + [json.dumps(r) for r in parent + mine]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    if not ok:
        raise SystemExit(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--single-only", action="store_true")
    ap.add_argument("--root", default=None)
    ap.add_argument("--against", default=None)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dropin_cvae_time.txt"))
    args = ap.parse_args()
    if args.against:
        return against(args)
    measure(args)


if __name__ == "__main__":
    main()
