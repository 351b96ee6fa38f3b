#!/usr/bin/env python3
"""Time the post-hoc pose-regressor probe at the reference sizes (B = 8, latents 128 x 8 x 8 and 128 x 4 x 4, n_out 34):

  * one training step of the module route (``Regressor.forward`` + autograd + ``FusedAdam``) and of the fused engine
    (reg_probe.RegProbeEngine: recorded and replayed; and issued eagerly),
  * the split-K embedder alone (vunet_reg_probe_embed + _finish) against ``ops.fused_conv`` on the same operand,
  * one probe iteration including the encoder pass (``ed(eu(x))`` at 256 x 256 under no_grad, then one step).

Device events around windows of many calls after a warm-up; the two routes of a pair alternate, ``--rounds`` windows each, and
the median and the spread (min .. max) of the windows are printed.  Needs the GPU; there is no fallback.

    python tools/time_reg_probe.py --out profiles/reg_probe_time.txt
"""
import argparse
import ctypes
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def window(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / calls     # us per call


def compare(named, calls, rounds, warm=20):
    for _, fn in named:
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {n: [] for n, _ in named}
    for _ in range(rounds):
        for n, fn in named:                    # alternating
            times[n].append(window(fn, calls))
    return {n: (statistics.median(v), min(v), max(v)) for n, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--no-encoder", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("time_reg_probe needs an MI355X")
    from behavior_driven_video_synthesis_amd import _lib, ops
    from behavior_driven_video_synthesis_amd.models.vunets import Regressor
    from behavior_driven_video_synthesis_amd.optim import FusedAdam
    from behavior_driven_video_synthesis_amd.reg_probe import split_k
    B = a.batch
    torch.manual_seed(0)
    kw = dict(n_out=34, n_latent_scales=2, nf_max=128, latent_widths=[8, 4], linear_width_factor=1, n_linear=2)
    means = [torch.randn(B, 128, 4, 4, device="cuda"), torch.randn(B, 128, 8, 8, device="cuda")]
    tgt = torch.rand(B, 34, device="cuda")
    lines = [f"# tools/time_reg_probe.py: B = {B}, latents 128x8x8 + 128x4x4, n_out 34; {a.calls} calls per window, {a.rounds} windows "
             f"per route, alternating; us per call: median (min .. max); {torch.cuda.get_device_name(0)}"]

    def row(title, res):
        for n, (med, lo, hi) in res.items():
            lines.append(f"{title:<34} {n:<28} {med:9.1f} us  ({lo:.1f} .. {hi:.1f})")
        print("\n".join(lines[-len(res):]), flush=True)

    # ---- one training step, old route and new
    reg_old = Regressor(**kw).cuda()
    opt = FusedAdam(list(reg_old.parameters()), lr=0.001)

    def step_old():
        loss = torch.norm(reg_old(means) - tgt, dim=1).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
    reg_new = Regressor(**kw).cuda()
    eng = reg_new.probe_engine()
    reg_eager = Regressor(**kw).cuda()
    eng_eager = reg_eager.probe_engine()
    eng_eager.graph.enabled = False
    row("training step", compare([("module+autograd+FusedAdam", step_old), ("engine (graph replay)", lambda: eng.step(means, tgt)),
                                  ("engine (eager issue)", lambda: eng_eager.step(means, tgt))], a.calls, a.rounds))

    # ---- the split-K embedder alone against fused_conv on the same operand
    lib = _lib.lib()
    for k_w in (8, 4):
        K = 128 * k_w * k_w
        w = (torch.randn(128, K, device="cuda") * (1.5 / K) ** 0.5).contiguous()
        bias = torch.zeros(128, device="cuda")
        x = torch.zeros(16 * ((B + 15) // 16), K, device="cuda")
        x[:B].normal_()
        S = split_k(128, K)
        part, y = torch.empty(S * x.shape[0] * 128, device="cuda"), torch.zeros(x.shape[0], 128, device="cuda")
        p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

        def split(x=x, w=w, K=K, S=S):
            lib.vunet_reg_probe_embed(p(x), p(w), B, 128, K, S, p(part), st)
            lib.vunet_reg_probe_embed_finish(p(part), S, p(bias), B, 128, p(y), 128, 0, st)
        x4, w4 = x[:B].reshape(B, K, 1, 1).contiguous(), w.reshape(128, K, 1, 1)

        def conv(x4=x4, w4=w4):
            with torch.no_grad():
                ops.fused_conv(x4, None, None, w4, None, bias, None, None, ops.ConvCfg(kind=1, k=1, out_act=ops.ACT_RELU))
        row(f"embedder 128 x {K} (S = {S})", compare([("split-K embed + finish", split), ("fused_conv 1x1", conv)], a.calls, a.rounds))

    # ---- one probe iteration including the encoder pass
    if not a.no_encoder:
        from behavior_driven_video_synthesis_amd.models.vunets import VunetAlter
        net = VunetAlter(spatial_size=256, bottleneck_factor=2, box_factor=2, n_scales=0, n_latent_scales=2, conv_layer_type="l1",
                         nf_start=32, nf_max=128, subpixel_upsampling=True, dropout_prob=0.0).cuda().eval()
        img = torch.rand(B, 3, 256, 256, device="cuda") * 2 - 1

        def encode():
            with torch.no_grad():
                return net.ed(net.eu(img), None)[1]

        def it_old():
            m = encode()
            loss = torch.norm(reg_old(m) - tgt, dim=1).mean()
            opt.zero_grad()
            loss.backward()
            opt.step()
        row("probe iteration with encoder", compare([("module route", it_old), ("engine (graph replay)", lambda: eng.step(encode(), tgt))],
                                                    max(a.calls // 10, 10), a.rounds, warm=5))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
