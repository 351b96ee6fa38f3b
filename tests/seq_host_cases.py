"""Small cases that between them reach every host branch of the seq engines (seq.FlowEngine / BehaviorEngine, seq_train's
train engines and autograd passes, the fused cVAE step of experiments.behavior_net), and a recorder for them.  Used by
tools/fused_conv_trace.py --cases=seq_host_cases (which records tests/seq_host_trace.json from the PARENT of a host-side
refactor) and by tests/test_hip_seq_host_trace.py (which replays the cases on the tree under test).

A record holds, per case: the trace of native calls ([entry point, stream ordinal, return code], as tests/fused_conv_cases.py
logs them, weight packing included) with every engine's ``graph.enabled`` False, so that each launch is visible, and the
SHA-256 of every output and gradient.  A case builds its modules afresh and runs once: several are first calls by nature
(ActNorm's data-dependent initialisation, the first steps of an optimiser).

Shapes: a flow of 2 blocks over 7 channels (c1 = 4 != 7 / 2) with hidden width 64; a behaviour net with H = 64 and 6 pose
dimensions, t_in = length = 3, at 3 rows (b_pad 16: h travels as rows) and 48 rows (the smallest b_pad at which h travels as
tiles).  The regressor's kernels take H as a multiple of 256 and sequences of ``REG_T`` frames: the case with the regressor
on has those.  Everything here uses only names of the package that a refactor keeps.
"""
import copy
import hashlib
import os

import torch

from behavior_driven_video_synthesis_amd import _lib, ops
from fused_conv_cases import _Proxy, tensor_bytes

DEV = "cuda:0"
C, MID, DEPTH, BLOCKS = 7, 64, 1, 2
H, N, T = 64, 6, 3

# entry points the recorded traces must contain between them (checked when the fixture is recorded), and a second stream
REQUIRED = ("vunet_seq_coupling", "vunet_seq_actnorm_init", "vunet_seq_lstm_gates_tiled", "vunet_seq_lstm_gates_tiled_h",
            "vunet_seq_decoder_out", "vunet_seq_start", "vunet_seq_bottleneck", "vunet_seq_coupling_bwd", "vunet_seq_dx",
            "vunet_seq_dx_finish", "vunet_seq_dwx", "vunet_seq_dz_finish", "vunet_seq_dw", "vunet_seq_actnorm_bwd", "vunet_seq_cell_bwd",
            "vunet_seq_bottleneck_bwd", "vunet_seq_flow_loss")


def _r(seed, *shape, scale=1.0):
    return (scale * torch.randn(*shape, generator=torch.Generator().manual_seed(seed))).to(DEV)


def _flow(fresh=False):
    from behavior_driven_video_synthesis_amd.models.flow.simple_flow import UnsupervisedTransformer2
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(4321)
        flow = UnsupervisedTransformer2(flow_in_channels=C, flow_mid_channels=MID, flow_hidden_depth=DEPTH, n_flows=BLOCKS)
        if not fresh:
            for blk in flow.flow.sub_layers:
                blk.norm_layer.loc.data.normal_(0.0, 0.2)
                blk.norm_layer.scale.data.uniform_(0.7, 1.3)
                blk.norm_layer.initialized.fill_(1)
    return flow.to(DEV)


def _net():
    from behavior_driven_video_synthesis_amd.models.pose_behavior_rnn import ResidualBehaviorNet
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(8765)
        net = ResidualBehaviorNet(N, information_bottleneck=True, decoder_arch="lstm", dim_hidden_b=H)
    return net.to(DEV)


def _params(prefix, module):
    return {f"{prefix}{n}": q.detach() for n, q in module.named_parameters()}


def _grads(prefix, module):
    return {f"{prefix}{n}": q.grad for n, q in module.named_parameters()}


# ---- the flow ----------------------------------------------------------------------------------------------------------
def flow_inference(weights):
    flow = _flow()
    flow.set_weight_precision(weights)
    flow.flow.engine().graph.enabled = False
    with torch.no_grad():
        z, logdet = flow(_r(1, 3, C))
        x = flow.reverse(_r(2, 3, C))
    return {"z": z, "logdet": logdet, "x": x}


def flow_first_forward():
    """The first forward of a fresh flow: ActNorm initialises itself block by block from the batch."""
    flow = _flow(fresh=True)
    flow.flow.engine().graph.enabled = False
    with torch.no_grad():
        z, logdet = flow(_r(3, 2, C))
        z2, logdet2 = flow(_r(4, 3, C))     # ... and the walk of an initialised flow on what that left
    return {"z": z, "logdet": logdet, "z2": z2, "logdet2": logdet2, **_params("", flow)}


def flow_train(fresh=False, **switches):
    """Two fused steps, then a pass under autograd on the updated weights, with ``switches`` set on the train engine."""
    flow = _flow(fresh)
    eng = flow.flow.train_engine(lr=1e-3, betas=(0.5, 0.9), weight_decay=1e-3)
    eng.graph.enabled = False
    for k, v in switches.items():
        assert hasattr(eng, k), k
        setattr(eng, k, v)
    out = {}
    for it in range(2):
        out[f"log{it}"] = eng.train_step(_r(10 + it, 3, C), _r(20 + it, 3, C)).clone()
    out.update(_params("after.", flow))
    x = _r(30, 3, C).requires_grad_(True)
    z, logdet = flow(x)
    ((z * _r(31, *z.shape)).sum() + (logdet * _r(32, *logdet.shape)).sum()).backward()
    out.update(z=z, logdet=logdet, dx=x.grad, **_grads("d.", flow))
    return out


def flow_autograd(max_passes):
    """``max_passes`` forward passes alive at once, each in a plan of its own; the first one's backward runs twice."""
    flow = _flow()
    eng = flow.flow.train_engine()
    eng.max_passes = max_passes
    out, alive = {}, []
    for i in range(max_passes):
        x = _r(40 + i, 3, C).requires_grad_(True)       # (one batch size: the second pass takes slot 1)
        z, logdet = flow(x)
        alive.append((x, z, logdet))
    for i, (x, z, logdet) in enumerate(alive):
        loss = (z * _r(50 + i, *z.shape)).sum() - logdet.mean()
        for run in range(2 if i == 0 else 1):
            flow.zero_grad(set_to_none=True)
            x.grad = None
            loss.backward(retain_graph=True)
            out.update({f"p{i}.r{run}.z": z, f"p{i}.r{run}.logdet": logdet, f"p{i}.r{run}.dx": x.grad}, **_grads(f"p{i}.r{run}.d.", flow))
    return out


# ---- the behaviour net -------------------------------------------------------------------------------------------------
def behavior_inference(rows, tiled_h=True):
    saved = os.environ.get("VUNET_SEQ_LSTM_TILED_H")
    try:
        if not tiled_h:
            os.environ["VUNET_SEQ_LSTM_TILED_H"] = "0"
        net = _net()
        net.engine().graph.enabled = False
        seq, eps = _r(60, rows, T, N, scale=0.5), _r(61, rows, H)
        with torch.no_grad():
            b, mu, logstd, pre = net.engine().infer_b(seq, eps)
            b0, mu0, logstd0, pre0 = net.engine().infer_b(seq, None)
            xs, cs = net.engine().generate_seq(b, seq, T, 1)
        return {"b": b, "mu": mu, "logstd": logstd, "pre": pre, "b0": b0, "mu0": mu0, "logstd0": logstd0, "pre0": pre0, "xs": xs, "cs": cs}
    finally:
        if saved is None:
            os.environ.pop("VUNET_SEQ_LSTM_TILED_H", None)
        else:
            os.environ["VUNET_SEQ_LSTM_TILED_H"] = saved


def behavior_autograd(rows, sample_prior=False, heads_only=False, tile_h=True):
    """``heads_only``: the loss sees mu and logstd alone -- nothing reaches the roll-out (the backward's ``decoder=False``)."""
    net = _net().train()
    net.train_engine().tile_h = tile_h
    x1, x2, eps = _r(70, rows, T, N, scale=0.5), _r(71, rows, T + 1, N, scale=0.5), _r(72, rows, H)
    xs, cs, _, b, mu, logstd, pre = net(x1, x2, T, start_frame=1, sample=sample_prior, eps=eps)
    outs = dict(mu=mu, logstd=logstd) if heads_only else dict(xs=xs, cs=cs, b=b, mu=mu, logstd=logstd, pre=pre)
    sum((t * _r(80 + i, *t.shape)).sum() for i, t in enumerate(outs.values())).backward()
    return dict(xs=xs, cs=cs, b=b, mu=mu, logstd=logstd, pre=pre, **_grads("d.", net))


def cvae_step(regressor=False, update=True, cvae=False):
    """Two fused steps through ``BehaviorNet.train_fn`` (issued eagerly: ``hip_graph`` False)."""
    from behavior_driven_video_synthesis_amd.experiments.behavior_net import BehaviorNet, DEFAULT_CONFIG
    from behavior_driven_video_synthesis_amd.seq_train import REG_T
    hid, t_len, rows = (256, REG_T, 3) if regressor else (H, T, 3)
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["architecture"].update(dim_hidden_b=hid, n_flows=1, flow_mid_channels_factor=1, flow_hidden_depth=1, cvae=cvae)
    cfg["training"].update(batch_size=rows, lr_init=1e-3, gamma_init=0.05, gamma_step=1e-3, information_max=5, use_regressor=regressor)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(2468)
        tr = BehaviorNet(cfg, n_kps=N, device=DEV, hip_graph=False)
    out = {}
    for it in range(2):
        log = tr.train_fn({"keypoints": _r(90 + it, rows, t_len + 1, N, scale=0.5)}, eps=_r(95 + it, rows, hid), sync=False, update=update,
                          reg_index=[(7 * it + 11 * k) % t_len for k in range(5)] if regressor else None)
        out.update({f"s{it}.{k}": v.clone() for k, v in log.items() if isinstance(v, torch.Tensor)})
    out.update(_params("after.", tr.net))
    if regressor:
        out.update(_params("after.reg.", tr.regressor))
    return out


CASES = {
    "flow_f32": lambda: flow_inference("f32"),
    "flow_bf16": lambda: flow_inference("bf16"),
    "flow_first_forward": flow_first_forward,
    "flow_train_defaults": flow_train,
    "flow_train_fresh": lambda: flow_train(fresh=True),
    "flow_train_two_streams": lambda: flow_train(two_streams=True),
    "flow_train_fused_dx": lambda: flow_train(fused_dx=True),
    "flow_train_fused_finish": lambda: flow_train(fused_finish=True),
    "flow_train_rowmajor_activations": lambda: flow_train(tile_activations=False),
    "flow_autograd_one_pass": lambda: flow_autograd(1),
    "flow_autograd_two_passes": lambda: flow_autograd(2),
    "behavior_inference_3": lambda: behavior_inference(3),
    "behavior_inference_48": lambda: behavior_inference(48),
    "behavior_inference_48_rows_only": lambda: behavior_inference(48, tiled_h=False),
    "behavior_autograd_3": lambda: behavior_autograd(3),
    "behavior_autograd_48": lambda: behavior_autograd(48),
    "behavior_autograd_48_rows_only": lambda: behavior_autograd(48, tile_h=False),
    "behavior_autograd_prior_3": lambda: behavior_autograd(3, sample_prior=True),
    "behavior_autograd_prior_48": lambda: behavior_autograd(48, sample_prior=True),
    "behavior_autograd_heads_only_3": lambda: behavior_autograd(3, heads_only=True),
    "behavior_autograd_heads_only_48": lambda: behavior_autograd(48, heads_only=True),
    "cvae_step": cvae_step,
    "cvae_step_frozen": lambda: cvae_step(update=False),
    "cvae_step_regressor": lambda: cvae_step(regressor=True, cvae=True),
    "cvae_step_regressor_frozen": lambda: cvae_step(regressor=True, update=False),
}


def record_case(name):
    """Run case ``name`` once under the logging proxy -> ({"trace", "sha256", "absent", "profile"}, {tensor name: bytes});
    ``profile`` is always None here (the key is what tools/fused_conv_trace.py merges and compares)."""
    lib, log = _lib.lib(), []
    torch.cuda.synchronize()
    try:
        _lib._LIB = _Proxy(lib, log, ops._stream().value or 0)
        tensors = CASES[name]()
        torch.cuda.synchronize()
    finally:
        _lib._LIB = lib
    raw = {k: tensor_bytes(t) for k, t in tensors.items() if t is not None}
    absent = sorted(k for k, t in tensors.items() if t is None)
    return ({"trace": log, "sha256": {k: hashlib.sha256(b).hexdigest() for k, b in raw.items()}, "absent": absent, "profile": None}, raw)


def missing_coverage(records):
    """REQUIRED entry points that no recorded trace contains (each with return code 0), and ["stream", 1] if no call of any
    trace went to a second stream (``two_streams``)."""
    seen = {(n, rc) for r in records.values() for n, _, rc in r["trace"]}
    missing = sorted([n, 0] for n in REQUIRED if (n, 0) not in seen)
    if not any(s == 1 for r in records.values() for _, s, _ in r["trace"]):
        missing.append(["stream", 1])
    return missing
