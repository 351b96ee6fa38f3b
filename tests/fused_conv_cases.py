"""Small cases that between them reach every host branch of ``ops.FusedConv`` and of the deferred weight-gradient queue,
and a recorder for them.  Used by tools/fused_conv_trace.py (which records tests/fused_conv_trace.json from the PARENT of
a host-side refactor) and by tests/test_hip_fused_conv_modes.py (which replays the cases on the tree under test).

A record holds, per case: the trace of native calls ([entry point, stream ordinal, return code]; stream 0 is the caller's,
1 the first other one seen, ...; None: the entry point takes no stream), the SHA-256 of every output, input gradient and
parameter gradient, and -- for cases run under ``ops.profile_start()`` -- the (key, flop, n) triples of
``profile_stop(detail=True)``.  Pure queries (names ending _supported, _nsplit, _variant, _batchable) are left out of the
trace: their caching is free to change.  Everything here uses only public names of the package that a refactor keeps.
"""
import hashlib
import re

import torch

from behavior_driven_video_synthesis_amd import _lib, ops, optim
from behavior_driven_video_synthesis_amd.lib.modules import Conv2d, NormConv2d

QUERY_SUFFIXES = ("_supported", "_nsplit", "_variant", "_batchable")
DEV = "cuda:0"

# entry point -> return codes the recorded traces must contain between them (checked when the fixture is recorded).
# The fused ReLU data gradient's fallback: the host asks the router (vunet_conv2d_wants_split) before it calls
# vunet_conv2d_dgrad_relu_x6, and that entry point refuses exactly what the same router refuses, so from FusedConv it
# cannot return -3; the -3 that takes the two-pass route (and drops the profiler record) comes from vunet_conv2d_dgrad_relu.
REQUIRED = {"vunet_conv2d_a2": (0,), "vunet_conv2d_bf16": (0,), "vunet_pack_bf16": (0,), "vunet_conv2d_dgrad_relu_x6": (0,),
            "vunet_conv2d_dgrad_relu": (0, -3), "vunet_act_bwd_from_out": (0,), "vunet_space_to_depth": (0,),
            "vunet_conv2d_wgrad_a2": (0,), "vunet_conv2d_wgrad_multi": (0,), "vunet_weightnorm_bwd": (0,),
            "vunet_weightnorm_bwd_multi": (0,), "vunet_weightnorm_fwd_multi": (0,)}


def _stream_args():
    """entry point -> index of its ``stream`` argument (parsed from the C headers)."""
    out = {}
    for m in re.finditer(r"\bint\s+(vunet_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", _lib._header_text(), flags=re.S):
        names = [a.split()[-1].lstrip("*") for a in m.group(2).split(",") if a.strip() and a.strip() != "void"]
        if "stream" in names:
            out[m.group(1)] = names.index("stream")
    return out


class _Proxy:
    """Forwards every attribute to the loaded library; calls of non-query entry points are logged."""

    def __init__(self, lib, log, home_stream):
        self._lib, self._log, self._streams, self._where = lib, log, {home_stream: 0}, _stream_args()

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("vunet_") or name.endswith(QUERY_SUFFIXES):
            return fn
        idx = self._where.get(name)

        def call(*args):
            rc = fn(*args)
            stream = None
            if idx is not None:
                raw = getattr(args[idx], "value", args[idx]) or 0
                stream = self._streams.setdefault(raw, len(self._streams))
            self._log.append([name, stream, rc])
            return rc
        return call


def _x(seed, *shape, grad=True):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(DEV).requires_grad_(grad)


def _modules(build):
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(1234)
        return build().to(DEV)


def _named(prefix, mods):
    return {f"{prefix}{i}.{n}": p for i, m in enumerate(mods) for n, p in m.named_parameters()}


def _finish(outs, ins, params, direct=False):
    """Backward from fixed output gradients, then every tensor of interest by name."""
    for p in params.values():
        if not getattr(p, "_vunet_direct_grad", False):
            p.grad = None
    torch.autograd.backward(list(outs), [_x(90 + i, *o.shape, grad=False) for i, o in enumerate(outs)])
    if direct:
        ops.join_wgrad_streams()
    res = {f"y{i}": o for i, o in enumerate(outs)}
    res.update({f"d{n}": t.grad for n, t in ins.items()})
    res.update({f"d{n}": p.grad for n, p in params.items()})
    return res


# ---- the cases: each builds its modules once and returns the step that is run twice (warm-up, then recorded) -------------
def two_sources():
    """Two sources + ELU + dropout + the residual is source 1; parameter gradients returned to autograd."""
    conv = _modules(lambda: NormConv2d(64, 32, 3, 1, 1))

    def step():
        x1, x2 = _x(1, 2, 32, 32, 32), _x(2, 2, 32, 32, 32)
        y = conv.fused((x1, x2), res=x1, in_act=ops.ACT_ELU, drop_p=0.1)
        return _finish([y], {"x1": x1, "x2": x2}, _named("c", [conv]))
    return step


def d2s_sigmoid():
    conv = _modules(lambda: NormConv2d(32, 64, 3, 1, 1))

    def step():
        x = _x(3, 2, 32, 16, 16)
        return _finish([conv.fused(x, in_act=ops.ACT_ELU, out_act=ops.ACT_SIGMOID, d2s=True)], {"x": x}, _named("c", [conv]))
    return step


def stride2_and_1x1():
    mods = _modules(lambda: torch.nn.ModuleList([NormConv2d(32, 64, 3, 2, 1), NormConv2d(64, 32, 1)]))

    def step():
        x = _x(4, 2, 32, 32, 32)
        h = mods[0].fused(x, in_act=ops.ACT_ELU, drop_p=0.1)
        return _finish([mods[1].fused(h, out_act=ops.ACT_LRELU, in_slope=0.2)], {"x": x}, _named("c", mods))
    return step


def conv1_1_like():
    conv = _modules(lambda: NormConv2d(3, 32, 3, 1, 1))

    def step():
        x = _x(5, 2, 3, 32, 32)
        return _finish([conv.fused(x)], {"x": x}, _named("c", [conv]))
    return step


def _passthrough(use_y, res_is_x):
    conv = _modules(lambda: NormConv2d(32, 32, 3, 1, 1))

    def step():
        x = _x(6, 2, 32, 32, 32)
        y, alias = conv.fused(x, res=x if res_is_x else None, in_act=ops.ACT_ELU, passthrough=True)
        return _finish([y, alias * 2.0] if use_y else [alias * 2.0], {"x": x}, _named("c", [conv]) if use_y else {})
    return step


def _frozen_stack(n, c_in, c, size, last_plain):
    """A frozen ReLU stack (VGG-like): the fused ReLU data gradient and its fallback; with a last layer without activation
    the layer below gets its gradient masked by the producer (premask) and runs the plain data gradient."""
    def build():
        m = torch.nn.ModuleList([Conv2d(c_in, c, 3, 1, 1), Conv2d(c, c, 3, 1, 1)] + ([Conv2d(c, c, 3, 1, 1)] if last_plain else []))
        return m.requires_grad_(False)
    mods = _modules(build)

    def step():
        x = _x(7, n, c_in, size, size)
        h = x
        for i, m in enumerate(mods):
            h = m.fused(h, out_act=ops.ACT_NONE if (last_plain and i == 2) else ops.ACT_RELU)
        return _finish([h], {"x": x}, {})
    return step


def double_backward():
    conv = _modules(lambda: NormConv2d(32, 32, 3, 1, 1))

    def step():
        x = _x(8, 2, 32, 16, 16)
        y = conv.fused(x, in_act=ops.ACT_LRELU, in_slope=0.2)
        gx, = torch.autograd.grad(y, x, _x(91, *y.shape, grad=False), create_graph=True)
        return _finish([gx], {"x": x}, _named("c", [conv]))
    return step


def _bucketed(batching=True, late=True, streams=False, prepack=True, partial=False):
    """Three layers whose parameter gradients are views of a flat bucket (``partial``: gamma and beta are not): immediate,
    deferred (with the short launches deferred too, or not) and companion-stream weight gradients."""
    mods = _modules(lambda: torch.nn.ModuleList([NormConv2d(32, 32, 3, 1, 1), NormConv2d(32, 64, 3, 2, 1), NormConv2d(64, 32, 1)]))
    names = _named("c", mods)
    bucket = optim.FlatBucket([p for n, p in names.items() if not (partial and n.endswith(("gamma", "beta")))])

    def forward(x):
        h = mods[0].fused(x, in_act=ops.ACT_ELU, drop_p=0.1)
        return mods[2].fused(mods[1].fused(h, in_act=ops.ACT_ELU), in_act=ops.ACT_ELU)
    forward(_x(9, 2, 32, 32, 32))   # the layers have been seen: ops.prepacked packs them from now on

    def step():
        saved = ops._wn_batch["on"], ops._wn_batch["wgrad"], ops._wgrad_streams["on"]
        try:
            ops.enable_wn_batching(batching)
            ops._wn_batch["wgrad"] = late
            ops.enable_wgrad_streams(streams)
            bucket.zero_grad()
            x = _x(9, 2, 32, 32, 32)
            if prepack:
                with ops.prepacked(mods):
                    return _finish([forward(x)], {"x": x}, names, direct=True)
            return _finish([forward(x)], {"x": x}, names, direct=True)
        finally:
            ops.join_wgrad_streams()
            ops.enable_wn_batching(saved[0])
            ops._wn_batch["wgrad"] = saved[1]
            ops.enable_wgrad_streams(saved[2])
    return step


def bf16_inference():
    conv = _modules(lambda: NormConv2d(64, 32, 3, 1, 1))

    def step():
        with torch.no_grad(), ops.inference_precision("bf16"):
            x1, x2 = _x(10, 2, 32, 32, 32, grad=False), _x(11, 2, 32, 32, 32, grad=False)
            return {"y0": conv.fused((x1, x2), res=x1, in_act=ops.ACT_ELU)}
    return step


# name -> (builder, conv scheme, profiled)
CASES = {
    "two_sources_h2": (two_sources, "h2", True),
    "two_sources_x6": (two_sources, "x6", True),
    "two_sources_f32": (two_sources, "f32", True),
    "d2s_sigmoid": (d2s_sigmoid, "h2", False),
    "stride2_and_1x1": (stride2_and_1x1, "h2", True),
    "conv1_1_like": (conv1_1_like, "h2", False),
    "passthrough_both": (lambda: _passthrough(True, False), "h2", False),
    "passthrough_both_residual": (lambda: _passthrough(True, True), "h2", False),
    "passthrough_alias_only": (lambda: _passthrough(False, False), "h2", False),
    "frozen_relu_fallback": (lambda: _frozen_stack(2, 3, 64, 32, False), "h2", True),
    "frozen_relu_premask": (lambda: _frozen_stack(2, 3, 64, 32, True), "h2", False),
    "frozen_relu_split_h2": (lambda: _frozen_stack(4, 32, 32, 64, False), "h2", True),   # (128 tiles: the split kernels' minimum)
    "frozen_relu_split_x6": (lambda: _frozen_stack(4, 32, 32, 64, False), "x6", False),
    "frozen_relu_tiled_f32": (lambda: _frozen_stack(4, 32, 32, 64, False), "f32", True),   # (no split image: the fp32 fused kernel)
    "double_backward": (double_backward, "h2", False),
    "direct_no_batching": (lambda: _bucketed(batching=False), "h2", False),
    "direct_not_prepacked": (lambda: _bucketed(prepack=False), "h2", False),
    "deferred_late": (lambda: _bucketed(), "h2", False),
    "deferred_late_profiled": (lambda: _bucketed(), "h2", True),
    "deferred_no_late": (lambda: _bucketed(late=False), "h2", False),
    "mixed_direct": (lambda: _bucketed(partial=True), "h2", False),
    "companion_deferred": (lambda: _bucketed(streams=True), "h2", False),
    "companion_immediate": (lambda: _bucketed(streams=True, batching=False), "x6", False),
    "bf16_inference": (bf16_inference, "h2", False),
}


def tensor_bytes(t):
    return t.detach().to("cpu", torch.float32).contiguous().numpy().tobytes()


def record_case(name):
    """Run case ``name`` twice and record the second run -> ({"trace", "sha256", "profile"}, {tensor name: bytes})."""
    build, scheme, profiled = CASES[name]
    saved_scheme, saved_drop, lib = ops.conv_precision(), dict(ops._drop_state), _lib.lib()
    log, prof = [], None
    try:
        ops.set_conv_precision(scheme)
        ops.set_dropout_seed(7)
        step = build()
        ops.set_dropout_seed(7)
        step()
        torch.cuda.synchronize()
        ops.set_dropout_seed(7)
        _lib._LIB = _Proxy(lib, log, ops._stream().value or 0)
        if profiled:
            ops.profile_start()
        tensors = step()
        if profiled:
            prof = [[list(k), v["flop"], v["n"]] for k, v in ops.profile_stop(detail=True).items()]
        torch.cuda.synchronize()
    finally:
        _lib._LIB = lib
        ops._prof["on"] = False
        ops.set_conv_precision(saved_scheme)
        ops._drop_state.update(saved_drop)
    raw = {k: tensor_bytes(t) for k, t in tensors.items() if t is not None}
    absent = sorted(k for k, t in tensors.items() if t is None)
    return ({"trace": log, "sha256": {k: hashlib.sha256(b).hexdigest() for k, b in raw.items()}, "absent": absent,
             "profile": prof}, raw)


def missing_coverage(records):
    """REQUIRED (entry point, return code) pairs that no recorded trace contains."""
    seen = {(n, rc) for r in records.values() for n, _, rc in r["trace"]}
    return sorted((n, rc) for n, rcs in REQUIRED.items() for rc in rcs if (n, rc) not in seen)
