"""Training plans of the behaviour path (BASELINE config 4; csrc/seq_train.hip, include/vunet_seq_train.h).

The flow stage of ``experiments/behavior_net.py`` (:703-714) is, per step,

    gauss, logdet = latent_flow(bs.detach());  f_loss, log = flow_loss(gauss, logdet)
    flow_optimizer.zero_grad();  f_loss.backward();  flow_optimizer.step()

with ``Adam(lr = flow_lr * batch_size, betas = (0.5, 0.9), weight_decay)`` (:384-395) and ``FlowLoss`` (lib/losses.py:294-317).
``FlowTrainEngine`` runs that step on the kernels of csrc/seq.hip (forward, every layer's output kept) and csrc/seq_train.hip
(loss, input gradients, and the weight gradient fused into Adam's update: dW is never written), recorded once per batch size
into a hipGraph.  The same backward kernels serve autograd (``flow_autograd``): there the gradients are written out and the
reference's own ``torch.optim.Adam`` applies them -- what an unchanged ``main.py`` does through ``dropin``.

There is no CPU path.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, List, Optional

import torch

from . import _lib
from .ops import _call, _p, _stream, _versions, mark_written
from .seq import (ACT_LRELU, BF16_INFERENCE_ONLY, FlowEngine, SeqCouplingDesc, _need_device, _up, padded_vector,  # noqa: F401
                  weight_image)
from .seq_passes import KeepsPasses, PassPool

LRELU_SLOPE = 0.01   # nn.LeakyReLU() default (lib/modules.py:244)

STALE_WEIGHTS = ("the {}'s parameters were modified between this pass's forward and its backward (an optimiser step, a "
                 "load_state_dict, an in-place operation): its saved activations belong to the weights before.  Run the backward "
                 "before the step, or run the forward again")


SeqAdamHp = _lib.struct("vunet_seq_adam_hp")
SeqDxDesc = _lib.struct("vunet_seq_dx_desc")
SeqCouplingBwdDesc = _lib.struct("vunet_seq_coupling_bwd_desc")
SeqDwLayer = _lib.struct("vunet_seq_dw_layer")             # (uploaded as a device table, as SeqActnormLayer)
SeqActnormLayer = _lib.struct("vunet_seq_actnorm_layer")
SeqCellBwdDesc = _lib.struct("vunet_seq_cell_bwd_desc")


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _table(entries, device) -> torch.Tensor:
    """A ctypes array of descriptors -> a device byte tensor (the kernels read their descriptors from device memory)."""
    arr = (type(entries[0]) * len(entries))(*entries)
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)


class AdamState:
    """torch.optim.Adam's hyper-parameters with the learning rate (float64) and the step count (int64) on the device."""

    def __init__(self, device, lr: float, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0):
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.lr_dev = torch.full((1,), self.lr, dtype=torch.float64, device=device)
        self.step_dev = torch.zeros(1, dtype=torch.int64, device=device)
        self.resolved_dev = torch.zeros(2, dtype=torch.float32, device=device)    # written by tick(), read by the step's kernels
        self.hp = SeqAdamHp(self.lr_dev.data_ptr(), self.step_dev.data_ptr(), self.betas[0], self.betas[1], self.eps, self.weight_decay,
                            self.resolved_dev.data_ptr())

    def set_lr(self, lr: float):
        if float(lr) != self.lr:
            self.lr = float(lr)
            self.lr_dev.fill_(self.lr)

    def set_hyper(self, betas, eps: float, weight_decay: float):
        """The launch arguments among the hyper-parameters: a recorded step holds the old ones (the caller forgets it)."""
        self.betas, self.eps, self.weight_decay = (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.hp.beta1, self.hp.beta2, self.hp.eps, self.hp.weight_decay = self.betas[0], self.betas[1], self.eps, self.weight_decay

    def tick(self):
        _call("vunet_seq_adam_tick", _p(self.step_dev), _p(self.lr_dev), self.hp.beta1, self.hp.beta2, _p(self.resolved_dev), _stream())

    @property
    def step(self) -> int:
        return int(self.step_dev.item())


def adam_state_dict(adam, step: int, moments, **group_extra) -> dict:
    """``torch.optim.Adam(...).state_dict()`` as the installed torch writes it, for the parameters whose (exp_avg, exp_avg_sq)
    ``moments`` lists in order: one float ``step`` tensor per entry, the group's full key set (+ ``group_extra``), and -- as
    torch's -- no state at all before the first step.  ``adam``: lr, betas, eps, weight_decay as plain attributes."""
    group = torch.optim.Adam([torch.zeros(1)], lr=adam.lr, betas=adam.betas, eps=adam.eps,
                             weight_decay=adam.weight_decay).state_dict()["param_groups"][0]
    group.update(group_extra, params=list(range(len(moments))))
    state = {i: {"step": torch.tensor(float(step)), "exp_avg": m, "exp_avg_sq": v} for i, (m, v) in enumerate(moments)} if step else {}
    return {"state": state, "param_groups": [group]}


def load_adam_state(adam, sd: dict):
    """The inverse: ``adam`` takes the group's hyper-parameters; -> ([(exp_avg, exp_avg_sq) or None per parameter], step)."""
    group = sd["param_groups"][0]
    adam.set_lr(group["lr"])
    adam.set_hyper(group["betas"], group["eps"], group["weight_decay"])
    states = [sd["state"].get(i) for i in range(len(group["params"]))]
    step = 0
    for st in states:
        if st is not None:
            step = int(st["step"])
    return [None if st is None else (st["exp_avg"], st["exp_avg_sq"]) for st in states], step


def dx_split(m: int, k: int, nets: int) -> int:
    """Row ranges (slabs) of W per input-gradient launch: as many as keep the launch within ONE round of workgroups on the
    chip's 256 CUs and a slab at >= 64 rows, at most 16 -- 4 for the flow's 2048 x 2048 layers (64 stripes), 16 for its first
    layers, 15 for the LSTM's gate matrix over [x | h] (17 stripes: 255 workgroups; slabs of 17 or 18 row groups)."""
    wgs = (k // 64) * nets
    if os.environ.get("VUNET_SEQ_DX_TAIL", "0") == "1":    # the rule before: doubled until >= 256 workgroups (17 stripes: 272)
        s = 1
        while wgs * s < 256 and m % (32 * s) == 0 and m // (2 * s) >= 64 and s < 16:
            s *= 2
        return s
    return max(1, min(16, 256 // wgs, m // 64))


def dx_chain(d: SeqDxDesc, w, dz: torch.Tensor, raw: torch.Tensor, below=None, slope: float = 0.0):
    """One layer of an input-gradient chain: ``vunet_seq_dx`` of the layer's dZ through ``w`` (one image per net) into the raw
    slabs and, with a layer ``below`` = (its output, its dZ), ``vunet_seq_dz_finish``: the slab sum times the derivative of the
    activation between them (LeakyReLU of ``slope``; 0: ReLU)."""
    _call("vunet_seq_dx", ctypes.byref(d), _p(w[0]), _p(w[1] if d.nets > 1 else None), _p(dz), _p(raw), _stream())
    if below is not None:
        _call("vunet_seq_dz_finish", _p(raw), _p(below[0]), _p(below[1]), d.nets, d.S, _up(d.B, 16), d.K, slope, _stream())


class TrainLayer:
    """One trainable (weight, bias) pair of the seq kernels: the operand images they read, Adam's moments beside them and the
    layer's entry of the update sweep's table.

    The images are [mp, kp] / [mp], multiples of 64.  A parameter whose 2-D view [out, in k k] fits and is contiguous IS its image
    and is updated in place; any other trains as a zero-padded image (padded rows produce zeros and receive no update) that
    ``write_back`` copies into the parameter.  Either way the write goes through a raw pointer: ``write_back`` announces its
    own (``ops.mark_written``), and the engine that launches the update sweep announces ``inplace_params()`` after it.
    ``pieces``: (first column of the parameter's matrix, columns, first column in the image) per column block of a padded image.  ``images``: a (weight, bias) image pair the caller already holds -- nothing is
    allocated or loaded here.  The moments ``m, v, bm, bv`` are shaped like the images and allocated on first use."""

    def __init__(self, name: str, weight: torch.Tensor, bias: torch.Tensor, pieces=None, kp: Optional[int] = None, images=None):
        w2 = weight.data.reshape(weight.shape[0], -1)
        self.name, self.weight, self.bias = name, weight, bias
        self.rows, self.k = w2.shape                       # (``m`` is Adam's first moment)
        self.pieces = [(0, self.k, 0)] if pieces is None else list(pieces)
        own = images is None
        if own:
            mp, kp = _up(self.rows, 64), _up(self.k, 64) if kp is None else kp
            fits = (mp, kp) == (self.rows, self.k) and w2.is_contiguous() and bias.data.is_contiguous()
            images = (w2, bias.data) if fits else (torch.zeros(mp, kp, device=weight.device), torch.zeros(mp, device=weight.device))
        self.w, self.b = images
        self.mp, self.kp = self.w.shape
        self.w_inplace, self.b_inplace = self.w.data_ptr() == weight.data_ptr(), self.b.data_ptr() == bias.data_ptr()
        self.m = self.v = self.bm = self.bv = None
        if own:
            self.load()

    @property
    def inplace(self) -> bool:
        return self.w_inplace and self.b_inplace

    def inplace_params(self) -> list:
        """The module tensors the update sweep itself writes: those that are their own image."""
        return [t for t, hit in ((self.weight, self.w_inplace), (self.bias, self.b_inplace)) if hit]

    def load(self):
        """The parameter's values -> the padded images."""
        if not self.w_inplace:
            self._scatter(self.w, self.weight.data)
        if not self.b_inplace:
            self.b[:self.rows].copy_(self.bias.data)

    def write_back(self):
        """A padded image is the training master: copy its valid part into the module's parameter."""
        if not self.w_inplace:
            if self.pieces == [(0, self.k, 0)] and self.weight.data.is_contiguous():
                _call("vunet_seq_unpack_rows", _p(self.w), self.kp, 0, 0, 1, _p(self.weight.data), self.rows, self.k, 0, _stream())
            else:
                self.weight.data.copy_(self._gather(self.w))
        if not self.b_inplace:
            _call("vunet_seq_unpack_rows", _p(self.b), self.mp, 0, 0, 1, _p(self.bias.data), 1, self.rows, 0, _stream())
        mark_written([t for t, hit in ((self.weight, self.w_inplace), (self.bias, self.b_inplace)) if not hit])

    def _gather(self, img: Optional[torch.Tensor]) -> torch.Tensor:
        """An image's valid part in the weight's own shape, as a copy (no image: zeros)."""
        out = torch.zeros(self.rows, self.k, device=self.w.device)
        if img is not None:
            for src, n, dst in self.pieces:
                out[:, src:src + n].copy_(img[:self.rows, dst:dst + n])
        return out.reshape(self.weight.shape)

    def _scatter(self, img: torch.Tensor, val: torch.Tensor):
        v2 = val.to(img.device, torch.float32).reshape(self.rows, self.k)
        for src, n, dst in self.pieces:
            img[:self.rows, dst:dst + n].copy_(v2[:, src:src + n])

    def ensure_moments(self):
        if self.m is None:
            self.m, self.v = torch.zeros_like(self.w), torch.zeros_like(self.w)
            self.bm, self.bv = torch.zeros_like(self.b), torch.zeros_like(self.b)

    def adopt_moments(self, other: "TrainLayer"):
        """Adam's moments survive a re-pack (a load_state_dict between two steps) as long as the image's shape does."""
        if other.m is not None and other.m.shape == self.w.shape:
            self.m, self.v, self.bm, self.bv = other.m, other.v, other.bm, other.bv

    def moments(self):
        """-> [(exp_avg, exp_avg_sq) of the weight, of the bias] in the parameters' own shapes, as copies (zeros before the
        first step: nothing is allocated for them)."""
        bias = [torch.zeros(self.rows, device=self.w.device) if t is None else t[:self.rows].clone() for t in (self.bm, self.bv)]
        return [(self._gather(self.m), self._gather(self.v)), tuple(bias)]

    def set_moments(self, w_state, b_state):
        """The inverse of ``moments``: (exp_avg, exp_avg_sq) of the weight and of the bias; None (a parameter without state, as
        in torch's dictionary before the first step): zeros."""
        if w_state is None and b_state is None and self.m is None:
            return
        self.ensure_moments()
        for img in (self.m, self.v, self.bm, self.bv):
            img.zero_()
        for img, val in zip((self.m, self.v), w_state or ()):
            self._scatter(img, val)
        for img, val in zip((self.bm, self.bv), b_state or ()):
            img[:self.rows].copy_(val.reshape(-1))

    def tiles(self, nchunk: int = 1) -> int:
        """64 x 64 tiles of the layer's entry in the sweep's table; ``nchunk`` > 1 (``vunet_seq_dwx``): tiles of 64 nchunk rows."""
        return -(-self.mp // (64 * nchunk)) * (self.kp // 64)

    def dw_entry(self, dz_ptr: int, ldz: int, x_ptr: int, ldx: int, tile0: int, *, grads=None, kv: Optional[int] = None,
                 nchunk: int = 1, dx_raw: Optional[int] = None) -> SeqDwLayer:
        """The layer's entry of a ``vunet_seq_dw`` / ``vunet_seq_dwx`` table (include/vunet_seq_train.h).  ``grads`` = (g, bg):
        write mode, the gradients go there and nothing is updated; None: the update fused into Adam, on the layer's moments
        (allocated here if they are not yet).  ``kv``: valid columns (default: all of the image's); ``nchunk``, ``dx_raw``:
        ``vunet_seq_dwx``'s rows per tile (in 64s) and its slabs."""
        if grads is None:
            self.ensure_moments()
        g, bg = grads if grads is not None else (None, None)
        return SeqDwLayer(w=_ptr(self.w), m=_ptr(self.m), v=_ptr(self.v), g=_ptr(g), bias=_ptr(self.b), bm=_ptr(self.bm),
                          bv=_ptr(self.bv), bg=_ptr(bg), dz=dz_ptr, x=x_ptr, M=self.mp, K=self.kp, ldz=ldz, ldx=ldx, tile0=tile0,
                          tiles_k=self.kp // 64, kv=self.kp if kv is None else kv, nchunk=nchunk, chunk_z=0, chunk_x=0, dx_raw=dx_raw)


class FlowTrainEngine(KeepsPasses, FlowEngine):
    """``UnconditionalFlow2`` forward with every intermediate kept, ``FlowLoss``, the backward pass and Adam, for one batch of
    <= 64 rows (``config/behavior_net.yaml``: batch_size 64).  Widths are padded to 64 (the tiles of the backward kernels); a
    parameter whose shape already fits -- every layer of the reference configuration -- is read and updated in place."""

    PAD = 64
    PAD_OUT = 64
    TILED = False     # the parameters are the kernels' images here and change every step: no second copy to keep in step

    def __init__(self, flow, lr: float = 1e-3, betas=(0.5, 0.9), eps: float = 1e-8, weight_decay: float = 0.0):
        super().__init__(flow)
        self._adam_args = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        self.adam: Optional[AdamState] = None
        # autograd's passes in flight (seq_passes).  The flow stage runs one pass per iteration (experiments/behavior_net.py:707-710):
        # by default one pass at a time: a forward takes the one plan whether or not an earlier pass is alive, and that pass's
        # backward raises; ``max_passes`` > 1 keeps several, each in a plan of its own
        self._passes = PassPool(1, "the flow")
        # the update sweep beside the next half's chain on a second stream: measured slower (8.1 vs 7.75 ms per step: the sweep's
        # 5120 workgroups hold every CU, the chain's 1024-thread workgroups wait for room) -- off unless asked for
        self.two_streams = os.environ.get("VUNET_SEQ_TRAIN_STREAMS", "1") == "2"
        self._side_stream = None
        # hidden activations also handed from layer to layer tile-major (include/vunet_seq_tiled.h; the row-major copies are the
        # backward pass's): bit-identical values
        self.tile_activations = os.environ.get("VUNET_SEQ_TRAIN_TILED_X", "1") != "0"
        # "1": ONE pass over W per layer in the backward pass -- the update sweep also forms the layer's input gradient
        # (vunet_seq_dwx: no second read of W, 2.5 GB less traffic per step).  Built, bit-for-bit tested, and SLOWER: 7.59 ms per
        # step against 7.09 for the separate vunet_seq_dx chain + one vunet_seq_dw launch per coupling half -- the update then runs
        # as 120 dependent per-layer launches of 512 - 1024 workgroups (each ~15 us per 64 x 64 sub-tile, whatever its size) instead
        # of 30 launches of 5120 independent tiles.  Off by default.
        self.fused_dx = os.environ.get("VUNET_SEQ_TRAIN_FUSED_DX", "0") == "1"
        # "1": the slab sum + LeakyReLU' of a hidden layer's input gradient inside the launch that writes the slabs
        # (vunet_seq_dx_finish: the last workgroup of a column stripe to arrive does it; 90 dependent launches fewer per step).
        # Built, bit-for-bit tested, and SLOWER: 9.6 ms per step against 6.5 -- the device-scope release / acquire around the
        # arrival counter (the slabs come from workgroups on other XCDs, i.e. other L2s) writes back and invalidates each L2
        # once per workgroup, in a step whose update sweep keeps every L2 full of dirty lines.  Off by default.
        self.fused_finish = os.environ.get("VUNET_SEQ_TRAIN_FUSED_FINISH", "0") == "1"

    # ---- weights
    def _pack(self, dev=None):
        if getattr(self.flow, "weight_precision", "f32") != "f32":   # (the inference engine's bf16 images: nothing here reads them)
            raise RuntimeError(BF16_INFERENCE_ONLY)
        before = self._packed_for
        super()._pack(dev)
        if self._packed_for == before and getattr(self, "layers", None) is not None:
            return
        dev = self.blocks[0]["scale"].device
        if self.adam is None:
            self.adam = AdamState(dev, **self._adam_args)
        old = {lay.name: lay for lay in self._all_layers()} if getattr(self, "layers", None) else {}
        self.layers: List[List[List[List[TrainLayer]]]] = []    # [block][half][net][layer]
        for bi, (blk, mod) in enumerate(zip(self.blocks, self.flow.sub_layers)):
            per_half = []
            for hi, half in enumerate(blk["halves"]):
                nets = []
                for ni, kind in enumerate(("s", "t")):
                    lins = getattr(mod.coupling, kind)[hi].linears()
                    nets.append([TrainLayer(f"sub_layers.{bi}.coupling.{kind}.{hi}.main.{2 * li}", lin.weight, lin.bias,
                                            images=(half.w[li][ni], half.b[li][ni])) for li, lin in enumerate(lins)])
                per_half.append(nets)
            self.layers.append(per_half)
        self.inv_swap = torch.argsort(self.swap.long()).to(torch.int32)
        for lay in self._all_layers():
            if lay.name in old:
                lay.adopt_moments(old[lay.name])
        self.norm_moments = getattr(self, "norm_moments", None)
        if self.norm_moments is None or self.norm_moments[0].device != dev:
            n = len(self.blocks)
            self.norm_moments = [torch.zeros(n, 4, self.C, device=dev)]   # per block: scale m, scale v, loc m, loc v

    def _all_layers(self):
        return [lay for blk in self.layers for half in blk for net in half for lay in net]

    # ---- buffers
    def _plan(self, rows: int, slot: int = 0) -> dict:
        """Slot 0 is the fused step's plan (``train_step``: its recorded graph points into it) and the first autograd pass's;
        slot k > 0 is allocated when k + 1 autograd passes of ``rows`` rows are alive."""
        key = ("train", rows) if slot == 0 else ("train", rows, slot)
        p = self._plans.get(key)
        if p is not None:
            return p
        dev = self.blocks[0]["scale"].device
        b_pad = _up(rows, 16)
        n = len(self.blocks)
        z = lambda *s: torch.zeros(*s, device=dev)   # noqa: E731
        halves = [h for blk in self.blocks for h in blk["halves"]]
        h0 = halves[0]
        n_lay = len(h0.dims)
        p = dict(b_pad=b_pad, x_in=z(rows, self.C), x_out=z(rows, self.C), logdet=z(b_pad), noise=z(rows, self.C), scalars=z(4),
                 s0=[z(b_pad, self.ld) for _ in range(n)], s1=[z(b_pad, self.ld) for _ in range(n)],
                 # per block, half: one output buffer per MLP layer (the heads: raw slabs when the head layer splits K)
                 y=[[[z(h.nets * b_pad * m * (h.head_split if li == n_lay - 1 else 1)) for li, (m, _) in enumerate(h.dims)]
                     for h in blk["halves"]] for blk in self.blocks],
                 dz=[[[z(h.nets * b_pad * m) for (m, _) in h.dims] for h in blk["halves"]] for blk in self.blocks],
                 yt=[z(max(h0.nets * b_pad * m for (m, _) in h0.dims[:-1])) for _ in range(2)] if n_lay > 1 else None,
                 dzl=z(b_pad, self.ld), dld=z(b_pad), g0=[z(b_pad, self.ld) for _ in range(2)], g1=z(b_pad, self.ld),
                 gfull=[z(b_pad, self.ld) for _ in range(n)], dx=z(rows, self.C))
        # raw input-gradient slabs: S row ranges of W per launch, chosen so that a launch has >= 256 workgroups
        # fused form (vunet_seq_dwx): one slab per 256-row tile of W; separate form: S row ranges chosen for >= 256 workgroups
        p["tsub"] = [self._dwx_rows(m, k, h0.nets) for (m, k) in h0.dims]      # 64-row sub-tiles per tile of the fused form
        p["S"] = ([(m + 64 * t - 1) // (64 * t) for (m, _), t in zip(h0.dims, p["tsub"])] if self.fused_dx
                  else [dx_split(m, k, h0.nets) for (m, k) in h0.dims])
        p["raw"] = z(max(h0.nets * s * b_pad * k for s, (_, k) in zip(p["S"], h0.dims)))
        p["dx_cnt"] = torch.zeros(h0.nets * max(k for (_, k) in h0.dims) // 64, dtype=torch.int32, device=dev)   # vunet_seq_dx_finish
        p["raw_in"] = [z(h0.nets * p["S"][0] * b_pad * h0.dims[0][1]) for _ in range(2)]
        self._plans[key] = p
        return p

    @staticmethod
    def _dwx_rows(m: int, k: int, nets: int) -> int:
        """Rows per tile of ``vunet_seq_dwx`` in units of 64: as tall as leaves the launch >= ``VUNET_SEQ_DWX_WGS`` workgroups
        (taller tiles: fewer slabs of dX to write and add; shorter: more workgroups in flight)."""
        want = int(os.environ.get("VUNET_SEQ_DWX_WGS", "512"))     # (measured: 512 -> 7.59 ms per step, 1024 -> 8.16, 2048 -> 8.37)
        t = 4
        while t > 1 and ((m + 64 * t - 1) // (64 * t)) * (k // 64) * nets < want:
            t //= 2
        return t

    # ---- forward, everything kept
    def _issue_train_forward(self, rows: int, p: dict):
        """``FlowEngine._issue_forward`` into buffers that stay alive: every block's two states and every MLP layer's output."""
        self._issue_forward(rows, p, p["s0"], p["s1"], p["y"], tile_bufs=p["yt"] if self.tile_activations else None)

    # ---- backward
    def _coupling_bwd(self, rows, p, gbase, ld_g, gslabs, inv_map, scale, in_state, half, heads, gfull, gout, ld_out, dzh):
        h0 = self.blocks[0]["halves"][0]
        d = SeqCouplingBwdDesc(rows, self.C, self.c1, ld_g, self.ld, ld_out, self.ld, half.out_pad if half else self.C,
                               half.head_split if half else 1, (h0.nets * p["S"][0]) if gslabs is not None else 0,
                               h0.dims[0][1], self.c1)
        _call("vunet_seq_coupling_bwd", ctypes.byref(d), _p(gbase), _p(gslabs), _p(inv_map), _p(scale), _p(in_state), _p(heads),
              _p(half.b[-1][0] if half else None), _p(half.b[-1][1] if half else None), _p(p["dld"]), _p(gfull), _p(gout), _p(dzh),
              _stream())

    def _mlp_bwd(self, rows, p, half, ys, dzs, raw_in):
        """The input-gradient chain of one coupling half: head -> first layer.  ``dzs[-1]`` holds the heads' dZ."""
        for li in range(len(half.dims) - 1, -1, -1):
            m_pad, k_pad = half.dims[li]
            raw = raw_in if li == 0 else p["raw"]
            d = SeqDxDesc(rows, m_pad, k_pad, half.nets, p["S"][li], 0)
            if li > 0 and self.fused_finish:   # the stripe's last workgroup finishes dZ of the layer below: one launch, not two
                _call("vunet_seq_dx_finish", ctypes.byref(d), _p(half.w[li][0]), _p(half.w[li][1] if half.nets > 1 else None),
                      _p(dzs[li]), _p(raw), _p(ys[li - 1]), _p(dzs[li - 1]), _p(p["dx_cnt"]), LRELU_SLOPE, _stream())
                continue
            dx_chain(d, half.w[li], dzs[li], raw, (ys[li - 1], dzs[li - 1]) if li > 0 else None, LRELU_SLOPE)

    def _dw_table(self, p: dict, grads: Optional[dict]) -> dict:
        """The update sweep's descriptor table: per block (last first) and half (1, then 0) the eight layers of its two nets.
        ``grads`` (write mode): name -> (g, bg) buffers."""
        b_pad = p["b_pad"]
        entries, ranges, tile = [], [], 0
        for bi in reversed(range(len(self.blocks))):
            for hi in (1, 0):
                half = self.blocks[bi]["halves"][hi]
                first = tile
                for ni in range(half.nets):
                    for li, (m_pad, k_pad) in enumerate(half.dims):
                        lay = self.layers[bi][hi][ni][li]
                        x = (p["s0"][bi] if hi == 0 else p["s1"][bi]) if li == 0 else p["y"][bi][hi][li - 1][ni * b_pad * k_pad:]
                        dz = p["dz"][bi][hi][li][ni * b_pad * m_pad:]
                        entries.append(lay.dw_entry(dz.data_ptr(), m_pad, x.data_ptr(), self.ld if li == 0 else k_pad, tile,
                                                    grads=None if grads is None else grads[lay.name], kv=lay.k))
                        tile += lay.tiles()
                ranges.append((first, tile - first))
        return dict(table=_table(entries, self.blocks[0]["scale"].device), n=len(entries), ranges=ranges, tiles=tile)

    def _dwx_table(self, p: dict, grads: Optional[dict]) -> dict:
        """The fused form's table: per block (last first), half (1, then 0) and LAYER (head first) the two nets' entries -- one
        ``vunet_seq_dwx`` launch each: the update of the layer AND its input gradient (raw slabs over the 256-row tiles of W)."""
        b_pad = p["b_pad"]
        entries, ranges, tile = [], {}, 0
        for bi in reversed(range(len(self.blocks))):
            for hi in (1, 0):
                half = self.blocks[bi]["halves"][hi]
                for li in reversed(range(len(half.dims))):
                    m_pad, k_pad = half.dims[li]
                    first = tile
                    s_li, tsub = p["S"][li], p["tsub"][li]
                    raw = p["raw_in"][hi] if li == 0 else p["raw"]
                    for ni in range(half.nets):
                        lay = self.layers[bi][hi][ni][li]
                        x = (p["s0"][bi] if hi == 0 else p["s1"][bi]) if li == 0 else p["y"][bi][hi][li - 1][ni * b_pad * k_pad:]
                        dz = p["dz"][bi][hi][li][ni * b_pad * m_pad:]
                        dx = raw[ni * s_li * b_pad * k_pad:]
                        entries.append(lay.dw_entry(dz.data_ptr(), m_pad, x.data_ptr(), self.ld if li == 0 else k_pad, tile,
                                                    grads=None if grads is None else grads[lay.name], kv=lay.k, nchunk=tsub,
                                                    dx_raw=dx.data_ptr()))
                        tile += lay.tiles(tsub)
                    ranges[(bi, hi, li)] = (first, tile - first)
        return dict(table=_table(entries, self.blocks[0]["scale"].device), n=len(entries), ranges=ranges, tiles=tile)

    def _norm_table(self, p: dict, grads: Optional[dict]) -> torch.Tensor:
        entries = []
        for bi, (blk, mod) in enumerate(zip(self.blocks, self.flow.sub_layers)):
            mom = self.norm_moments[0][bi]
            gs, gl = grads[f"sub_layers.{bi}.norm_layer"] if grads is not None else (None, None)
            entries.append(SeqActnormLayer(_ptr(blk["scale"]), _ptr(blk["loc"]), _ptr(mom[0]), _ptr(mom[1]), _ptr(mom[2]), _ptr(mom[3]),
                                           _ptr(gs), _ptr(gl), _ptr(p["gfull"][bi]), _ptr(p["s0"][bi]), self.ld, 0))
        return _table(entries, self.blocks[0]["scale"].device)

    def _issue_train_backward(self, rows: int, p: dict, gz: torch.Tensor, ld_gz: int, tables: dict, hp: Optional[SeqAdamHp]):
        """``gz``: d loss / d z [rows.., ld_gz]; ``p['dld']``: d loss / d logdet.  Per block, last first: the step that ends the
        block (coupling half 1 + shuffle + the next block's ActNorm), then that half's MLP -- its input-gradient chain and the
        update of its eight layers, or with ``fused_dx`` both in ONE pass over W per layer (``vunet_seq_dwx`` updates the layer and
        leaves its input gradient as raw slabs: no ``vunet_seq_dx``, the chain does not read W a second time); the same for half 0;
        finally block 0's ActNorm and the ActNorm gradients of all blocks."""
        n, b_pad = len(self.blocks), p["b_pad"]
        hpp = ctypes.byref(hp) if hp is not None else None
        side = self._side() if self.two_streams and not self.fused_dx else None      # (the fused form has no sweep to set aside)
        main = torch.cuda.current_stream()

        def chain_then_sweep(bi, hi, half):
            """The update of one half's eight layers after its chain.  Nothing downstream of it in this pass reads what it
            writes (W, the moments) and the chain never touches the dZ / activation buffers it reads again: with ``two_streams``
            it runs on the side stream beside the next half's input-gradient chain, which alone leaves most of the HBM
            bandwidth idle."""
            dw = tables["dw"]
            self._mlp_bwd(rows, p, half, p["y"][bi][hi], p["dz"][bi][hi], p["raw_in"][hi])
            first, cnt = dw["ranges"][2 * (n - 1 - bi) + 1 - hi]     # (the table's order: block, last first; half 1, then 0)
            if side is None:
                _call("vunet_seq_dw", _p(dw["table"]), dw["n"], first, cnt, rows, hpp, _stream())
                return
            side.wait_stream(main)
            with torch.cuda.stream(side):
                _call("vunet_seq_dw", _p(dw["table"]), dw["n"], first, cnt, rows, hpp, _stream())

        def update_with_dx(bi, hi, half):
            dwx = tables["dwx"]
            for li in reversed(range(len(half.dims))):
                first, cnt = dwx["ranges"][(bi, hi, li)]
                _call("vunet_seq_dwx", _p(dwx["table"]), dwx["n"], first, cnt, rows, hpp, _stream())
                if li > 0:
                    _call("vunet_seq_dz_finish", _p(p["raw"]), _p(p["y"][bi][hi][li - 1]), _p(p["dz"][bi][hi][li - 1]), half.nets,
                          p["S"][li], b_pad, half.dims[li][1], LRELU_SLOPE, _stream())
        mlp = update_with_dx if self.fused_dx else chain_then_sweep
        gbase, ld_g, gsl = gz, ld_gz, None
        for i in reversed(range(n)):
            blk = self.blocks[i]
            h0, h1 = blk["halves"]
            last = i == n - 1
            nxt = None if last else self.blocks[i + 1]
            # half 1: out[c] = A_next(v[fwd[c]]), v = couple_1(S1_i)
            self._coupling_bwd(rows, p, gbase, ld_g, gsl, blk["bwd"], None if last else nxt["scale"], p["s1"][i], h1, p["y"][i][1][-1],
                               None if last else p["gfull"][i + 1], p["g1"], self.ld, p["dz"][i][1][-1])
            mlp(i, 1, h1)
            # half 0: out[c] = v[swap[c]], v = couple_0(S0_i)
            g0 = p["g0"][i % 2]
            self._coupling_bwd(rows, p, p["g1"], self.ld, p["raw_in"][1], self.inv_swap, None, p["s0"][i], h0, p["y"][i][0][-1], None, g0,
                               self.ld, p["dz"][i][0][-1])
            mlp(i, 0, h0)
            gbase, ld_g, gsl = g0, self.ld, p["raw_in"][0]
        # the first step of the pass: S0_0 = A_0(x)
        self._coupling_bwd(rows, p, gbase, ld_g, gsl, None, self.blocks[0]["scale"], None, None, None, p["gfull"][0], p["dx"], self.C, None)
        _call("vunet_seq_actnorm_bwd", _p(tables["norm"]), n, self.C, rows, _p(p["dld"]), hpp, _stream())
        if side is not None:
            main.wait_stream(side)

    def _side(self):
        if self._side_stream is None:
            self._side_stream = torch.cuda.Stream()
        return self._side_stream

    def _write_back(self):
        for lay in self._all_layers():
            lay.write_back()

    # ---- the fused step
    def _initialise_actnorm(self, x2: torch.Tensor):
        """ActNorm's data-dependent initialisation happens on the first forward call of a fresh flow (lib/modules.py:303-305)."""
        if self._initialised():
            return
        if not 2 <= x2.shape[0] <= 64:
            raise ValueError("ActNorm's data-dependent initialisation needs one batch of 2..64 rows")
        p = FlowEngine._plan(self, x2.shape[0])
        p["x_in"].copy_(x2)
        self._issue_forward(x2.shape[0], p, init=True)
        self._all_init = True

    def _check_input(self, x: torch.Tensor) -> torch.Tensor:
        _need_device(x)
        _lib.lib()
        self._pack(x.device)
        x2 = x.reshape(x.shape[0], -1)
        if x2.shape[1] != self.C:
            raise ValueError(f"flow over {self.C} channels got {tuple(x.shape)}")
        if not 1 <= x2.shape[0] <= 64:
            raise ValueError(f"the flow's training step takes one batch of 1..64 rows (config/behavior_net.yaml: 64), got {x2.shape[0]}")
        return x2

    def train_step(self, x: torch.Tensor, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One optimisation step on the batch ``x`` [B, C]: -> device tensor [4] = (flow_loss, reference_nll_loss, nlogdet_loss,
        nll_loss), the entries of ``FlowLoss``'s log (lib/losses.py:310-315).  ``noise``: the draw behind the logged
        ``reference_nll_loss`` (None: ``torch.randn``, as :309 does)."""
        x2 = self._check_input(x.detach())
        rows = x2.shape[0]
        first = not self._initialised()
        self._initialise_actnorm(x2)
        p = self._plan(rows)
        p["x_in"].copy_(x2)
        if noise is None:
            torch.randn(p["noise"].shape, out=p["noise"])
        else:
            p["noise"].copy_(noise.reshape(rows, self.C))
        if "tables" not in p:
            p["tables"] = dict(norm=self._norm_table(p, None), **({"dwx": self._dwx_table(p, None)} if self.fused_dx
                                                                 else {"dw": self._dw_table(p, None)}))

        def issue():
            self.adam.tick()
            self._issue_train_forward(rows, p)
            _call("vunet_seq_flow_loss", _p(p["x_out"]), self.C, _p(p["logdet"]), _p(p["noise"]), rows, self.C, _p(p["scalars"]),
                  _p(p["dzl"]), self.ld, _p(p["dld"]), _stream())
            self._issue_train_backward(rows, p, p["dzl"], self.ld, p["tables"], self.adam.hp)
            self._write_back()
        self.graph.run_step(("train", rows), issue)
        # the step wrote every parameter of the flow; a replayed recording runs no host code, so it is announced here.  This
        # engine's images are what was written: it takes the new stamp instead of re-packing at its next call (the step that
        # ran ActNorm's initialisation does not: the ``initialized`` buffers moved too, and the call after it re-packs once)
        mark_written(self.flow.parameters())
        if not first:
            self._packed_for = self._key()
        return p["scalars"]

    # ---- autograd's view of the same kernels
    def train_forward(self, x: torch.Tensor):
        """-> (z, logdet, token).  With ``max_passes`` > 1 the pass takes the lowest free slot of its batch size and keeps that
        plan until ``token`` (held by the autograd node) is collected, as the behaviour net's passes do.  With ``max_passes`` 1
        (the default) there is one plan and no waiting for it: a forward takes it whether or not an earlier pass is alive, and
        that pass's backward then raises.  Either way ``train_backward(token, ...)`` may run any number of times, and the token
        carries the plan itself: its buffers stay valid when a re-pack clears ``_plans``."""
        x2 = self._check_input(x.detach())
        rows = x2.shape[0]
        self._initialise_actnorm(x2)
        lease = self._passes.lease(rows) if self._passes.max_passes > 1 else None
        p = self._plan(rows, lease.slot if lease is not None else 0)
        p["x_in"].copy_(x2)
        self._issue_train_forward(rows, p)
        p["pass"] = p.get("pass", 0) + 1      # which forward the plan's activations belong to
        return p["x_out"].clone(), p["logdet"][:rows].clone(), (p, lease, rows, p["pass"], self._key())

    def train_backward(self, token, gz: Optional[torch.Tensor], gld: Optional[torch.Tensor]):
        """-> (dx [B, C], {parameter name: gradient}) for the forward pass ``token`` came from.  The pass is not spent: every
        buffer the chain writes is written anew by each run, so a second call returns the same bits.  Parameters that were
        modified since the forward are refused, as torch refuses them (the kernels read the weights in place: the gradients would
        be those of another function)."""
        p, _, rows, pass_id, versions = token
        if pass_id != p["pass"]:
            raise RuntimeError("the flow was run again before this pass's backward: its saved activations are gone (with max_passes "
                               "= 1, the default, the engine keeps one forward pass at a time: raise its max_passes attribute to keep "
                               "several in flight)")
        if versions != self._key():
            raise RuntimeError(STALE_WEIGHTS.format("flow"))
        dev = p["x_in"].device
        p["dzl"].zero_()
        if gz is not None:
            p["dzl"][:rows, :self.C].copy_(gz.reshape(rows, self.C))
        p["dld"].zero_()
        if gld is not None:
            p["dld"][:rows].copy_(gld.reshape(rows))
        grads = {lay.name: (torch.empty_like(lay.w), torch.empty_like(lay.b)) for lay in self._all_layers()}
        for bi in range(len(self.blocks)):
            grads[f"sub_layers.{bi}.norm_layer"] = (torch.empty(self.C, device=dev), torch.empty(self.C, device=dev))
        tables = dict(norm=self._norm_table(p, grads), **({"dwx": self._dwx_table(p, grads)} if self.fused_dx
                                                          else {"dw": self._dw_table(p, grads)}))
        self._issue_train_backward(rows, p, p["dzl"], self.ld, tables, None)
        out = {}
        for lay in self._all_layers():
            g, bg = grads[lay.name]
            m, k = lay.weight.shape
            out[lay.name + ".weight"] = g if g.shape == (m, k) else g[:m, :k].contiguous()
            out[lay.name + ".bias"] = bg if bg.numel() == m else bg[:m].contiguous()
        for bi in range(len(self.blocks)):
            gs, gl = grads[f"sub_layers.{bi}.norm_layer"]
            out[f"sub_layers.{bi}.norm_layer.scale"] = gs.reshape(1, self.C, 1, 1)
            out[f"sub_layers.{bi}.norm_layer.loc"] = gl.reshape(1, self.C, 1, 1)
        return p["dx"].clone(), out

    # ---- torch.optim.Adam's state layout (checkpoints: experiments/behavior_net.py:392-393, :1003-1011)
    def _norm_moment_views(self):
        """name -> (exp_avg, exp_avg_sq) views of the ActNorm moments, in the parameters' shapes."""
        out = {}
        for bi in range(len(self.blocks)):
            mom = self.norm_moments[0][bi].reshape(4, 1, self.C, 1, 1)
            out[f"sub_layers.{bi}.norm_layer.scale"], out[f"sub_layers.{bi}.norm_layer.loc"] = (mom[0], mom[1]), (mom[2], mom[3])
        return out

    def optimizer_state_dict(self) -> dict:
        self._pack()
        by_name = {n: (m.clone(), v.clone()) for n, (m, v) in self._norm_moment_views().items()}
        for lay in self._all_layers():
            by_name[lay.name + ".weight"], by_name[lay.name + ".bias"] = lay.moments()
        return adam_state_dict(self.adam, self.adam.step, [by_name[n] for n, _ in self.flow.named_parameters()], name="latent_flow")

    def load_optimizer_state_dict(self, sd: dict):
        self._pack()
        states, step = load_adam_state(self.adam, sd)
        by_name = dict(zip((n for n, _ in self.flow.named_parameters()), states))
        for lay in self._all_layers():
            lay.set_moments(by_name[lay.name + ".weight"], by_name[lay.name + ".bias"])
        for n, views in self._norm_moment_views().items():
            for i, view in enumerate(views):
                if by_name[n] is None:
                    view.zero_()
                else:
                    view.copy_(by_name[n][i])
        self.adam.step_dev.fill_(step)
        self.graph.clear()   # the hyper-parameters are launch arguments of the recorded step


class _FlowFn(torch.autograd.Function):
    """``UnconditionalFlow2.forward(x)`` -> (z, logdet) as one autograd node whose backward is ``FlowTrainEngine.train_backward``:
    what ``f_loss.backward()`` (experiments/behavior_net.py:710) reaches when the reference's own loop drives these modules."""

    @staticmethod
    def forward(ctx, engine, names, x, *params):
        z, logdet, token = engine.train_forward(x)
        ctx.engine, ctx.names, ctx.token, ctx.x_shape = engine, names, token, x.shape
        return z, logdet

    @staticmethod
    def backward(ctx, gz, gld):
        dx, grads = ctx.engine.train_backward(ctx.token, gz, gld)
        out = [None, None, dx.reshape(ctx.x_shape) if ctx.needs_input_grad[2] else None]
        for i, n in enumerate(ctx.names):
            out.append(grads[n] if ctx.needs_input_grad[3 + i] else None)
        return tuple(out)


def flow_autograd(engine: FlowTrainEngine, x: torch.Tensor):
    """(z [B, C], logdet [B]) with a graph: the forward of the flow for a loop that calls ``backward()`` itself."""
    if getattr(engine.flow, "weight_precision", "f32") != "f32":
        raise RuntimeError(BF16_INFERENCE_ONLY)
    named = list(engine.flow.named_parameters())
    return _FlowFn.apply(engine, [n for n, _ in named], x, *[p for _, p in named])


# ================================================================================================
# the behaviour cVAE (first stage of experiments/behavior_net.py: :591-660)
# ================================================================================================
from .seq import BehaviorEngine, SeqLinearDesc, SeqLstmDesc, ACT_NONE, linear   # noqa: E402


class BehaviorTrainEngine(KeepsPasses, BehaviorEngine):
    """``ResidualBehaviorNet.forward(x1, x2, len)`` (models/pose_behavior_rnn.py:574-586) with every step's operand row, cell
    state and gate activations kept, and its backward pass: back-propagation through time over the decoder's roll-out and the
    encoder's LSTM (csrc/seq_bptt.hip + the matrix kernels of csrc/seq_train.hip).  One batch of <= 64 rows
    (config/behavior_net.yaml: 64).  Gradients are written in torch's parameter layout -- into the ``.grad`` views of the fused
    optimiser (``experiments.behavior_net``) or into fresh tensors for autograd (``behavior_autograd``).

    Under autograd several passes may be alive at once, as in the reference's ``train_fn`` (experiments/behavior_net.py:616, :627,
    :681: three calls of one shape per iteration): every pass keeps a plan of its own -- the lowest free slot of its shape,
    ``seq_passes.PassPool``; slot k is allocated when k + 1 passes of that shape are alive, at most ``max_passes`` (4) -- until its
    autograd node dies, and its backward may run more than once (``retain_graph=True``).  A backward after the parameters were
    modified raises, as torch's does -- after a step of ``optim.FusedAdam`` too, which announces its writes
    (``ops.mark_written``).  ``experiments.behavior_net.BehaviorNet``'s fused step works in slot 0 without taking it."""

    HOFF_PAD = 64

    def __init__(self, net):
        super().__init__(net)
        self._passes = PassPool(4, "the behaviour net")

    def _check(self, dev=None):
        net = self.net
        if net.decoder.use_nin:
            raise NotImplementedError("training with linear_in_decoder=True is not built (config/behavior_net.yaml trains with False): "
                                      "the input layer is folded into the gate matrix on this path")
        if not net.ib:
            raise NotImplementedError("training without the information bottleneck is not built (experiments/behavior_net.py:310 "
                                      "always constructs the net with information_bottleneck=True)")
        self._pack(dev)
        if self.H % 64:
            raise ValueError("dim_hidden_b must be a multiple of 64 for training on the HIP path")

    def _tplan(self, rows: int, t_in: int, t2: int, length: int, slot: int = 0) -> dict:
        """Slot 0 is the fused step's plan (its recorded graph points into it) and the first autograd pass's."""
        key = ("train", rows, t_in, t2, length) + ((slot,) if slot else ())
        p = self._plans.get(key)
        if p is not None:
            return p
        dev = self.dec_w.device
        bp, H, n, ldx = _up(rows, 16), self.H, self.n, self.ldx
        z = lambda *s: torch.zeros(*s, device=dev)   # noqa: E731
        s_d, s_e, s_h = dx_split(4 * H, ldx, 1), dx_split(4 * H, H, 1), dx_split(H, H, 2)
        p = dict(b_pad=bp, x1=z(rows, t_in, n), x2=z(rows, t2, n), eps=z(rows, H), target=z(rows, length, n),
                 xh_e=z(t_in + 1, bp, ldx), c_e=z(t_in + 1, bp, H), gates_e=z(t_in, bp, 4 * H),
                 xh_d=z(length + 1, bp, ldx), c_d=z(length + 1, bp, H), gates_d=z(length, bp, 4 * H),
                 xraw=z(bp, self.ldraw), pre=z(bp, H), heads=z(2 * bp * H), mu=z(rows, H), logstd=z(rows, H), b=z(rows, H),
                 xs=z(rows, length, n), cs=z(rows, length, n),
                 dgates_d=z(length, bp, 4 * H), dgates_e=z(t_in, bp, 4 * H), gx=z(length + 1, bp, 64), gc=z(bp, H), dy=z(2, bp, H),
                 S=(s_d, s_e, s_h), raw_d=z(s_d * bp * ldx), raw_e=z(s_e * bp * H), raw_h=z(2 * s_h * bp * H),
                 gxs=z(rows, length, n), gmu=z(rows, H), glogstd=z(rows, H),
                 ht=[z(bp * H) for _ in range(2)] if self._h_as_tiles(bp) else None,
                 g_dec=z(4 * H, ldx), gb_dec=z(4 * H), g_enc=z(4 * H, ldx), gb_enc=z(4 * H), g_out=z(64, H), gb_out=z(64),
                 g_mu=z(H, H), gb_mu=z(H), g_std=z(H, H), gb_std=z(H), zero_bias=z(4 * H),
                 part=z(length + 3 * rows), scalars=z(6), per_seq=z(length))
        # the weight-gradient sweep (write mode): every layer of the net in one launch
        entries, tile = [], 0

        def layer(g, gb, dz, x, m, k, ldz, ldx_, nchunk, cz, cx):
            nonlocal tile
            entries.append(SeqDwLayer(None, None, None, g.data_ptr(), p["zero_bias"].data_ptr(), None, None, gb.data_ptr(), dz.data_ptr(),
                                      x.data_ptr(), m, k, ldz, ldx_, tile, k // 64, k, nchunk, cz, cx, None))
            tile += (m // 64) * (k // 64)
        layer(p["g_dec"], p["gb_dec"], p["dgates_d"], p["xh_d"], 4 * H, ldx, 4 * H, ldx, length, bp * 4 * H, bp * ldx)
        layer(p["g_enc"], p["gb_enc"], p["dgates_e"], p["xh_e"], 4 * H, ldx, 4 * H, ldx, t_in, bp * 4 * H, bp * ldx)
        layer(p["g_out"], p["gb_out"], p["gx"], p["xh_d"][1:, :, self.hoff:], 64, H, 64, ldx, length, bp * 64, bp * ldx)
        layer(p["g_mu"], p["gb_mu"], p["dy"][0], p["pre"], H, H, H, H, 1, 0, 0)
        layer(p["g_std"], p["gb_std"], p["dy"][1], p["pre"], H, H, H, H, 1, 0, 0)
        p["dw"] = dict(table=_table(entries, dev), n=len(entries), tiles=tile)
        self._plans[key] = p
        return p

    # ---- forward, everything kept
    def _issue_train_forward(self, rows, p, t_in, t2, length, start_frame, sample_prior: bool):
        dec = self.net.decoder
        n, H, esz = self.n, self.H, 4
        x1, x2 = p["x1"], p["x2"]
        _call("vunet_seq_start", _p(x1), t_in * n, None, None, None, 0, _p(p["xh_e"][0]), self.ldx, self.hoff, _p(p["c_e"][0]), rows, n, H,
              _stream())
        d = SeqLstmDesc(rows, H, self.ldx, self.hoff, n, self.ldraw, t_in * n)
        for t in range(t_in):
            x_next = ctypes.c_void_p(x1.data_ptr() + (t + 1) * n * esz) if t + 1 < t_in else None
            self._lstm_step(d, self.enc_wt, self.enc_b, p["xh_e"][t], p["xh_e"][t + 1], p["c_e"][t], p["c_e"][t + 1], *self._ht(p, t),
                            p["pre"] if t == t_in - 1 else None, x_next, p["gates_e"][t])
        w, bias = self.heads
        dl = SeqLinearDesc(rows, H, H, H, ACT_NONE, ACT_NONE, 2, 1, 1)
        linear(dl, w, p["pre"], bias, p["heads"])
        _call("vunet_seq_bottleneck", _p(p["heads"]), H, _p(p["eps"]), _p(p["mu"]), _p(p["logstd"]), _p(p["b"]), rows, H, _stream())
        b_used = p["eps"] if sample_prior else p["b"]      # ``sample=True``: b is the noise itself (:198-199, :208-209)
        x0 = ctypes.c_void_p(x2.data_ptr() + start_frame * n * esz)
        _call("vunet_seq_start", x0, t2 * n, _p(b_used), _p(b_used), _p(p["xraw"]), self.ldraw, _p(p["xh_d"][0]), self.ldx, self.hoff,
              _p(p["c_d"][0]), rows, n, H, _stream())
        d = SeqLstmDesc(rows, H, self.ldx, self.hoff, n, self.ldraw, length * n)
        xs, cs = p["xs"], p["cs"]
        for t in range(length):
            self._lstm_step(d, self.dec_wt, self.dec_b, p["xh_d"][t], p["xh_d"][t + 1], p["c_d"][t], p["c_d"][t + 1], *self._ht(p, t),
                            None, None, p["gates_d"][t])
            _call("vunet_seq_decoder_out", ctypes.byref(d), _p(p["xh_d"][t + 1]), _p(dec.n_out.weight.detach()), _p(dec.n_out.bias.detach()),
                  _p(p["xraw"]), ctypes.c_void_p(xs.data_ptr() + t * n * esz), ctypes.c_void_p(cs.data_ptr() + t * n * esz), _stream())

    # ---- backward
    def _issue_train_backward(self, rows, p, t_in, length, sample_prior: bool, gpre: Optional[torch.Tensor] = None,
                              decoder: bool = True):
        """``p['gxs']`` = d loss / d xs, ``p['gmu']`` / ``p['glogstd']`` = the loss's direct gradients wrt the heads.  Leaves the
        weight gradients as images in ``p`` (``_unpack_grads`` turns them into torch's layout).  Every buffer the chain reads is
        written by the chain first (``gc`` starts from zero by the ``first`` flags, the slabs and dgates are stored, not added
        to): the pass can be run again.  ``decoder`` False: nothing reaches the roll-out (the loss sees mu / logstd / pre only) --
        its 2 x length launches are skipped and what they would have left, all zeros, is filled in."""
        dec = self.net.decoder
        n, H, esz = self.n, self.H, 4
        s_d, s_e, s_h = p["S"]
        w_out = dec.n_out.weight.detach()
        if not decoder:
            for k in ("raw_d", "gc", "dgates_d", "gx"):
                p[k].zero_()
        for t in reversed(range(length if decoder else 0)):
            first = t == length - 1
            d = SeqCellBwdDesc(rows, H, n, s_d, self.ldx, self.hoff, 3 if first else 0, 0, length * n)
            _call("vunet_seq_cell_bwd", ctypes.byref(d), None if first else _p(p["raw_d"]), _p(w_out),
                  ctypes.c_void_p(p["gxs"].data_ptr() + t * n * esz), None if first else _p(p["gx"][t + 1]), _p(p["gx"][t]),
                  _p(p["gates_d"][t]), _p(p["c_d"][t]), _p(p["c_d"][t + 1]), _p(p["gc"]), _p(p["dgates_d"][t]), _stream())
            dd = SeqDxDesc(rows, 4 * H, self.ldx, 1, s_d, 0)
            _call("vunet_seq_dx", ctypes.byref(dd), _p(self.dec_w), None, _p(p["dgates_d"][t]), _p(p["raw_d"]), _stream())
        # h0 = c0 = b (models/pose_behavior_rnn.py:612-614); b = eps exp(logstd) + mu, or the noise itself
        _call("vunet_seq_bottleneck_bwd", _p(p["raw_d"]), s_d, self.ldx, self.hoff, _p(p["gc"]), None if sample_prior else _p(p["eps"]),
              _p(p["logstd"]), _p(p["gmu"]), _p(p["glogstd"]), _p(p["dy"]), rows, H, _stream())
        if sample_prior:   # b does not depend on the encoder: only the loss's direct terms reach the heads
            p["dy"][0, :rows].copy_(p["gmu"])
            p["dy"][1, :rows].copy_(p["glogstd"])
        dh = SeqDxDesc(rows, H, H, 2, s_h, 0)
        _call("vunet_seq_dx", ctypes.byref(dh), _p(self.heads[0][0]), _p(self.heads[0][1]), _p(p["dy"]), _p(p["raw_h"]), _stream())
        if gpre is not None:
            p["raw_h"][:p["b_pad"] * H].view(p["b_pad"], H)[:rows].add_(gpre)
        enc_w_h = ctypes.c_void_p(self.enc_w.data_ptr() + self.hoff * esz)
        for t in reversed(range(t_in)):
            last = t == t_in - 1
            d = SeqCellBwdDesc(rows, H, n, 2 * s_h if last else s_e, H, 0, 2 if last else 0, 0, 0)
            _call("vunet_seq_cell_bwd", ctypes.byref(d), _p(p["raw_h"] if last else p["raw_e"]), None, None, None, None,
                  _p(p["gates_e"][t]), _p(p["c_e"][t]), _p(p["c_e"][t + 1]), _p(p["gc"]), _p(p["dgates_e"][t]), _stream())
            if t > 0:   # (h0 of the encoder is a constant)
                de = SeqDxDesc(rows, 4 * H, H, 1, s_e, self.ldx)
                _call("vunet_seq_dx", ctypes.byref(de), enc_w_h, None, _p(p["dgates_e"][t]), _p(p["raw_e"]), _stream())
        _call("vunet_seq_dw", _p(p["dw"]["table"]), p["dw"]["n"], 0, p["dw"]["tiles"], rows, None, _stream())

    def _unpack_grads(self, p, out: Dict[str, torch.Tensor]):
        """The images of the sweep -> ``out[name]`` (tensors in the parameters' shapes, written in place)."""
        net = self.net
        n, H = self.n, self.H
        _call("vunet_seq_lstm_grads_unpack", _p(p["g_dec"]), _p(p["gb_dec"]), self.ldx, self.hoff, n, H, _p(out["decoder.rnn.weight_ih"]),
              _p(out["decoder.rnn.weight_hh"]), _p(out["decoder.rnn.bias_ih"]), _p(out["decoder.rnn.bias_hh"]), _stream())
        _call("vunet_seq_lstm_grads_unpack", _p(p["g_enc"]), _p(p["gb_enc"]), self.ldx, self.hoff, n, H, _p(out["b_enc.rnn.weight_ih_l0"]),
              _p(out["b_enc.rnn.weight_hh_l0"]), _p(out["b_enc.rnn.bias_ih_l0"]), _p(out["b_enc.rnn.bias_hh_l0"]), _stream())
        _call("vunet_seq_unpack_rows", _p(p["g_out"]), H, 0, 0, 1, _p(out["decoder.n_out.weight"]), n, H, 0, _stream())
        _call("vunet_seq_unpack_rows", _p(p["gb_out"]), 64, 0, 0, 1, _p(out["decoder.n_out.bias"]), 1, n, 0, _stream())
        for tag, head, g, gb in (("mu_fn", net.b_enc.mu_fn, p["g_mu"], p["gb_mu"]), ("std_fn", net.b_enc.std_fn, p["g_std"], p["gb_std"])):
            v, gg, bias, gamma, beta = head._params()
            q = f"b_enc.{tag}."
            _call("vunet_seq_normlinear_bwd", _p(g), _p(gb), _p(v.detach()), _p(gg.detach()), _p(bias.detach()), _p(gamma.detach()), H, H,
                  _p(out[q + "conv.weight_v"]), _p(out[q + "conv.weight_g"]), _p(out[q + "conv.bias"]), _p(out[q + "gamma"]),
                  _p(out[q + "beta"]), _stream())

    def grad_names(self):
        return [n for n, _ in self.net.named_parameters()]

    # ---- autograd's view
    def train_forward(self, x1, x2, length, start_frame, eps, sample_prior):
        _need_device(x1, x2, eps)
        _lib.lib()
        self._check(x1.device)
        rows, t_in, t2 = x1.shape[0], x1.shape[1], x2.shape[1]
        if not 1 <= rows <= 64:
            raise ValueError(f"the behaviour net's training step takes one batch of 1..64 rows, got {rows}")
        if x1.shape[2] != self.n or x2.shape[2] != self.n or x2.shape[0] != rows:
            raise ValueError(f"forward: sequences {tuple(x1.shape)}, {tuple(x2.shape)} for {self.n} pose dimensions")
        start_frame = start_frame % t2
        lease = self._passes.lease((rows, t_in, t2, length))
        p = self._tplan(rows, t_in, t2, length, lease.slot)
        p["x1"].copy_(x1)
        p["x2"].copy_(x2)
        p["eps"].copy_(eps)
        # (the weight images are those of the parameters as they are: ``_check`` -> ``_pack`` re-filled them if a version moved)
        self._issue_train_forward(rows, p, t_in, t2, length, start_frame, sample_prior)
        return p, (p, lease, rows, t_in, length, sample_prior, _versions(list(self.net.parameters())))

    def train_backward(self, token, gxs, gcs, gb, gmu, glogstd, gpre):
        """{parameter name: gradient} of the pass ``token`` came from; the pass is not spent (``retain_graph=True``)."""
        p, _, rows, t_in, length, sample_prior, versions = token
        if versions != _versions(list(self.net.parameters())):
            raise RuntimeError(STALE_WEIGHTS.format("behaviour net"))
        p["gxs"].zero_()
        if gxs is not None:
            p["gxs"].copy_(gxs)
        if gcs is not None:      # cs[t] is the input of step t: x_start for t = 0, xs[t - 1] after (:618-620)
            p["gxs"][:, :-1].add_(gcs[:, 1:])
        p["gmu"].zero_()
        p["glogstd"].zero_()
        if gmu is not None:
            p["gmu"].copy_(gmu)
        if glogstd is not None:
            p["glogstd"].copy_(glogstd)
        if gb is not None and not sample_prior:   # b = eps exp(logstd) + mu
            p["gmu"].add_(gb)
            p["glogstd"].add_(gb * p["eps"] * torch.exp(p["logstd"]))
        self._issue_train_backward(rows, p, t_in, length, sample_prior, gpre,
                                   decoder=not (gxs is None and gcs is None and gb is None))
        out = {n: torch.empty_like(q) for n, q in self.net.named_parameters()}
        self._unpack_grads(p, out)
        return out


class _BehaviorFn(torch.autograd.Function):
    """``ResidualBehaviorNet.forward`` as one autograd node (inputs are data: no gradient wrt the sequences)."""

    @staticmethod
    def forward(ctx, engine, names, x1, x2, length, start_frame, eps, sample_prior, *params):
        p, token = engine.train_forward(x1, x2, length, start_frame, eps, sample_prior)
        ctx.engine, ctx.names, ctx.token = engine, names, token
        ctx.set_materialize_grads(False)
        b = p["eps"] if sample_prior else p["b"]
        return p["xs"].clone(), p["cs"].clone(), b.clone(), p["mu"].clone(), p["logstd"].clone(), p["pre"][:x1.shape[0]].clone()

    @staticmethod
    def backward(ctx, gxs, gcs, gb, gmu, glogstd, gpre):
        grads = ctx.engine.train_backward(ctx.token, gxs, gcs, gb, gmu, glogstd, gpre)
        return (None,) * 8 + tuple(grads[n] if ctx.needs_input_grad[8 + i] else None for i, n in enumerate(ctx.names))


def behavior_autograd(engine: BehaviorTrainEngine, x1, x2, length, start_frame, eps, sample_prior):
    """(xs, cs, b, mu, logstd, pre) with a graph whose backward is the HIP back-propagation through time."""
    named = list(engine.net.named_parameters())
    return _BehaviorFn.apply(engine, [n for n, _ in named], x1.contiguous(), x2.contiguous(), int(length), int(start_frame), eps,
                             bool(sample_prior), *[q for _, q in named])


# ================================================================================================
# the cVAE's adversarial pose regressor (experiments/behavior_net.py:627-648; models/pose_behavior_rnn.py:47-62)
# ================================================================================================
ACT_RELU_SEQ = 3   # vunet_seq_linear's plain ReLU
REG_STEPS = 5      # inner regressor steps per cVAE step (:628)
REG_T, REG_C = _lib.const("VUNET_SEQ_REG_T"), _lib.const("VUNET_SEQ_REG_C")   # fc4 is Linear(50, 128) on the one-hot of a step


class RegressorTrainEngine:
    """``Regressor_fly``'s five inner steps of the cVAE's first stage and the adversarial term's gradient wrt mu, issued into
    the cVAE step's recorded launch sequence (include/vunet_seq_reg.h, csrc/seq_reg.hip).  Per inner step k: forward (fc1 -> fc2
    -> fc3 with ReLU, fc4 of the one-hot as one column of W4, fc5), ``L_k = mean((pred - seq_b[:, idx_k])^2)``, its input
    gradients on the weights before the step, then the weight gradients fused into the regressor's own Adam (betas 0.9 / 0.999,
    eps 1e-8; its step count advances by five per cVAE step).  After the fifth, the input gradient of ``L_5`` is run back to mu
    through the UPDATED weights with the fifth forward's ReLU masks -- what the reference's torch 1.3.1 computes, whose Adam
    writes through ``p.data`` -- scaled by ``-w ([L_5 <= 0.45] + [L_5 <= 0.7])``.

    The module's fc1 .. fc4 parameters are the kernels' operands and are updated in place (fc4, one column per inner step, by a
    kernel of its own on moments in the parameter's shape); fc5 (51 rows) trains as a zero-padded 64-row image, written back into
    the module by ``write_back``."""

    def __init__(self, reg, lr: float = 1e-4, betas=(0.9, 0.999), eps: float = 1e-8):
        H, n = reg.n_dim, reg.n_key
        if H % 256:
            raise ValueError(f"the regressor's training kernels take dim_hidden_b as a multiple of 256 (its fc3 has dim_hidden_b / 4 "
                             f"rows, tiles of 64), got {H}")
        if n > 64:
            raise ValueError(f"the regressor's output is padded to 64 rows: at most 64 pose dimensions, got {n}")
        self.reg = reg
        self.H, self.H4, self.K5, self.n = H, H // 4, H // 4 + REG_C, n
        dev = reg.fc1.weight.device
        self.adam = AdamState(dev, lr, betas, eps, 0.0)
        self._plans: Dict[int, dict] = {}
        self.load_module()

    def load_module(self):
        """(Re)build the training state from the module's parameters: the fc5 image; Adam's moments and step count are reset."""
        r = self.reg
        self.fc1, self.fc2, self.fc3, self.fc5 = (TrainLayer(n, lin.weight, lin.bias)
                                                  for n, lin in (("fc1", r.fc1), ("fc2", r.fc2), ("fc3", r.fc3), ("fc5", r.fc5)))
        self.fc4 = TrainLayer("fc4", r.fc4.weight, r.fc4.bias, images=(r.fc4.weight.data, r.fc4.bias.data))
        self.layers = [self.fc1, self.fc2, self.fc3, self.fc4, self.fc5]          # the order of ``reg.parameters()``
        for layer in self.layers:
            layer.ensure_moments()
        self._inplace = [t for layer in self.layers for t in layer.inplace_params()]
        self.w5, self.b5 = self.fc5.w, self.fc5.b
        self.adam.step_dev.zero_()
        self._plans.clear()

    def plan(self, rows: int) -> dict:
        p = self._plans.get(rows)
        if p is not None:
            return p
        dev = self.w5.device
        bp, H, H2, H4, K5 = _up(rows, 16), self.H, self.H // 2, self.H4, self.K5
        z = lambda *s: torch.zeros(*s, device=dev)   # noqa: E731
        S = {"fc5": dx_split(64, K5, 1), "fc3": dx_split(H4, H2, 1), "fc2": dx_split(H2, H, 1), "fc1": dx_split(H, H, 1)}
        p = dict(b_pad=bp, S=S, idx=torch.zeros(REG_STEPS, dtype=torch.int32, device=dev), mu=z(bp, H), h1=z(bp, H), h2=z(bp, H2),
                 h3=z(bp, H4), cat=z(bp, K5), pred=z(bp, 64), tgt=z(bp, self.n), dpred=z(bp, 64), dz1=z(bp, H), dz2=z(bp, H2),
                 dz3=z(bp, H4), dzc=z(bp, REG_C), reg=z(6), adv=z(rows, H),
                 raw=z(max(S["fc5"] * bp * K5, S["fc3"] * bp * H2, S["fc2"] * bp * H, S["fc1"] * bp * H)))
        # the update sweep: fc1, fc2, fc3, fc5 in one launch (fc4 has its own kernel)
        entries, tile = [], 0
        for layer, dz, x in zip((self.fc1, self.fc2, self.fc3, self.fc5), (p["dz1"], p["dz2"], p["dz3"], p["dpred"]),
                                (p["mu"], p["h1"], p["h2"], p["cat"])):
            entries.append(layer.dw_entry(dz.data_ptr(), layer.mp, x.data_ptr(), layer.kp, tile))
            tile += layer.tiles()
        p["dw"] = dict(table=_table(entries, dev), n=len(entries), tiles=tile)
        self._plans[rows] = p
        return p

    def _dx_chain(self, rows: int, p: dict, dzc: Optional[torch.Tensor]):
        """d L / d pred (p['dpred']) back to the dZ of fc1 (p['dz1']) on the weights as they are now; ``dzc``: fc4's dZ too."""
        S = p["S"]
        dx_chain(SeqDxDesc(rows, 64, self.K5, 1, S["fc5"], 0), [self.w5], p["dpred"], p["raw"])
        _call("vunet_seq_reg_cat_bwd", _p(p["raw"]), S["fc5"], p["b_pad"], self.H4, _p(p["cat"]), _p(p["dz3"]), _p(dzc), _stream())
        for lay, dz_in, y_prev, dz_out in ((self.fc3, p["dz3"], p["h2"], p["dz2"]), (self.fc2, p["dz2"], p["h1"], p["dz1"])):
            dx_chain(SeqDxDesc(rows, lay.mp, lay.kp, 1, S[lay.name], 0), [lay.w], dz_in, p["raw"], (y_prev, dz_out))

    def issue_step(self, rows: int, p: dict, mu: torch.Tensor, seq: torch.Tensor, t_len: int, weight: float, scalars: torch.Tensor,
                   gmu: Optional[torch.Tensor]):
        """The five inner steps on ``mu`` [rows, H] and ``seq`` [rows, t_len, n] with the indices in ``p['idx']``; the fifth adds
        the adversarial term into ``scalars[0]`` (the logged loss) and -- ``gmu`` not None -- its gradient into ``gmu``."""
        r, H, H2, H4, K5 = self.reg, self.H, self.H // 2, self.H4, self.K5
        hpp = ctypes.byref(self.adam.hp)
        _call("vunet_seq_unpack_rows", _p(mu), H, 0, 0, 1, _p(p["mu"]), rows, H, 0, _stream())     # fc1's operand, padded rows
        for k in range(REG_STEPS):
            for lin, x, y, m, kk in ((r.fc1, p["mu"], p["h1"], H, H), (r.fc2, p["h1"], p["h2"], H2, H), (r.fc3, p["h2"], p["h3"], H4, H2)):
                linear(SeqLinearDesc(rows, m, kk, kk, ACT_RELU_SEQ, ACT_NONE, 1, 1, 1), [lin.weight.data], x, [lin.bias.data], y)
            _call("vunet_seq_reg_gather", _p(r.fc4.weight.data), _p(r.fc4.bias.data), _p(p["idx"]), k, _p(p["h3"]), _p(seq), t_len * self.n,
                  self.n, rows, H4, _p(p["cat"]), _p(p["tgt"]), _stream())
            linear(SeqLinearDesc(rows, 64, K5, K5, ACT_NONE, ACT_NONE, 1, 1, 1), [self.w5], p["cat"], [self.b5], p["pred"])
            last = k == REG_STEPS - 1
            _call("vunet_seq_reg_loss", _p(p["pred"]), 64, _p(p["tgt"]), rows, self.n, k, float(weight), _p(p["reg"]), _p(p["dpred"]),
                  _p(scalars) if last else None, _stream())
            self._dx_chain(rows, p, p["dzc"])          # on the weights before this step's update
            self.adam.tick()
            _call("vunet_seq_dw", _p(p["dw"]["table"]), p["dw"]["n"], 0, p["dw"]["tiles"], rows, hpp, _stream())
            _call("vunet_seq_reg_fc4_adam", _p(p["dzc"]), p["b_pad"], _p(p["idx"]), k, _p(r.fc4.weight.data), _p(r.fc4.bias.data),
                  _p(self.fc4.m), _p(self.fc4.v), _p(self.fc4.bm), _p(self.fc4.bv), hpp, _stream())
        if gmu is None:
            return
        # the adversarial term: L_5's input gradient through the updated weights, the fifth forward's masks (torch 1.3.1)
        self._dx_chain(rows, p, None)
        s1 = p["S"]["fc1"]
        d = SeqDxDesc(rows, H, H, 1, s1, 0)
        _call("vunet_seq_dx", ctypes.byref(d), _p(r.fc1.weight.data), None, _p(p["dz1"]), _p(p["raw"]), _stream())
        _call("vunet_seq_reg_adv", _p(p["raw"]), s1, rows, H, _p(p["reg"]), _p(gmu), _p(p["adv"]), _stream())

    def mark_written(self):
        """``issue_step`` ran, or a recording that holds it was replayed: announce the parameters its updates wrote in place."""
        mark_written(self._inplace)

    # ---- checkpoints: the reference's layout (``Regressor_fly`` keys; torch.optim.Adam's state)
    def write_back(self):
        self.fc5.write_back()

    def _params(self):
        r = self.reg
        return [r.fc1.weight, r.fc1.bias, r.fc2.weight, r.fc2.bias, r.fc3.weight, r.fc3.bias, r.fc4.weight, r.fc4.bias, r.fc5.weight,
                r.fc5.bias]

    def state_dict(self) -> dict:
        self.write_back()
        return self.reg.state_dict()

    def optimizer_state_dict(self) -> dict:
        return adam_state_dict(self.adam, self.adam.step, [mv for layer in self.layers for mv in layer.moments()])
