"""The training loop of the real-vs-fake classifier study (experiments/behavior_net.py:1302-1521) on the HIP kernels of
csrc/seq_cls.hip (include/vunet_seq_cls.h).

``StudyEngine`` holds every net of every start time at once: the trained GRU classifiers (prior, cross and, with a flow, flow
samples against the real sequences: len(kinds) per start time), the never-trained ``class_real_self`` of each start time
(forward on the fake half only), and one regressor per start time.  One training iteration and one final-pass iteration are
each recorded once into a hipGraph and replayed; the batch they read follows a device-resident counter, and every loss and
accuracy stays on the device until ``results`` copies the curves to the host once.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List

import numpy as np
import torch

from . import _lib
from .ops import _call, _graph_recording, _p, _stream
from .seq_train import SeqAdamHp

NIN, KP, HID, G3 = (_lib.const("VUNET_CLS_" + n) for n in ("NIN", "KP", "H", "G"))
OFF_WHH, OFF_BIH, OFF_BHH, OFF_FCW, OFF_FCB = (_lib.const("VUNET_CLS_OFF_" + n) for n in ("WHH", "BIH", "BHH", "FCW", "FCB"))
P = _lib.const("VUNET_CLS_P")            # floats of one classifier's parameter block
MAX_BS = _lib.const("VUNET_CLS_MAX_BS")
KINDS = ("prior", "cross", "flow")


GemmDesc = _lib.struct("vunet_seq_cls_gemm")


def _ptr(t: torch.Tensor, off: int = 0) -> int:
    return t.data_ptr() + 4 * off


def gemm(A, B, C, M, N, K, nets, a, b, c, split=1, c_split=0, bias=None, bias_net=0, mask=None, mask_net=0, mask_m=0, relu=0,
         accumulate=0):
    """C = A . B batched over nets; A, B, C are raw addresses (``_ptr``) and a / b / c their (net, row, column) element strides."""
    d = GemmDesc(A, B, C, bias, mask, a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2], c_split, bias_net, mask_net, mask_m,
                 M, N, K, nets, split, relu, accumulate, 0)
    _call("vunet_seq_cls_gemm_run", ctypes.byref(d), _stream())


def pack_classifier(sd: Dict[str, torch.Tensor]) -> torch.Tensor:
    """A torch-layout state dict of ``Classifier(51, 1)`` (GRU.weight_ih_l0, GRU.weight_hh_l0, GRU.bias_ih_l0, GRU.bias_hh_l0,
    fc1.weight, fc1.bias) -> the kernels' parameter block of P floats."""
    out = torch.zeros(P, dtype=torch.float32)
    wih = torch.zeros(G3, KP)
    wih[:, :NIN] = sd["GRU.weight_ih_l0"].float()
    out[:OFF_WHH] = wih.reshape(-1)
    out[OFF_WHH:OFF_BIH] = sd["GRU.weight_hh_l0"].float().reshape(-1)
    out[OFF_BIH:OFF_BHH] = sd["GRU.bias_ih_l0"].float()
    out[OFF_BHH:OFF_FCW] = sd["GRU.bias_hh_l0"].float()
    out[OFF_FCW:OFF_FCB] = sd["fc1.weight"].float().reshape(-1)
    out[OFF_FCB] = sd["fc1.bias"].float().reshape(())
    return out


def unpack_classifier(block: torch.Tensor) -> Dict[str, torch.Tensor]:
    b = block.detach().cpu()
    return {"GRU.weight_ih_l0": b[:OFF_WHH].reshape(G3, KP)[:, :NIN].clone(), "GRU.weight_hh_l0": b[OFF_WHH:OFF_BIH].reshape(G3, HID).clone(),
            "GRU.bias_ih_l0": b[OFF_BIH:OFF_BHH].clone(), "GRU.bias_hh_l0": b[OFF_BHH:OFF_FCW].clone(),
            "fc1.weight": b[OFF_FCW:OFF_FCB].reshape(1, HID).clone(), "fc1.bias": b[OFF_FCB:OFF_FCB + 1].clone()}


def reg_layout(h: int):
    """Offsets of the regressor's block: fc1 [H/2][H], fc1.b, fc2 [H/4][H/2], fc2.b, fc3 [51][H/4], fc3.b."""
    h2, h4 = h // 2, h // 4
    shapes = [("fc1.weight", (h2, h)), ("fc1.bias", (h2,)), ("fc2.weight", (h4, h2)), ("fc2.bias", (h4,)), ("fc3.weight", (NIN, h4)),
              ("fc3.bias", (NIN,))]
    lay, o = {}, 0
    for k, s in shapes:
        n = int(np.prod(s))
        lay[k] = (o, s)
        o += n
    return lay, o


def pack_regressor(sd: Dict[str, torch.Tensor], h: int) -> torch.Tensor:
    lay, n = reg_layout(h)
    out = torch.zeros(n, dtype=torch.float32)
    for k, (o, s) in lay.items():
        out[o:o + int(np.prod(s))] = sd[k].float().reshape(-1)
    return out


class StudyEngine:
    """All nets of ``classifier_study`` (behavior_eval.py) and their recorded iterations.

    ``sets``: device float32 tensors orig / prior / cross / self [N, T, 51] (flow too, with a flow), ``embed`` [N, H].
    ``cls_blocks`` [n_times, len(kinds) + 1, P] (the trained kinds in KINDS order, then self), ``reg_blocks`` [n_times, Pr]."""

    def __init__(self, sets: Dict[str, torch.Tensor], embed: torch.Tensor, times: List[int], bs: int, iterations: int,
                 cls_blocks: torch.Tensor, reg_blocks: torch.Tensor, split: int = 8):
        dev = embed.device
        self.flow = "flow" in sets
        self.kinds = KINDS if self.flow else KINDS[:2]
        n, t = sets["orig"].shape[:2]
        self.N, self.T, self.bs, self.H = n, t, bs, embed.shape[1]
        self.nb = n // bs
        self.epochs = iterations // self.nb
        self.iters = self.epochs * self.nb
        self.L = self.iters + self.nb
        nt, nk = len(times), len(self.kinds)
        self.nt, self.nk = nt, nk
        self.Gt, self.Gs = nt * nk, nt
        self.S = split
        f32 = dict(device=dev, dtype=torch.float32)
        self.sets = {k: v.to(dev, torch.float32).contiguous() for k, v in sets.items()}
        self.embed = embed.to(dev, torch.float32).contiguous()
        blocks = cls_blocks.to(dev, torch.float32)
        self.params = torch.cat([blocks[:, :nk].reshape(self.Gt, P), blocks[:, nk]], 0).contiguous()   # trained nets, then self
        self.buf = torch.zeros(self.Gt, P, **f32)
        self.grad = torch.zeros(self.Gt, self.S, P, **f32)
        # the pointer tables: trained net s nk + k reads kinds[k] against orig; self net s reads self only
        tab_t = []
        for s in range(nt):
            for k in self.kinds:
                tab_t += [self.sets[k].data_ptr(), self.sets["orig"].data_ptr()]
        self.tab_t = torch.tensor(tab_t, dtype=torch.int64, device=dev)
        self.tab_s = torch.tensor([self.sets["self"].data_ptr(), 0] * nt, dtype=torch.int64, device=dev)
        self.tab_mu = torch.tensor([self.embed.data_ptr(), 0], dtype=torch.int64, device=dev)
        R2, R1 = 2 * bs, bs
        self.grp_t = self._group(self.Gt, R2)
        self.grp_s = self._group(self.Gs, R1)
        self.dh = [torch.zeros(self.Gt, R2 * HID, **f32) for _ in range(2)]
        self.it = torch.zeros(1, dtype=torch.int32, device=dev)
        self.ones = torch.ones(1, **f32)
        self.loss_c = torch.zeros(self.Gt, self.L, **f32)
        self.acc_c = torch.zeros(self.Gt, self.L, **f32)
        self.acc_s = torch.zeros(self.Gs, self.L, **f32)
        # regressors
        lay, pr = reg_layout(self.H)
        self.rlay, self.Pr = lay, pr
        self.rp = reg_blocks.to(dev, torch.float32).reshape(nt, pr).contiguous()
        self.rm, self.rv, self.rg = (torch.zeros(nt, pr, **f32) for _ in range(3))
        h2, h4 = self.H // 2, self.H // 4
        self.mub = torch.zeros(bs * self.H, **f32)
        self.a1, self.da1 = (torch.zeros(nt, bs * h2, **f32) for _ in range(2))
        self.a2, self.da2 = (torch.zeros(nt, bs * h4, **f32) for _ in range(2))
        self.pred, self.dpred = (torch.zeros(nt, bs * KP, **f32) for _ in range(2))
        self.starts = torch.tensor(list(times), dtype=torch.int32, device=dev)
        self.reg_loss = torch.zeros(nt, self.L, **f32)
        self.de = torch.zeros(nt, self.L, **f32)
        self.adam_step = torch.zeros(1, dtype=torch.int64, device=dev)
        self.lr = torch.full((1,), 1e-3, dtype=torch.float64, device=dev)
        self.hp = SeqAdamHp(self.lr.data_ptr(), self.adam_step.data_ptr(), 0.9, 0.999, 1e-8, 0.0, None)
        self.graphs = {}

    def _group(self, nets, R):
        T = self.T
        f32 = dict(device=self.embed.device, dtype=torch.float32)
        gi_net, h_net, xb_net = T * R * G3, (T + 1) * R * HID, T * R * KP
        return dict(nets=nets, R=R, gi_net=gi_net, h_net=h_net, xb_net=xb_net, xb=torch.zeros(nets, xb_net, **f32),
                    gi=torch.zeros(nets, gi_net, **f32), gh=torch.zeros(nets, gi_net, **f32), gates=torch.zeros(nets, gi_net, **f32),
                    h=torch.zeros(nets, h_net, **f32))

    # ---- one iteration, as launches
    def _forward(self, grp, params, R):
        T, nets = self.T, grp["nets"]
        gemm(_ptr(grp["xb"]), _ptr(params), _ptr(grp["gi"]), T * R, G3, KP, nets, (grp["xb_net"], KP, 1), (P, 1, KP), (grp["gi_net"], G3, 1),
             bias=_ptr(params, OFF_BIH), bias_net=P)
        for t in range(T):
            gemm(_ptr(grp["h"], t * R * HID), _ptr(params, OFF_WHH), _ptr(grp["gh"], t * R * G3), R, G3, HID, nets,
                 (grp["h_net"], HID, 1), (P, 1, HID), (grp["gi_net"], G3, 1), bias=_ptr(params, OFF_BHH), bias_net=P)
            _call("vunet_seq_cls_cell_fwd", _p(grp["gi"]), _p(grp["gh"]), _p(grp["gates"]), _p(grp["h"]), nets, T, R, t, grp["gi_net"],
                  grp["h_net"], _stream())

    def _backward(self):
        grp, T, R, nets = self.grp_t, self.T, 2 * self.bs, self.Gt
        params = self.params
        cur, nxt = self.dh
        for t in range(T - 1, -1, -1):
            _call("vunet_seq_cls_cell_bwd", _p(grp["gi"]), _p(grp["gh"]), _p(grp["gates"]), _p(grp["h"]), _p(cur), _p(nxt), nets, T, R, t,
                  grp["gi_net"], grp["h_net"], R * HID, _stream())
            if t > 0:
                gemm(_ptr(grp["gh"], t * R * G3), _ptr(params, OFF_WHH), _ptr(nxt), R, HID, G3, nets, (grp["gi_net"], G3, 1), (P, HID, 1),
                     (R * HID, HID, 1), accumulate=1)
            cur, nxt = nxt, cur
        # weight and bias gradients over all T R rows: S slices of the reduction, summed by the SGD kernel in slice order
        K, gn, S = T * R, self.S * P, self.S
        gemm(_ptr(grp["gi"]), _ptr(grp["xb"]), _ptr(self.grad), G3, KP, K, nets, (grp["gi_net"], 1, G3), (grp["xb_net"], KP, 1), (gn, KP, 1),
             split=S, c_split=P)
        gemm(_ptr(grp["gh"]), _ptr(grp["h"]), _ptr(self.grad, OFF_WHH), G3, HID, K, nets, (grp["gi_net"], 1, G3), (grp["h_net"], HID, 1),
             (gn, HID, 1), split=S, c_split=P)
        gemm(_ptr(grp["gi"]), _ptr(self.ones), _ptr(self.grad, OFF_BIH), G3, 1, K, nets, (grp["gi_net"], 1, G3), (0, 0, 0), (gn, 1, 1),
             split=S, c_split=P)
        gemm(_ptr(grp["gh"]), _ptr(self.ones), _ptr(self.grad, OFF_BHH), G3, 1, K, nets, (grp["gi_net"], 1, G3), (0, 0, 0), (gn, 1, 1),
             split=S, c_split=P)
        _call("vunet_seq_cls_sgd", _p(params), _p(self.grad), _p(self.buf), nets, S, ctypes.c_float(1e-3), ctypes.c_float(0.9), _p(self.it),
              _stream())

    def _regressor(self, final: bool):
        bs, H, nt = self.bs, self.H, self.nt
        h2, h4 = H // 2, H // 4
        lay, pr = self.rlay, self.Pr
        o = {k: v[0] for k, v in lay.items()}
        rp, rg = self.rp, self.rg
        gemm(_ptr(self.mub), _ptr(rp, o["fc1.weight"]), _ptr(self.a1), bs, h2, H, nt, (0, H, 1), (pr, 1, H), (bs * h2, h2, 1),
             bias=_ptr(rp, o["fc1.bias"]), bias_net=pr, relu=1)
        gemm(_ptr(self.a1), _ptr(rp, o["fc2.weight"]), _ptr(self.a2), bs, h4, h2, nt, (bs * h2, h2, 1), (pr, 1, h2), (bs * h4, h4, 1),
             bias=_ptr(rp, o["fc2.bias"]), bias_net=pr, relu=1)
        gemm(_ptr(self.a2), _ptr(rp, o["fc3.weight"]), _ptr(self.pred), bs, NIN, h4, nt, (bs * h4, h4, 1), (pr, 1, h4), (bs * KP, KP, 1),
             bias=_ptr(rp, o["fc3.bias"]), bias_net=pr)
        _call("vunet_seq_cls_reg_loss", _p(self.pred), KP, bs * KP, _p(self.sets["orig"]), _p(self.sets["cross"]) if final else None, self.T,
              bs, self.nb, _p(self.starts), _p(self.it), 0, _p(self.reg_loss), _p(self.de), self.L, _p(self.dpred), nt, _stream())
        gemm(_ptr(self.dpred), _ptr(self.a2), _ptr(rg, o["fc3.weight"]), NIN, h4, bs, nt, (bs * KP, 1, KP), (bs * h4, h4, 1), (pr, h4, 1))
        gemm(_ptr(self.dpred), _ptr(self.ones), _ptr(rg, o["fc3.bias"]), NIN, 1, bs, nt, (bs * KP, 1, KP), (0, 0, 0), (pr, 1, 1))
        gemm(_ptr(self.dpred), _ptr(rp, o["fc3.weight"]), _ptr(self.da2), bs, h4, NIN, nt, (bs * KP, KP, 1), (pr, h4, 1), (bs * h4, h4, 1),
             mask=_ptr(self.a2), mask_net=bs * h4, mask_m=h4)
        gemm(_ptr(self.da2), _ptr(self.a1), _ptr(rg, o["fc2.weight"]), h4, h2, bs, nt, (bs * h4, 1, h4), (bs * h2, h2, 1), (pr, h2, 1))
        gemm(_ptr(self.da2), _ptr(self.ones), _ptr(rg, o["fc2.bias"]), h4, 1, bs, nt, (bs * h4, 1, h4), (0, 0, 0), (pr, 1, 1))
        gemm(_ptr(self.da2), _ptr(rp, o["fc2.weight"]), _ptr(self.da1), bs, h2, h4, nt, (bs * h4, h4, 1), (pr, h2, 1), (bs * h2, h2, 1),
             mask=_ptr(self.a1), mask_net=bs * h2, mask_m=h2)
        gemm(_ptr(self.da1), _ptr(self.mub), _ptr(rg, o["fc1.weight"]), h2, H, bs, nt, (bs * h2, 1, h2), (0, H, 1), (pr, H, 1))
        gemm(_ptr(self.da1), _ptr(self.ones), _ptr(rg, o["fc1.bias"]), h2, 1, bs, nt, (bs * h2, 1, h2), (0, 0, 0), (pr, 1, 1))
        _call("vunet_seq_cls_tick", None, _p(self.adam_step), _stream())
        _call("vunet_seq_cls_adam", _p(rp), _p(self.rm), _p(self.rv), _p(rg), nt, pr, ctypes.byref(self.hp), _stream())

    def _iteration(self, final: bool):
        bs, T, nb = self.bs, self.T, self.nb
        R = bs if final else 2 * bs
        gt, gs = self.grp_t, self.grp_s
        _call("vunet_seq_cls_gather", _p(self.tab_t), self.Gt, T, NIN, KP, bs, nb, 0 if final else 1, _p(self.it), _p(gt["xb"]), gt["xb_net"],
              _stream())
        _call("vunet_seq_cls_gather", _p(self.tab_s), self.Gs, T, NIN, KP, bs, nb, 0, _p(self.it), _p(gs["xb"]), gs["xb_net"], _stream())
        _call("vunet_seq_cls_gather", _p(self.tab_mu), 1, 1, self.H, self.H, bs, nb, 0, _p(self.it), _p(self.mub), bs * self.H, _stream())
        pt = self.params
        ps = self.params[self.Gt:]
        self._forward(gt, pt, R)
        self._forward(gs, ps, bs)
        h_t = gt["h"][:, T * R * HID:]
        _call("vunet_seq_cls_head", _p(h_t), gt["h_net"], _p(pt), self.Gt, bs, 0 if final else 1, _p(self.it), 0, _p(self.loss_c),
              _p(self.acc_c), self.L, None if final else _p(self.dh[0]), None if final else _p(self.grad), self.S * P, _stream())
        _call("vunet_seq_cls_head", _p(gs["h"][:, T * bs * HID:]), gs["h_net"], _p(ps), self.Gs, bs, 0, _p(self.it), 0, None, _p(self.acc_s),
              self.L, None, None, 0, _stream())
        if not final:
            self._backward()
        self._regressor(final)
        _call("vunet_seq_cls_tick", _p(self.it), None, _stream())

    def step(self, final: bool, graph: bool = True):
        if not graph:
            self._iteration(final)
            return
        g = self.graphs.get(final)
        if g is None:
            g = torch.cuda.CUDAGraph()
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with _graph_recording(g, s):
                self._iteration(final)
            torch.cuda.current_stream().wait_stream(s)
            self.graphs[final] = g
        g.replay()

    def run(self, graph: bool = True):
        for _ in range(self.iters):
            self.step(False, graph)
        for _ in range(self.nb):
            self.step(True, graph)

    def results(self):
        """The curves, one device-to-host copy: (loss_c [Gt, L], acc_c [Gt, L], acc_s [Gs, L], reg_loss [nt, L], de [nt, L])."""
        flat = torch.cat([self.loss_c.reshape(-1), self.acc_c.reshape(-1), self.acc_s.reshape(-1), self.reg_loss.reshape(-1),
                          self.de.reshape(-1)]).cpu().numpy()
        out, o = [], 0
        for shape in ((self.Gt, self.L), (self.Gt, self.L), (self.Gs, self.L), (self.nt, self.L), (self.nt, self.L)):
            n = shape[0] * shape[1]
            out.append(flat[o:o + n].reshape(shape))
            o += n
        return out
