"""Inference-only Inception-v3 on the GPU: what the reference takes from torchvision for its FID and Inception score
(``models/imagenet_pretrained.py:64-111`` FIDInceptionModel, ``lib/metrics.py:381`` ``inception_v3(pretrained=True,
transform_input=False)``).  torchvision is a third-party dependency of the reference, absent here: the topology of its
``Inception3`` (without ``AuxLogits``) is restated with torchvision's state-dict key names, so a user-supplied ``inception_v3``
state dict loads key for key.

The device sees convolution + bias + ReLU only: every ``BasicConv2d`` (conv without bias -> BatchNorm2d(eps=1e-3) in eval form
-> ReLU) is folded in float64 on the host, once per parameter version, and packed K-major for ``vunet_convg``
(csrc/inception.hip, include/vunet_inception.h): an implicit GEMM on the fp32 matrix instruction.  The last convolution of
every branch stores into its channel slice of the block's output (no ``torch.cat``); the pools are ``vunet_pool2d``.  A forward is
a fixed list of launches on the current stream -- the PLAN, built once per (N, H, W): descriptors and offsets into one arena;
nothing is allocated after the first call at a shape.

ASSUMPTION (unpinned): ``stem_pool="avg"``.  The reference's FIDInceptionModel loops over ``v3._modules`` and applies
``F.avg_pool2d(3, 2)`` after ``Conv2d_2b_3x3`` and ``Conv2d_4a_3x3``.  With torchvision 0.4.x -- the version paired with the
reference's pinned pytorch 1.3.1 -- the two stem max-pools are functional calls inside ``Inception3.forward``, so that loop never
sees them and the average pools stand IN THEIR PLACE; ``transform_input`` is bypassed alike.  From torchvision 0.6 on the
max-pools are modules (``maxpool1`` / ``maxpool2``) and the same loop would pool twice.  torchvision is not installed, so neither
the version nor the pretrained weights are pinned here.
"""
from __future__ import annotations

import ctypes
import math
from collections import OrderedDict
from typing import Dict, List, Optional, Tuple

import torch
from torch import nn

from .. import _lib, ops
from ..ops import _call, _p, _stream

BN_EPS = 1e-3
SIZE = _lib.const("VUNET_INCEPTION_SIZE")
MIN_SIZE = 75                   # the smallest input whose maps reach 1 x 1 at Mixed_7a
KC, MT = _lib.const("VUNET_CONVG_KC"), _lib.const("VUNET_CONVG_MT")   # the packing's K and M padding
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
INPUT_MODES = {"none": 0, "transform": 1, "fid": 2}
N_FEATURES, N_CLASSES = 2048, 1000


ConvgDesc = _lib.struct("vunet_convg_desc")
Pool2dDesc = _lib.struct("vunet_pool2d_desc")


def _pair(v) -> Tuple[int, int]:
    return (v, v) if isinstance(v, int) else (int(v[0]), int(v[1]))


def _out(size: int, k: int, s: int, p: int) -> int:
    return (size + 2 * p - k) // s + 1


# ------------------------------------------------------------------------------------------------
# The topology: torchvision's Inception3 without AuxLogits.  name -> (cin, cout, kernel, stride, pad), in torchvision's order.
# ------------------------------------------------------------------------------------------------
BLOCKS = (("Mixed_5b", "A", 192, 32), ("Mixed_5c", "A", 256, 64), ("Mixed_5d", "A", 288, 64), ("Mixed_6a", "B", 288, 0),
          ("Mixed_6b", "C", 768, 128), ("Mixed_6c", "C", 768, 160), ("Mixed_6d", "C", 768, 160), ("Mixed_6e", "C", 768, 192),
          ("Mixed_7a", "D", 768, 0), ("Mixed_7b", "E", 1280, 0), ("Mixed_7c", "E", 2048, 0))
BLOCK_OUT = {"Mixed_5b": 256, "Mixed_5c": 288, "Mixed_5d": 288, "Mixed_6a": 768, "Mixed_6b": 768, "Mixed_6c": 768, "Mixed_6d": 768,
             "Mixed_6e": 768, "Mixed_7a": 1280, "Mixed_7b": 2048, "Mixed_7c": 2048}


def conv_specs() -> "OrderedDict[str, tuple]":
    L: "OrderedDict[str, tuple]" = OrderedDict()

    def add(name, cin, cout, k, s=1, p=0):
        L[name] = (cin, cout, _pair(k), _pair(s), _pair(p))
    add("Conv2d_1a_3x3", 3, 32, 3, 2)
    add("Conv2d_2a_3x3", 32, 32, 3)
    add("Conv2d_2b_3x3", 32, 64, 3, 1, 1)
    add("Conv2d_3b_1x1", 64, 80, 1)
    add("Conv2d_4a_3x3", 80, 192, 3)
    for name, kind, cin, arg in BLOCKS:
        if kind == "A":
            add(f"{name}.branch1x1", cin, 64, 1)
            add(f"{name}.branch5x5_1", cin, 48, 1)
            add(f"{name}.branch5x5_2", 48, 64, 5, 1, 2)
            add(f"{name}.branch3x3dbl_1", cin, 64, 1)
            add(f"{name}.branch3x3dbl_2", 64, 96, 3, 1, 1)
            add(f"{name}.branch3x3dbl_3", 96, 96, 3, 1, 1)
            add(f"{name}.branch_pool", cin, arg, 1)
        elif kind == "B":
            add(f"{name}.branch3x3", cin, 384, 3, 2)
            add(f"{name}.branch3x3dbl_1", cin, 64, 1)
            add(f"{name}.branch3x3dbl_2", 64, 96, 3, 1, 1)
            add(f"{name}.branch3x3dbl_3", 96, 96, 3, 2)
        elif kind == "C":
            c7 = arg
            add(f"{name}.branch1x1", cin, 192, 1)
            add(f"{name}.branch7x7_1", cin, c7, 1)
            add(f"{name}.branch7x7_2", c7, c7, (1, 7), 1, (0, 3))
            add(f"{name}.branch7x7_3", c7, 192, (7, 1), 1, (3, 0))
            add(f"{name}.branch7x7dbl_1", cin, c7, 1)
            add(f"{name}.branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0))
            add(f"{name}.branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3))
            add(f"{name}.branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0))
            add(f"{name}.branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3))
            add(f"{name}.branch_pool", cin, 192, 1)
        elif kind == "D":
            add(f"{name}.branch3x3_1", cin, 192, 1)
            add(f"{name}.branch3x3_2", 192, 320, 3, 2)
            add(f"{name}.branch7x7x3_1", cin, 192, 1)
            add(f"{name}.branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3))
            add(f"{name}.branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0))
            add(f"{name}.branch7x7x3_4", 192, 192, 3, 2)
        else:
            add(f"{name}.branch1x1", cin, 320, 1)
            add(f"{name}.branch3x3_1", cin, 384, 1)
            add(f"{name}.branch3x3_2a", 384, 384, (1, 3), 1, (0, 1))
            add(f"{name}.branch3x3_2b", 384, 384, (3, 1), 1, (1, 0))
            add(f"{name}.branch3x3dbl_1", cin, 448, 1)
            add(f"{name}.branch3x3dbl_2", 448, 384, 3, 1, 1)
            add(f"{name}.branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1))
            add(f"{name}.branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0))
            add(f"{name}.branch_pool", cin, 192, 1)
    return L


SPECS = conv_specs()


# ------------------------------------------------------------------------------------------------
# Folding and packing (host, float64)
# ------------------------------------------------------------------------------------------------
def fold_bn(w, gamma, beta, mean, var, eps: float = BN_EPS):
    """conv(bias=False) -> BatchNorm2d in eval form as ONE convolution with bias, in float64:
    ``w' = w gamma / sqrt(var + eps)``, ``b' = beta - mean gamma / sqrt(var + eps)``."""
    s = gamma.double() / torch.sqrt(var.double() + eps)
    return w.double() * s.view(-1, 1, 1, 1), beta.double() - mean.double() * s


def fold_input_affine(w, b, scale, shift):
    """A per-channel ``x_c scale_c + shift_c`` in front of an UNPADDED convolution, folded into it (float64): exact, since
    without padding every tap reads a transformed pixel."""
    scale, shift = torch.as_tensor(scale, dtype=torch.float64), torch.as_tensor(shift, dtype=torch.float64)
    return w * scale.view(1, -1, 1, 1), b + (w * shift.view(1, -1, 1, 1)).sum(dim=(1, 2, 3))


def pack_weight(w) -> torch.Tensor:
    """[M, C, KH, KW] -> the K-major image ``vunet_convg`` reads: fp32 [Kpad, Mpad], row ``(c KH + kh) KW + kw``, zero-padded to
    multiples of 64 rows and 64 columns (so the kernel's weight loads need no bounds checks)."""
    m, k = int(w.shape[0]), int(w[0].numel())
    out = torch.zeros(-(-k // KC) * KC, -(-m // MT) * MT, dtype=torch.float32)
    out[:k, :m] = w.reshape(m, k).t().to(torch.float32)
    return out


# ------------------------------------------------------------------------------------------------
# Modules (parameter containers with torchvision's key names; never called)
# ------------------------------------------------------------------------------------------------
class BasicConv2d(nn.Module):
    def __init__(self, cin, cout, k, s, p):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, stride=s, padding=p, bias=False)
        self.bn = nn.BatchNorm2d(cout, eps=BN_EPS)


class _Block(nn.Module):
    pass


class _Step:
    """One launch of a plan: ``fn`` in ("conv", "pool", "gap", "input", "input_boxes"), its descriptor, arena offsets (floats; ``src`` None = the
    caller's tensor) and for a convolution the layer whose packed weights it reads."""
    __slots__ = ("fn", "desc", "src", "dst", "layer", "args", "label")

    def __init__(self, fn, desc, src, dst, layer=None, args=(), label=""):
        self.fn, self.desc, self.src, self.dst, self.layer, self.args, self.label = fn, desc, src, dst, layer, args, label


class Plan:
    """The launches of one forward at (N, H, W): ``steps``, the arena size in floats, and where the results are.  Pure host
    arithmetic (no device needed): buffers are offsets into one arena -- the outputs of the stem layers and of the blocks one after
    the other, then a scratch region that the temporaries of each block share (a block's launches are in stream order, and its
    temporaries are dead when the next block starts)."""

    def __init__(self, n: int, h: int, w: int, stem_pool: str = "max", resize_mode: Optional[str] = None, logits: bool = True,
                 boxed: Optional[Tuple[int, int]] = None):
        if stem_pool not in ("max", "avg"):
            raise ValueError(f"stem_pool: 'max' or 'avg' expected, got {stem_pool!r}")
        self.n = int(n)
        self.steps: List[_Step] = []
        self.map_sizes: List[Tuple[int, int]] = []      # after each stem conv / pool and each grid-size change
        self.block_out: Dict[str, Tuple[int, int, int]] = {}
        self.block_slices: Dict[str, List[Tuple[int, int]]] = {}   # block -> (channel offset, channels) of each branch, in order
        self._top, self._scratch, self._scratch_max = 0, 0, 0
        self._bufs: List[list] = []
        n = self.n
        src = None
        if resize_mode is not None:
            x0 = self._buf(3, SIZE, SIZE)
            if boxed is None:
                self.steps.append(_Step("input", None, None, x0, args=(n, int(h), int(w), INPUT_MODES[resize_mode]), label="input"))
            else:   # (crop size, sampling code): the person-box crop and the resize in one launch; boxes / valid come with the call
                self.steps.append(_Step("input_boxes", None, None, x0, args=(n, int(h), int(w), int(boxed[0]), int(boxed[1]),
                                                                             INPUT_MODES[resize_mode]), label="input_boxes"))
            src, h, w = x0, SIZE, SIZE
        elif boxed is not None:
            raise ValueError("a boxed plan crops inside the resize step: it needs a resize mode")
        if h < MIN_SIZE or w < MIN_SIZE:
            raise ValueError(f"Inception-v3 needs H, W >= {MIN_SIZE}, got {h} x {w}")
        cur = (src, 3, h, w)       # (buffer, channels, h, w)
        pool_mode = 0 if stem_pool == "max" else 1
        cur = self._conv_new("Conv2d_1a_3x3", cur); self.map_sizes.append(cur[2:])
        cur = self._conv_new("Conv2d_2a_3x3", cur); self.map_sizes.append(cur[2:])
        cur = self._conv_new("Conv2d_2b_3x3", cur); self.map_sizes.append(cur[2:])
        cur = self._pool_new(cur, 2, 0, pool_mode, "stem_pool1"); self.map_sizes.append(cur[2:])
        cur = self._conv_new("Conv2d_3b_1x1", cur); self.map_sizes.append(cur[2:])
        cur = self._conv_new("Conv2d_4a_3x3", cur); self.map_sizes.append(cur[2:])
        cur = self._pool_new(cur, 2, 0, pool_mode, "stem_pool2"); self.map_sizes.append(cur[2:])
        for name, kind, cin, _ in BLOCKS:
            assert cur[1] == cin, (name, cur[1], cin)
            cur = getattr(self, "_block_" + kind)(name, cur)
            self.block_out[name] = cur[1:]
            self.map_sizes.append(cur[2:])
            self._scratch_max, self._scratch = max(self._scratch_max, self._scratch), 0
        feat = self._buf(N_FEATURES, 1, 1)
        self.steps.append(_Step("gap", None, cur[0], feat, args=(n * N_FEATURES, cur[2] * cur[3]), label="global_avgpool"))
        self.features_off, self.logits_off = feat, None
        if logits:
            self.logits_off = self._conv_new("fc", (feat, N_FEATURES, 1, 1), relu=False)[0]
        # scratch offsets were counted from 0: move them behind the persistent buffers
        base = self._top
        for b in self._bufs:
            if b[1]:
                b[0] += base
        for st in self.steps:
            st.src = None if st.src is None else st.src[0]
            st.dst = st.dst[0]
        self.features_off = self.features_off[0]
        self.logits_off = None if self.logits_off is None else self.logits_off[0]
        self.arena_floats = base + self._scratch_max

    # ---- buffers: a one-element-list offset (patched once the persistent size is known), scratch flag
    def _buf(self, c, h, w, scratch=False):
        size = -(-self.n * c * h * w // 64) * 64
        if scratch:
            b = [self._scratch, True]
            self._scratch += size
        else:
            b = [self._top, False]
            self._top += size
        self._bufs.append(b)
        return b

    def _conv(self, layer, src, dst, dst_ctot, dst_coff, relu=True):
        """src = (buffer, ctot, h, w[, coff, c]): the convolution ``layer`` from a channel slice of src into a slice of dst."""
        cin, cout, (kh, kw), (sh, sw), (ph, pw) = SPECS[layer] if layer != "fc" else (N_FEATURES, N_CLASSES, (1, 1), (1, 1), (0, 0))
        buf, ctot, h, w = src[:4]
        coff, c = (src[4], src[5]) if len(src) > 4 else (0, ctot)
        assert c == cin, (layer, c, cin)
        ho, wo = _out(h, kh, sh, ph), _out(w, kw, sw, pw)
        k = cin * kh * kw
        d = ConvgDesc(self.n, cin, h, w, cout, ho, wo, kh, kw, sh, sw, ph, pw, ctot, coff, dst_ctot, dst_coff, int(relu),
                      -(-k // KC) * KC, -(-cout // MT) * MT, 0)
        self.steps.append(_Step("conv", d, buf, dst, layer=layer, label=layer))
        return ho, wo

    def _conv_new(self, layer, src, relu=True, scratch=False):
        cin, cout, (kh, kw), (sh, sw), (ph, pw) = SPECS[layer] if layer != "fc" else (N_FEATURES, N_CLASSES, (1, 1), (1, 1), (0, 0))
        ho, wo = _out(src[2], kh, sh, ph), _out(src[3], kw, sw, pw)
        dst = self._buf(cout, ho, wo, scratch)
        self._conv(layer, src, dst, cout, 0, relu)
        return (dst, cout, ho, wo)

    def _pool(self, src, dst, dst_ctot, dst_coff, stride, pad, mode, label):
        buf, c, h, w = src
        ho, wo = _out(h, 3, stride, pad), _out(w, 3, stride, pad)
        d = Pool2dDesc(self.n, c, h, w, ho, wo, stride, pad, mode, c, 0, dst_ctot, dst_coff)
        self.steps.append(_Step("pool", d, buf, dst, label=label))
        return ho, wo

    def _pool_new(self, src, stride, pad, mode, label, scratch=False):
        _, c, h, w = src
        ho, wo = _out(h, 3, stride, pad), _out(w, 3, stride, pad)
        dst = self._buf(c, ho, wo, scratch)
        self._pool(src, dst, c, 0, stride, pad, mode, label)
        return (dst, c, ho, wo)

    def _chain(self, name, layers, src, out, ctot, coff):
        """``layers`` of block ``name`` one after the other: all but the last into scratch, the last into the slice of ``out``."""
        cur = src
        for l in layers[:-1]:
            cur = self._conv_new(f"{name}.{l}", cur, scratch=True)
        self._conv(f"{name}.{layers[-1]}", cur, out, ctot, coff)
        cout = SPECS[f"{name}.{layers[-1]}"][1]
        self.block_slices.setdefault(name, []).append((coff, cout))
        return coff + cout

    def _block_A(self, name, src):
        _, cin, h, w = src
        ctot = BLOCK_OUT[name]
        out = self._buf(ctot, h, w)
        off = self._chain(name, ["branch1x1"], src, out, ctot, 0)
        off = self._chain(name, ["branch5x5_1", "branch5x5_2"], src, out, ctot, off)
        off = self._chain(name, ["branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"], src, out, ctot, off)
        pooled = self._pool_new(src, 1, 1, 1, name + ".avg_pool", scratch=True)
        off = self._chain(name, ["branch_pool"], pooled, out, ctot, off)
        assert off == ctot
        return (out, ctot, h, w)

    def _block_B(self, name, src):
        _, cin, h, w = src
        ctot, ho, wo = BLOCK_OUT[name], _out(h, 3, 2, 0), _out(w, 3, 2, 0)
        out = self._buf(ctot, ho, wo)
        off = self._chain(name, ["branch3x3"], src, out, ctot, 0)
        off = self._chain(name, ["branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"], src, out, ctot, off)
        self._pool(src, out, ctot, off, 2, 0, 0, name + ".max_pool")
        self.block_slices[name].append((off, cin))
        assert off + cin == ctot
        return (out, ctot, ho, wo)

    def _block_C(self, name, src):
        _, cin, h, w = src
        ctot = BLOCK_OUT[name]
        out = self._buf(ctot, h, w)
        off = self._chain(name, ["branch1x1"], src, out, ctot, 0)
        off = self._chain(name, ["branch7x7_1", "branch7x7_2", "branch7x7_3"], src, out, ctot, off)
        off = self._chain(name, ["branch7x7dbl_%d" % i for i in range(1, 6)], src, out, ctot, off)
        pooled = self._pool_new(src, 1, 1, 1, name + ".avg_pool", scratch=True)
        off = self._chain(name, ["branch_pool"], pooled, out, ctot, off)
        assert off == ctot
        return (out, ctot, h, w)

    def _block_D(self, name, src):
        _, cin, h, w = src
        ctot, ho, wo = BLOCK_OUT[name], _out(h, 3, 2, 0), _out(w, 3, 2, 0)
        out = self._buf(ctot, ho, wo)
        off = self._chain(name, ["branch3x3_1", "branch3x3_2"], src, out, ctot, 0)
        off = self._chain(name, ["branch7x7x3_%d" % i for i in range(1, 5)], src, out, ctot, off)
        self._pool(src, out, ctot, off, 2, 0, 0, name + ".max_pool")
        self.block_slices[name].append((off, cin))
        assert off + cin == ctot
        return (out, ctot, ho, wo)

    def _block_E(self, name, src):
        _, cin, h, w = src
        ctot = BLOCK_OUT[name]
        out = self._buf(ctot, h, w)
        off = self._chain(name, ["branch1x1"], src, out, ctot, 0)
        b3 = self._conv_new(f"{name}.branch3x3_1", src, scratch=True)
        off = self._chain(name, ["branch3x3_2a"], b3, out, ctot, off)
        off = self._chain(name, ["branch3x3_2b"], b3, out, ctot, off)
        bd = self._conv_new(f"{name}.branch3x3dbl_1", src, scratch=True)
        bd = self._conv_new(f"{name}.branch3x3dbl_2", bd, scratch=True)
        off = self._chain(name, ["branch3x3dbl_3a"], bd, out, ctot, off)
        off = self._chain(name, ["branch3x3dbl_3b"], bd, out, ctot, off)
        pooled = self._pool_new(src, 1, 1, 1, name + ".avg_pool", scratch=True)
        off = self._chain(name, ["branch_pool"], pooled, out, ctot, off)
        assert off == ctot
        return (out, ctot, h, w)


class InceptionV3(nn.Module):
    """torchvision's ``inception_v3(aux_logits=False)``, inference only.  ``forward(x)``: [N, 3, H, W] fp32 on the GPU, H, W >= 75
    -> logits [N, 1000]; ``features(x)`` -> the pooled ``Mixed_7c`` output [N, 2048].  ``state_dict``: a torchvision-format state
    dict (``AuxLogits.*`` keys are dropped, as torchvision does for ``aux_logits=False``); None: seeded random weights that keep
    the activations O(1) (tests, timing).  ``transform_input``: torchvision's per-channel re-normalisation
    ``x_c (std_c / 0.5) + (mean_c - 0.5) / 0.5`` first -- folded into ``Conv2d_1a_3x3`` (unpadded, so the fold is exact).
    ``stem_pool``: "max" (torchvision) or "avg" (what FIDInceptionModel computes: see the module header).

    The returned tensors are views into the plan's arena: valid until the next call at the same shape."""

    def __init__(self, state_dict=None, transform_input: bool = False, stem_pool: str = "max", seed: int = 1234):
        super().__init__()
        if stem_pool not in ("max", "avg"):
            raise ValueError(f"stem_pool: 'max' or 'avg' expected, got {stem_pool!r}")
        self.transform_input, self.stem_pool = bool(transform_input), stem_pool
        for name, (cin, cout, k, s, p) in SPECS.items():
            parent, _, leaf = name.rpartition(".")
            holder = self
            if parent:
                if parent not in self._modules:
                    self.add_module(parent, _Block())
                holder = self._modules[parent]
            holder.add_module(leaf, BasicConv2d(cin, cout, k, s, p))
        self.fc = nn.Linear(N_FEATURES, N_CLASSES)
        for p in self.parameters():
            p.requires_grad_(False)
        self.__dict__["_packs"] = {}
        self.__dict__["_plans"] = {}
        nn.Module.train(self, False)
        if state_dict is None:
            self.init_synthetic(seed)
        else:
            self.load_state_dict(state_dict)

    # ---- parameters
    def init_synthetic(self, seed: int = 1234):
        """Seeded weights: He-normal convolutions, batch-norm statistics near the identity (gamma, var in [0.8, 1.2], beta, mean
        in [-0.1, 0.1]) -- activations stay O(1) through the 94 layers."""
        g = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for name in SPECS:
                m = self.layer(name)
                k = m.conv.weight[0].numel()
                m.conv.weight.copy_(torch.randn(m.conv.weight.shape, generator=g) * math.sqrt(2.0 / k))
                c = m.bn.weight.shape[0]
                m.bn.weight.copy_(0.8 + 0.4 * torch.rand(c, generator=g))
                m.bn.running_var.copy_(0.8 + 0.4 * torch.rand(c, generator=g))
                m.bn.bias.copy_(0.2 * torch.rand(c, generator=g) - 0.1)
                m.bn.running_mean.copy_(0.2 * torch.rand(c, generator=g) - 0.1)
            self.fc.weight.copy_(torch.randn(self.fc.weight.shape, generator=g) / math.sqrt(N_FEATURES))
            self.fc.bias.copy_(0.2 * torch.rand(N_CLASSES, generator=g) - 0.1)
        return self

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        return super().load_state_dict({k: v for k, v in state_dict.items() if not k.startswith("AuxLogits.")}, strict=strict, **kw)

    def layer(self, name: str) -> BasicConv2d:
        m = self
        for part in name.split("."):
            m = m._modules[part]
        return m

    def train(self, mode: bool = True):
        if mode:
            raise RuntimeError("InceptionV3 is inference only: batch norm is folded into the convolutions (eval form), there is no "
                               "training path")
        return super().train(False)

    # ---- packed weights
    def _pack(self, name: str, device):
        if name == "fc":
            params = (self.fc.weight, self.fc.bias)
        else:
            m = self.layer(name)
            params = (m.conv.weight, m.bn.weight, m.bn.bias, m.bn.running_mean, m.bn.running_var)
        stamp = ops._versions(params)
        hit = self._packs.get(name)
        if hit is not None and hit[0] == stamp:
            return hit
        host = [t.detach().cpu() for t in params]
        if name == "fc":
            w, b = host[0].double().view(N_CLASSES, N_FEATURES, 1, 1), host[1].double()
        else:
            w, b = fold_bn(*host)
        if name == "Conv2d_1a_3x3" and self.transform_input:
            w, b = fold_input_affine(w, b, [s / 0.5 for s in STD], [(m_ - 0.5) / 0.5 for m_ in MEAN])
        hit = (stamp, pack_weight(w).to(device), b.to(torch.float32).to(device))
        self._packs[name] = hit
        return hit

    # ---- plans
    def plan(self, n: int, h: int, w: int, resize_mode: Optional[str] = None, boxed: Optional[Tuple[int, int]] = None) -> Plan:
        return Plan(n, h, w, self.stem_pool, resize_mode, boxed=boxed)

    def _bound_plan(self, x, resize_mode, boxed=None):
        n, _, h, w = x.shape
        key = (n, h, w, resize_mode, x.device.index, _stream().value)
        if boxed is not None:   # a plan (and an arena) of its own: the plain plans keep their keys
            key = key + ("boxes",) + tuple(boxed)
        rec = self._plans.get(key)
        if rec is None:
            plan = self.plan(n, h, w, resize_mode, boxed)
            arena = torch.empty(plan.arena_floats, device=x.device, dtype=torch.float32)
            rec = self._plans[key] = (plan, arena)
        return rec

    def _boxed(self, x, resize_mode, boxes, valid, crop_size, sampling):
        """The checked box arguments of a call: None without boxes, else ((crop size, sampling code), boxes, valid)."""
        if boxes is None:
            if valid is not None or crop_size is not None:
                raise ValueError("valid / crop_size come with boxes")
            return None
        from .. import person_crop
        if resize_mode is None:
            raise ValueError("boxes are cropped inside the resize-to-299 launch: pass resize=True")
        if crop_size is None or int(crop_size) < 2:
            raise ValueError(f"boxes need crop_size >= 2 (the side the reference resizes the crop to), got {crop_size}")
        boxes, valid = person_crop._boxes_device(x, boxes, valid)
        return (int(crop_size), person_crop._sampling(sampling)), boxes, valid

    def _run(self, x, resize_mode=None, upto_features=False, on_step=None, boxes=None, valid=None, crop_size=None,
             sampling="reference"):
        if not (torch.is_tensor(x) and x.is_cuda):
            raise RuntimeError("InceptionV3 needs device tensors (hand-written gfx950 kernels; no CPU fallback)")
        if x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"fp32 [N, 3, H, W] expected, got {x.dtype} {tuple(x.shape)}")
        if any(p.device != x.device for p in (self.fc.weight, self.Conv2d_1a_3x3.conv.weight)):
            raise RuntimeError("InceptionV3 and its input are on different devices (model.cuda() first)")
        x = x.contiguous()
        boxed = self._boxed(x, resize_mode, boxes, valid, crop_size, sampling)
        with torch.cuda.device(x.device):
            plan, arena = self._bound_plan(x, resize_mode, None if boxed is None else boxed[0])
            base, stream = arena.data_ptr(), _stream()

            def at(off):
                return ctypes.c_void_p(x.data_ptr() if off is None else base + 4 * off)
            for st in plan.steps:
                if upto_features and st.layer == "fc":
                    break
                if on_step is not None:
                    on_step(st, False)
                if st.fn == "conv":
                    _, wp, b = self._pack(st.layer, x.device)
                    _call("vunet_convg", ctypes.byref(st.desc), at(st.src), _p(wp), _p(b), at(st.dst), stream)
                elif st.fn == "pool":
                    _call("vunet_pool2d", ctypes.byref(st.desc), at(st.src), at(st.dst), stream)
                elif st.fn == "gap":
                    _call("vunet_global_avgpool", at(st.src), at(st.dst), *st.args, stream)
                elif st.fn == "input":
                    _call("vunet_inception_input", at(st.src), at(st.dst), *st.args, stream)
                else:
                    n_, h_, w_, size_, smp_, mode_ = st.args
                    _call("vunet_inception_input_boxes", at(st.src), n_, h_, w_, _p(boxed[1]), _p(boxed[2]), size_, smp_, mode_,
                          at(st.dst), stream)
                if on_step is not None:
                    on_step(st, True)
        n = plan.n
        feats = arena[plan.features_off: plan.features_off + n * N_FEATURES].view(n, N_FEATURES)
        if upto_features:
            return feats
        return arena[plan.logits_off: plan.logits_off + n * N_CLASSES].view(n, N_CLASSES)

    @torch.no_grad()
    def features(self, x, boxes=None, valid=None, crop_size=None, sampling="reference", resize=False):
        return self._run(x, "none" if resize else None, upto_features=True, boxes=boxes, valid=valid, crop_size=crop_size,
                         sampling=sampling)

    @torch.no_grad()
    def forward(self, x, boxes=None, valid=None, crop_size=None, sampling="reference", resize=False):
        """``resize``: the bilinear resize to 299 x 299 first (``nn.Upsample``, align_corners False: lib/metrics.py:385).  ``boxes``
        [N, 4] int32 (+ ``valid``, ``crop_size``, ``sampling``: person_crop.py) with ``resize=True``: every image is cut to its box,
        resized to ``crop_size`` and then to 299 in that same first launch -- bit-identical to
        ``forward(inception_input(person_crop.crop_and_resize(x, boxes, crop_size, valid, sampling)))``."""
        return self._run(x, "none" if resize else None, boxes=boxes, valid=valid, crop_size=crop_size, sampling=sampling)


class FIDInceptionModel(InceptionV3):
    """models/imagenet_pretrained.py:64-111: bilinear resize to 299 x 299 (``nn.Upsample`` default, align_corners False) ->
    ``clamp((x + 1) / 2, 0, 1)`` -> ``(x - mean) / std`` (one launch) -> the modules up to ``Mixed_7c`` with ``F.avg_pool2d(3, 2)``
    after ``Conv2d_2b_3x3`` and ``Conv2d_4a_3x3`` (``stem_pool="avg"``: an assumption about the torchvision version, see the module
    header) -> the global average: [N, 3, H, W] in [-1, 1] -> [N, 2048].  The state-dict keys are torchvision's (no ``v3.`` prefix,
    ``mean`` / ``std`` are constants of the input kernel)."""

    def __init__(self, state_dict=None, seed: int = 1234):
        super().__init__(state_dict, transform_input=False, stem_pool="avg", seed=seed)

    @torch.no_grad()
    def forward(self, x, boxes=None, valid=None, crop_size=None, sampling="reference"):
        return self._run(x, resize_mode="fid", upto_features=True, boxes=boxes, valid=valid, crop_size=crop_size, sampling=sampling)

    features = forward


def inception_input(x: torch.Tensor, mode: str = "none") -> torch.Tensor:
    """[N, 3, H, W] fp32 on the GPU -> [N, 3, 299, 299]: bilinear (align_corners False) with the point-wise affine of ``mode``
    fused -- "none", "transform" (torchvision's transform_input) or "fid" (FIDInceptionModel's clamp + normalise)."""
    ops._dev(x)
    if x.dim() != 4 or x.shape[1] != 3:
        raise ValueError(f"[N, 3, H, W] expected, got {tuple(x.shape)}")
    x = x.contiguous()
    y = torch.empty(x.shape[0], 3, SIZE, SIZE, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _call("vunet_inception_input", _p(x), _p(y), int(x.shape[0]), int(x.shape[2]), int(x.shape[3]), INPUT_MODES[mode], _stream())
    return y
