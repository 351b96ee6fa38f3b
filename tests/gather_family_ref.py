"""float64 restatement of one fused convolution layer as the fp32-input kernels of vunet_conv2d_gather compute it, and an
elementwise error bound DERIVED from the arithmetic (tests/test_hip_gather_family.py).  Plain torch on the CPU.

With U = 2^-24 (fp32's unit roundoff), a = the operand after the prologue, mag = conv(|a|, |w|), T = taps x (C1 + C2):

    |got - ref| <= 2 (T + 4) U mag + conv(da, |w|) + 4 U (|shift| + |res| + |ref|) + TINY

  * 2 (T + 4) U mag: forward error of a length-T fp32 sum in ANY order ((T - 1) U mag to first order); the factor 2 allows
    for the matrix cores' unspecified accumulation order and intermediate rounding that need not be to nearest.
  * da: what the prologue's own rounding puts into each operand -- 0 without a prologue, the bound
    tests/test_hip_pointwise.py::_act_bound holds vunet_act_fwd to for ELU, 2 U |a| for leaky ReLU; the dropout keep-scale
    is one more fp32 product (U |a|: a rounding the first statement of this bound left out).
  * an ELU / sigmoid output activation passes the accumulated bound through its Lipschitz constant (1 and 1/4) and adds
    its own _act_bound term.
  * mode 1 with aux: the accumulated bound times |act'(aux)|, plus 4 U |ref|, plus |conv| x the error of act' itself --
    ELU' is ``__expf`` below zero, whose relative error grows with |x| (the same (|x| + 1) e^x term _act_bound has; a
    second rounding the first statement left out).
"""
import numpy as np
import torch
import torch.nn.functional as F

from hip_parity_utils import dropout_keep_mask
from test_hip_pointwise import ACTS, TINY, U, _act_bound, _act_ref

ACT_NONE, ACT_ELU, ACT_RELU, ACT_SIGMOID, ACT_LRELU = 0, ACTS["elu"], ACTS["relu"], ACTS["sigmoid"], ACTS["lrelu"]
SEED2_OFFSET = 0x9E3779B9   # (ops.SEED2_OFFSET; the tests assert the two are one number)


def keep_scale(p: float) -> float:
    """1 / (1 - p) as make_inact (csrc/common.h) forms it: every step in fp32."""
    p32 = np.float32(p)
    return float(np.float32(1.0) / (np.float32(1.0) - p32))


def _d2s(t):
    from oracle import vunet_oracle as O
    return O.depth_to_space(t)


def prologue64(x, act, slope, drop_p, seed):
    """-> (a, da): the operand the kernel multiplies and the bound of its fp32 error."""
    t = x.double().cpu()
    if act == ACT_ELU:
        a = _act_ref("elu", t)
        da = _act_bound("elu", t, a)
    elif act == ACT_LRELU:
        a = torch.where(t > 0, t, t * float(np.float32(slope)))
        da = 2 * U * a.abs()
    elif act == ACT_RELU:
        a, da = torch.relu(t), torch.zeros_like(t)
    else:
        a, da = t, torch.zeros_like(t)
    if drop_p > 0:
        keep = dropout_keep_mask(tuple(x.shape), drop_p, seed).double() * keep_scale(drop_p)
        a = a * keep
        da = da * keep + U * a.abs()      # the product with the keep-scale rounds once more
    return a, da


def act_grad64(aux, act, slope, drop_p, seed):
    """-> (g, dg): d/dv of the forward's prologue at the pre-activation value (in_act_grad, csrc/common.h) and its error."""
    t = aux.double().cpu()
    if act == ACT_ELU:
        g = torch.where(t > 0, torch.ones_like(t), torch.exp(t))
        # __expf below zero: _act_bound's ELU expression bounds the error of e^x (it is the error of e^x - 1)
        dg = torch.where(t > 0, torch.zeros_like(t), _act_bound("elu", t, _act_ref("elu", t)))
    elif act == ACT_RELU:
        g, dg = (t > 0).double(), torch.zeros_like(t)
    elif act == ACT_LRELU:
        g, dg = torch.where(t > 0, torch.ones_like(t), torch.full_like(t, float(np.float32(slope)))), torch.zeros_like(t)
    else:
        g, dg = torch.ones_like(t), torch.zeros_like(t)
    if drop_p > 0:
        keep = dropout_keep_mask(tuple(aux.shape), drop_p, seed).double() * keep_scale(drop_p)
        g = g * keep
        dg = dg * keep + U * g.abs()
    return g, dg


def _core(d, a, w):
    """The convolution of the descriptor on a float64 operand: conv2d (mode 0) or its transpose (mode 1)."""
    if d.mode == 0:
        return F.conv2d(a, w, None, stride=d.stride, padding=d.pad)
    oph = d.Ho - ((d.Hs - 1) * d.stride - 2 * d.pad + d.KH)
    opw = d.Wo - ((d.Ws - 1) * d.stride - 2 * d.pad + d.KW)
    return F.conv_transpose2d(a, w, None, stride=d.stride, padding=d.pad, output_padding=(oph, opw))


def ref_conv64(d, x1, x2, w_eff, shift, res, aux, relu_mask=None):
    """One fused layer of descriptor ``d`` (any object with vunet_conv_desc's fields) in float64 -> (ref, bound).

    ``w_eff``: the fp32 weight the kernel multiplies, [M, C1 + C2, KH, KW] for mode 0 and [C1, M, KH, KW] (the forward
    layer's [Cout, Cin, ...]) for mode 1.  ``relu_mask``: the forward OUTPUT of a ReLU layer -- the masked data gradient
    dgrad(dy * [y > 0]); a select, so it adds no error."""
    w = w_eff.double().cpu()
    ops_a, ops_da = [], []
    for i, x in enumerate((x1, x2)):
        if x is None:
            continue
        seed = d.drop_seed if i == 0 else (d.drop_seed + SEED2_OFFSET) & 0xFFFFFFFF
        a, da = prologue64(x, d.in_act, d.in_slope, d.drop_p, seed)
        if relu_mask is not None:
            a = torch.where(relu_mask.double().cpu() > 0, a, torch.zeros_like(a))
        ops_a.append(a)
        ops_da.append(da)
    a, da = torch.cat(ops_a, dim=1), torch.cat(ops_da, dim=1)
    T = d.KH * d.KW * (d.C1 + d.C2)
    ref = _core(d, a, w)
    bound = 2 * (T + 4) * U * _core(d, a.abs(), w.abs()) + _core(d, da, w.abs())
    if d.mode == 0:
        if shift is not None:
            sh = shift.double().cpu().view(1, -1, 1, 1)
            ref = ref + sh
            bound = bound + 4 * U * (sh.abs() + ref.abs())
        if d.out_act == ACT_RELU:
            ref = torch.relu(ref)
        elif d.out_act == ACT_SIGMOID:
            pre, ref = ref, torch.sigmoid(ref)
            bound = bound / 4 + _act_bound("sigmoid", pre, ref)
        elif d.out_act == ACT_ELU:
            pre, ref = ref, _act_ref("elu", ref)
            bound = bound + _act_bound("elu", pre, ref)
        elif d.out_act != ACT_NONE:
            raise ValueError("output activation not restated here")
        if d.d2s:
            ref, bound = _d2s(ref), _d2s(bound)
    elif aux is not None:
        g, dg = act_grad64(aux, d.aux_act, d.aux_slope, d.aux_drop_p, d.aux_drop_seed)
        bound = bound * g.abs() + ref.abs() * dg
        ref = ref * g
        bound = bound + 4 * U * ref.abs()
    if res is not None:
        r = res.double().cpu()
        ref = ref + r
        bound = bound + 4 * U * r.abs()
    return ref, bound + 4 * U * ref.abs() + TINY
