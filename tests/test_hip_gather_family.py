"""The fp32-input convolution family behind vunet_conv2d_gather -- conv_tiled_kernel, conv_gather_kernel,
conv_gather_splitk_kernel, the per-parity phase launches, conv_1x1_kernel and the four conv_thin_* kernels -- one
instantiation at a time, by the name the router reports, against a float64 restatement of the fused layer under a bound
derived from the arithmetic (tests/gather_family_ref.py), and the |y| maxima five of these kernels publish.

This family is what ``set_conv_precision("f32")`` runs, what takes every layer the split router refuses, and the baseline the
split kernels' own tests compare with.  Without a GPU: the table is checked against a literal list of every instantiation
of the launch switches, every row against the router's answer, and the bound against five mutations of a stand-in kernel.
With one (-m gpu): every row launches on the smallest shape that reaches its instantiation; each test prints the worst
|got - ref| / bound it saw (profiles/gather_family_accuracy.txt keeps the figures of one run).
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from gather_family_ref import ACT_ELU, ACT_LRELU, ACT_NONE, ACT_RELU, ACT_SIGMOID, SEED2_OFFSET, keep_scale, ref_conv64
from hip_parity_utils import assert_close, assert_ulps, dropout_keep_mask

gpu = pytest.mark.gpu
SEED, AUX_SEED = 0xC0FFEE, 0xBEEF51
UNSUPPORTED = -3   # VUNET_ERR_UNSUPPORTED


def _ops():
    from behavior_driven_video_synthesis_amd import ops
    return ops


# ------------------------------------------------------------------------------------------------ the table
# Every instantiation the launch switches of conv_tiled_mt1.hip / conv_tiled_mt2.hip (launch_tiled_pro), conv_gather.hip
# (launch_gather, launch_splitk, the CONV_PHASE loop), conv_1x1.hip (launch_1x1) and conv_thin.hip (vunet_conv_thin_launch)
# can start, in rocprofv3's spelling as conv_route_name prints it.  Written out: a new instantiation without a row in
# GATHER_EVERY fails test_table_covers_every_instantiation.
ALL_INSTANTIATIONS = [
    "conv_tiled_kernel<1, 1, 8, 0, 0, 32, 1>", "conv_tiled_kernel<1, 1, 8, 0, 1, 32, 1>",
    "conv_tiled_kernel<1, 1, 8, 0, 2, 32, 1>", "conv_tiled_kernel<1, 1, 8, 1, 0, 32, 1>",
    "conv_tiled_kernel<1, 1, 8, 1, 4, 32, 1>", "conv_tiled_kernel<1, 2, 8, 0, 0, 32, 1>",
    "conv_tiled_kernel<1, 2, 8, 0, 1, 32, 1>", "conv_tiled_kernel<1, 2, 8, 0, 2, 32, 1>",
    "conv_tiled_kernel<1, 2, 8, 1, 0, 32, 1>", "conv_tiled_kernel<1, 2, 8, 1, 4, 32, 1>",
    "conv_tiled_kernel<1, 4, 8, 0, 0, 32, 1>", "conv_tiled_kernel<1, 4, 8, 0, 1, 32, 1>",
    "conv_tiled_kernel<1, 4, 8, 0, 2, 32, 1>", "conv_tiled_kernel<1, 4, 8, 1, 0, 32, 1>",
    "conv_tiled_kernel<1, 4, 8, 1, 4, 32, 1>", "conv_tiled_kernel<1, 1, 8, 0, 0, 16, 1>",
    "conv_tiled_kernel<1, 1, 8, 0, 1, 16, 1>", "conv_tiled_kernel<1, 1, 8, 0, 2, 16, 1>",
    "conv_tiled_kernel<1, 1, 8, 1, 0, 16, 1>", "conv_tiled_kernel<1, 1, 8, 1, 4, 16, 1>",
    "conv_tiled_kernel<1, 1, 8, 0, 0, 32, 2>", "conv_tiled_kernel<1, 1, 8, 0, 1, 32, 2>",
    "conv_tiled_kernel<1, 1, 8, 0, 2, 32, 2>", "conv_tiled_kernel<2, 1, 8, 0, 0, 32, 1>",
    "conv_tiled_kernel<2, 1, 8, 0, 1, 32, 1>", "conv_tiled_kernel<2, 1, 8, 0, 2, 32, 1>",
    "conv_tiled_kernel<2, 1, 8, 1, 0, 32, 1>", "conv_tiled_kernel<2, 1, 8, 1, 4, 32, 1>",
    "conv_tiled_kernel<2, 2, 8, 0, 0, 32, 1>", "conv_tiled_kernel<2, 2, 8, 0, 1, 32, 1>",
    "conv_tiled_kernel<2, 2, 8, 0, 2, 32, 1>", "conv_tiled_kernel<2, 2, 8, 1, 0, 32, 1>",
    "conv_tiled_kernel<2, 2, 8, 1, 4, 32, 1>", "conv_tiled_kernel<2, 4, 4, 0, 0, 32, 1>",
    "conv_tiled_kernel<2, 4, 4, 0, 1, 32, 1>", "conv_tiled_kernel<2, 4, 4, 0, 2, 32, 1>",
    "conv_tiled_kernel<2, 4, 4, 1, 0, 32, 1>", "conv_tiled_kernel<2, 4, 4, 1, 4, 32, 1>",
    "conv_tiled_kernel<2, 1, 8, 0, 0, 16, 1>", "conv_tiled_kernel<2, 1, 8, 0, 1, 16, 1>",
    "conv_tiled_kernel<2, 1, 8, 0, 2, 16, 1>", "conv_tiled_kernel<2, 1, 8, 1, 0, 16, 1>",
    "conv_tiled_kernel<2, 1, 8, 1, 4, 16, 1>", "conv_tiled_kernel<2, 1, 8, 0, 0, 32, 2>",
    "conv_tiled_kernel<2, 1, 8, 0, 1, 32, 2>", "conv_tiled_kernel<2, 1, 8, 0, 2, 32, 2>",
    "conv_gather_kernel<1, 4, 0, 0>", "conv_gather_kernel<1, 4, 0, 1>", "conv_gather_kernel<1, 4, 0, 3>",
    "conv_gather_kernel<1, 4, 1, 0>", "conv_gather_kernel<1, 4, 1, 1>", "conv_gather_kernel<1, 4, 1, 3>",
    "conv_gather_kernel<1, 4, 2, 0>", "conv_gather_kernel<1, 4, 2, 1>", "conv_gather_kernel<1, 4, 2, 3>",
    "conv_gather_kernel<1, 4, 3, 0>", "conv_gather_kernel<1, 4, 3, 1>", "conv_gather_kernel<1, 4, 3, 3>",
    "conv_gather_kernel<2, 2, 0, 0>", "conv_gather_kernel<2, 2, 0, 1>", "conv_gather_kernel<2, 2, 0, 3>",
    "conv_gather_kernel<2, 2, 1, 0>", "conv_gather_kernel<2, 2, 1, 1>", "conv_gather_kernel<2, 2, 1, 3>",
    "conv_gather_kernel<2, 2, 2, 0>", "conv_gather_kernel<2, 2, 2, 1>", "conv_gather_kernel<2, 2, 2, 3>",
    "conv_gather_kernel<2, 2, 3, 0>", "conv_gather_kernel<2, 2, 3, 1>", "conv_gather_kernel<2, 2, 3, 3>",
    "conv_gather_splitk_kernel<16, 0, 0>", "conv_gather_splitk_kernel<16, 0, 1>", "conv_gather_splitk_kernel<16, 0, 3>",
    "conv_gather_splitk_kernel<16, 1, 0>", "conv_gather_splitk_kernel<16, 1, 1>", "conv_gather_splitk_kernel<16, 1, 3>",
    "conv_gather_splitk_kernel<16, 2, 0>", "conv_gather_splitk_kernel<16, 2, 1>", "conv_gather_splitk_kernel<16, 2, 3>",
    "conv_gather_splitk_kernel<16, 3, 0>", "conv_gather_splitk_kernel<16, 3, 1>", "conv_gather_splitk_kernel<16, 3, 3>",
    "conv_gather_kernel<phase x4>", "conv_1x1_kernel<1, 0, 0>", "conv_1x1_kernel<1, 0, 1>", "conv_1x1_kernel<1, 0, 2>",
    "conv_1x1_kernel<1, 1, 0>", "conv_1x1_kernel<2, 0, 0>", "conv_1x1_kernel<2, 0, 1>", "conv_1x1_kernel<2, 0, 2>",
    "conv_1x1_kernel<2, 1, 0>", "conv_1x1_kernel<4, 0, 0>", "conv_1x1_kernel<4, 0, 1>", "conv_1x1_kernel<4, 0, 2>",
    "conv_1x1_kernel<4, 1, 0>", "conv_thin_m_kernel<0>", "conv_thin_m_kernel<1>", "conv_thin_mv_kernel<0, 4>",
    "conv_thin_mv_kernel<1, 4>", "conv_thin_k_kernel<1, 3>", "conv_thin_k_kernel<3, 3>", "conv_thin_kv_kernel<3, 4>",
]
# instantiation -> the routing line that keeps the C ABI from reaching it at any shape (dead code, kept in the list above)
UNREACHABLE = {}


def _row(name, n, c1, c2, m, hs, ws, k=3, stride=1, pad=1, mode=0, in_act=ACT_NONE, slope=0.0, drop=0.0, out_act=ACT_NONE,
         d2s=0, res=False, aux_act=None, aux_drop=0.0, nt=0, masked=False, ho=None, wo=None, yoff=0, parity=None):
    """One case.  mode 0: x1 [n, c1, hs, ws] (+ x2 with c2 channels) -> y [n, m, ho, wo].  mode 1: the source is dy
    [n, c1, hs, ws] (c1 = the forward layer's output channels), the result dx [n, m, ho, wo]; aux_act: the forward's
    prologue, applied as act'(aux) in the epilogue; masked: through vunet_conv2d_dgrad_relu.  nt: tiled_force_nt.
    yoff: y is a view that many floats into its allocation.  parity: what each parity launch of a phase row must be."""
    if mode == 0:
        ho = (hs + 2 * pad - k) // stride + 1 if ho is None else ho
        wo = (ws + 2 * pad - k) // stride + 1 if wo is None else wo
    else:
        ho = hs if ho is None else ho
        wo = ws if wo is None else wo
    return dict(name=name, n=n, c1=c1, c2=c2, m=m, hs=hs, ws=ws, k=k, stride=stride, pad=pad, mode=mode, in_act=in_act,
                slope=slope, drop=drop, out_act=out_act, d2s=d2s, res=res, aux_act=aux_act, aux_drop=aux_drop, nt=nt,
                masked=masked, ho=ho, wo=wo, yoff=yoff, parity=parity)


def _tiled_rows():
    """conv_tiled_kernel<MT, nt, CK, mode, pro, TW, S>: ten tile forms forced on their smallest geometry with
    tiled_force_nt.  TW 32: H = 4 nt, W = 32, two images (a tile boundary between them); TW 16: 8 x 48 (three column tiles);
    stride 2: 8 x 64 -> 4 x 32.  M = 32 / 40 (ragged second m-tile), C1 = 24 (an odd number of 8-channel chunks), a second
    source of 8 channels on the prologue rows, a residual on half of them (the ELU + dropout ones)."""
    rows, i = [], 0
    for mt in (1, 2):
        m = 32 if mt == 1 else 40
        for nt, ck, tw, s in ((1, 8, 32, 1), (2, 8, 32, 1), (4, 8 if mt == 1 else 4, 32, 1), (1, 8, 16, 1), (1, 8, 32, 2)):
            h, w = (8, 64) if s == 2 else ((8, 48) if tw == 16 else (4 * nt, 32))
            geo = dict(k=3, stride=s, pad=1, nt=nt)
            for pro in (0, 1, 2):
                i += 1
                rows.append(_row("conv_tiled_kernel<%d, %d, %d, 0, %d, %d, %d>" % (mt, nt, ck, pro, tw, s), 2, 24,
                                 8 if pro else 0, m, h, w, in_act=ACT_ELU if pro else ACT_NONE, drop=0.1 if pro == 2 else 0.0,
                                 out_act=ACT_RELU if (pro == 0 and i % 2 == 0) else ACT_NONE,
                                 res=pro == 2 or (pro == 0 and i % 2 == 1), **geo))
            if s == 2:
                continue
            i += 1
            rows.append(_row("conv_tiled_kernel<%d, %d, %d, 1, 0, %d, 1>" % (mt, nt, ck, tw), 2, 24, 0, m, h, w, mode=1,
                             aux_act=ACT_ELU, aux_drop=0.1 if i % 2 else 0.0, res=True, **geo))
            rows.append(_row("conv_tiled_kernel<%d, %d, %d, 1, 4, %d, 1>" % (mt, nt, ck, tw), 2, 24, 0, m, h, w, mode=1,
                             masked=True, res=bool(i % 2), **geo))
    # ten masked rows: the eight instantiations and the other residual setting of the two 4-row forms
    rows.append(_row("conv_tiled_kernel<1, 1, 8, 1, 4, 32, 1>", 2, 24, 0, 32, 4, 32, mode=1, masked=True, res=True, nt=1))
    rows.append(_row("conv_tiled_kernel<2, 1, 8, 1, 4, 32, 1>", 2, 24, 0, 40, 4, 32, mode=1, masked=True, res=False, nt=1))
    return rows


E, L, R_, S_ = ACT_ELU, ACT_LRELU, ACT_RELU, ACT_SIGMOID
# conv_gather_kernel<MT, NT, pro, KS>: one wave per tile; <1, 4> for M <= 32, <2, 2> above.  Kept off the LDS-tiled kernel
# (W = 9, channel counts that are no multiple of 8) and off split-K (fewer than 32 channel pairs; k = 4: fewer than 18).
# pro 3: any prologue but ELU (+ dropout).  KS 0: k = 4, both strides.
_GATHER_ROWS = [
    _row("conv_gather_kernel<1, 4, 0, 3>", 3, 1, 0, 8, 7, 9),                                   # C1 = 1; 189 pixels: no multiple of 32
    _row("conv_gather_kernel<1, 4, 1, 3>", 2, 33, 5, 32, 4, 4, in_act=E, res=True),               # odd channel pairs; map smaller than the reach
    _row("conv_gather_kernel<1, 4, 2, 3>", 2, 8, 8, 12, 6, 9, in_act=E, drop=0.2, d2s=1, res=True),
    _row("conv_gather_kernel<1, 4, 3, 3>", 2, 5, 0, 7, 9, 9, pad=0, in_act=L, slope=0.2),         # pad 0
    _row("conv_gather_kernel<2, 2, 0, 3>", 2, 33, 0, 35, 5, 9, out_act=S_),
    _row("conv_gather_kernel<2, 2, 1, 3>", 1, 16, 0, 64, 4, 9, in_act=E, d2s=1),
    _row("conv_gather_kernel<2, 2, 2, 3>", 2, 24, 8, 40, 5, 9, in_act=E, drop=0.1, res=True),
    _row("conv_gather_kernel<2, 2, 3, 3>", 2, 7, 3, 33, 9, 11, stride=2, drop=0.3, out_act=S_),   # dropout without ELU, stride 2
    _row("conv_gather_kernel<1, 4, 0, 1>", 2, 33, 0, 32, 8, 8, k=1, pad=0, out_act=R_),
    _row("conv_gather_kernel<1, 4, 1, 1>", 1, 32, 0, 16, 5, 9, k=1, pad=0, in_act=E),
    _row("conv_gather_kernel<1, 4, 2, 1>", 2, 16, 16, 32, 7, 9, k=1, pad=0, in_act=E, drop=0.1, res=True),
    _row("conv_gather_kernel<1, 4, 3, 1>", 2, 32, 0, 8, 8, 8, k=1, pad=0, in_act=L, slope=0.2, d2s=1),
    _row("conv_gather_kernel<2, 2, 0, 1>", 2, 33, 0, 64, 8, 8, k=1, pad=0, res=True),
    _row("conv_gather_kernel<2, 2, 1, 1>", 3, 31, 0, 35, 6, 6, k=1, pad=0, in_act=E),
    _row("conv_gather_kernel<2, 2, 2, 1>", 1, 16, 8, 48, 5, 9, k=1, pad=0, in_act=E, drop=0.1, out_act=E),
    _row("conv_gather_kernel<2, 2, 3, 1>", 2, 32, 0, 40, 8, 8, k=1, pad=0, in_act=R_),
    _row("conv_gather_kernel<1, 4, 0, 0>", 2, 3, 0, 8, 10, 10, k=4, stride=2),                    # the PatchGAN layers
    _row("conv_gather_kernel<1, 4, 1, 0>", 2, 8, 0, 4, 6, 6, k=4, in_act=E),
    _row("conv_gather_kernel<1, 4, 2, 0>", 2, 16, 8, 32, 8, 12, k=4, stride=2, in_act=E, drop=0.1),
    _row("conv_gather_kernel<1, 4, 3, 0>", 1, 33, 0, 16, 7, 7, k=4, pad=0, in_act=L, slope=0.2),
    _row("conv_gather_kernel<2, 2, 0, 0>", 2, 33, 0, 35, 6, 6, k=4),
    _row("conv_gather_kernel<2, 2, 1, 0>", 2, 16, 0, 64, 8, 8, k=4, stride=2, in_act=E, res=True),
    _row("conv_gather_kernel<2, 2, 2, 0>", 2, 8, 8, 40, 5, 9, k=4, in_act=E, drop=0.1),
    _row("conv_gather_kernel<2, 2, 3, 0>", 2, 9, 7, 33, 10, 10, k=4, stride=2, in_act=L, slope=0.2, drop=0.1),
    # the stride-1 data gradient of a layer the tiled kernel does not take
    _row("conv_gather_kernel<1, 4, 0, 3>", 2, 10, 0, 6, 5, 9, mode=1, aux_act=E, aux_drop=0.1, res=True),
]
# conv_gather_splitk_kernel<16, pro, KS>: 16 waves share a tile's K loop (want_splitk, conv_x6.hip: at least 32 channel pairs
# on at most 768 tiles)
_SPLITK_ROWS = [
    _row("conv_gather_splitk_kernel<16, 0, 3>", 2, 64, 0, 35, 4, 4, res=True),
    _row("conv_gather_splitk_kernel<16, 1, 3>", 2, 32, 32, 32, 8, 8, in_act=E, out_act=R_),
    _row("conv_gather_splitk_kernel<16, 2, 3>", 2, 64, 8, 64, 5, 5, in_act=E, drop=0.1, d2s=1, res=True),   # 50 pixels
    _row("conv_gather_splitk_kernel<16, 3, 3>", 1, 65, 0, 33, 6, 6, in_act=L, slope=0.2),
    _row("conv_gather_splitk_kernel<16, 0, 1>", 2, 64, 0, 32, 8, 8, k=1, pad=0),                 # (the 1x1 kernel would take it)
    _row("conv_gather_splitk_kernel<16, 1, 1>", 2, 33, 33, 35, 5, 5, k=1, pad=0, in_act=E, res=True),
    _row("conv_gather_splitk_kernel<16, 2, 1>", 2, 64, 32, 64, 4, 8, k=1, pad=0, in_act=E, drop=0.1, d2s=1),
    _row("conv_gather_splitk_kernel<16, 3, 1>", 2, 64, 0, 16, 4, 4, k=1, pad=0, in_act=L, slope=0.2, out_act=S_),
    _row("conv_gather_splitk_kernel<16, 0, 0>", 2, 64, 0, 32, 8, 8, k=4, stride=2),
    _row("conv_gather_splitk_kernel<16, 1, 0>", 2, 32, 32, 35, 5, 5, k=4, in_act=E),
    _row("conv_gather_splitk_kernel<16, 2, 0>", 2, 48, 16, 40, 8, 8, k=4, stride=2, in_act=E, drop=0.1, res=True),
    _row("conv_gather_splitk_kernel<16, 3, 0>", 2, 64, 0, 8, 5, 5, k=4, in_act=R_, d2s=1),
]
# the stride-2 data gradient: one generic-gather launch per output parity, each of the form conv_route_gather_form picks for
# its own pixel count.  Odd Ho / Wo: the four parities differ in size.
_PHASE_ROWS = [
    _row("conv_gather_kernel<phase x4>", 2, 64, 0, 24, 5, 5, stride=2, mode=1, ho=9, wo=9, parity="splitk"),
    _row("conv_gather_kernel<phase x4>", 2, 32, 0, 35, 4, 6, k=4, stride=2, mode=1, ho=9, wo=13, aux_act=E, aux_drop=0.1,
         res=True, parity="onewave"),
    _row("conv_gather_kernel<phase x4>", 2, 24, 0, 8, 4, 4, stride=2, mode=1, ho=8, wo=8, aux_act=E, res=True,
         parity="onewave"),
    _row("conv_gather_kernel<phase x4>", 1, 64, 0, 33, 4, 4, k=4, stride=2, mode=1, ho=8, wo=8, res=True, parity="splitk"),
]
# conv_1x1_kernel<MT, mode, pro>: MT above 1 needs N H W >= 131072 (vunet_conv_1x1_mt).  W = 40: pixel tiles straddle rows.
_BIG = dict(hs=256, ws=256, k=1, pad=0)
_1X1_ROWS = [
    _row("conv_1x1_kernel<1, 0, 0>", 2, 32, 0, 32, 8, 8, k=1, pad=0, res=True),
    _row("conv_1x1_kernel<1, 0, 0>", 2, 32, 0, 32, 8, 8, k=1, pad=0, res=True, yoff=1),          # y off 16-byte alignment: scalar epilogue
    _row("conv_1x1_kernel<1, 0, 1>", 2, 32, 0, 24, 8, 40, k=1, pad=0, in_act=E, out_act=S_),
    _row("conv_1x1_kernel<1, 0, 2>", 2, 32, 32, 35, 112, 112, k=1, pad=0, in_act=E, drop=0.1, res=True),   # two sources: past split-K
    _row("conv_1x1_kernel<1, 1, 0>", 2, 32, 0, 32, 8, 40, k=1, pad=0, mode=1, aux_act=E, aux_drop=0.1, res=True),
    _row("conv_1x1_kernel<2, 0, 0>", 2, 32, 0, 64, out_act=R_, **_BIG),
    _row("conv_1x1_kernel<2, 0, 1>", 2, 32, 0, 64, in_act=E, res=True, **_BIG),
    _row("conv_1x1_kernel<2, 0, 2>", 2, 32, 0, 64, in_act=E, drop=0.1, **_BIG),
    _row("conv_1x1_kernel<2, 1, 0>", 2, 32, 0, 64, mode=1, aux_act=E, res=True, **_BIG),
    _row("conv_1x1_kernel<4, 0, 0>", 2, 32, 0, 128, res=True, **_BIG),
    _row("conv_1x1_kernel<4, 0, 1>", 2, 32, 0, 128, in_act=E, **_BIG),
    _row("conv_1x1_kernel<4, 0, 2>", 2, 32, 0, 128, in_act=E, drop=0.1, **_BIG),
    _row("conv_1x1_kernel<4, 1, 0>", 2, 32, 0, 128, mode=1, **_BIG),
]
# the VALU kernels for <= 4 channels on one side: N H W >= 65536; the strip forms from H = 32.  W = 176: 5.5 tiles.
_THIN_ROWS = [
    _row("conv_thin_m_kernel<0>", 14, 8, 0, 3, 28, 176),
    _row("conv_thin_m_kernel<1>", 14, 8, 0, 4, 28, 176, mode=1, res=True),
    _row("conv_thin_mv_kernel<0, 4>", 11, 8, 0, 4, 36, 176, out_act=S_),
    _row("conv_thin_mv_kernel<1, 4>", 11, 16, 0, 3, 36, 176, mode=1, res=True),
    _row("conv_thin_k_kernel<1, 3>", 14, 3, 0, 40, 28, 176, k=1, pad=0, out_act=R_),
    _row("conv_thin_k_kernel<3, 3>", 14, 3, 0, 40, 28, 176),
    _row("conv_thin_k_kernel<3, 3>", 8, 3, 0, 128, 24, 352, out_act=R_),
    _row("conv_thin_k_kernel<3, 3>", 14, 3, 0, 40, 28, 176, mode=1),
    _row("conv_thin_kv_kernel<3, 4>", 11, 3, 0, 40, 36, 176, out_act=R_),
    _row("conv_thin_kv_kernel<3, 4>", 11, 3, 0, 128, 36, 176),
]
GATHER_EVERY = _tiled_rows() + _GATHER_ROWS + _SPLITK_ROWS + _PHASE_ROWS + _1X1_ROWS + _THIN_ROWS
# a masked data gradient conv_route_tiled refuses (a 9-wide map): vunet_conv2d_dgrad_relu answers VUNET_ERR_UNSUPPORTED
REFUSED_MASKED = _row("refused", 2, 24, 0, 32, 4, 9, mode=1, masked=True, res=True, nt=1)


def _family(name):
    if name.endswith("<phase x4>"):
        return "phase"
    return name.split("_kernel")[0].replace("conv_", "")


def _id(r):
    return "%s-n%dc%d+%dm%d-%dx%d%s%s" % (r["name"].replace(" ", ""), r["n"], r["c1"], r["c2"], r["m"], r["hs"], r["ws"],
                                         "-dx" if r["mode"] else "", "-off" if r["yoff"] else ("-res" if r["res"] else ""))


# ------------------------------------------------------------------------------------------------ inputs, descriptor, launch
def _r32(x):
    return (x + 31) // 32 * 32


def make_inputs(r, seed):
    """CPU fp32 tensors of one row: sources, weight-norm parameters of the layer, residual, aux, ReLU-mask source."""
    g_ = torch.Generator().manual_seed(seed)
    n, c1, c2, m, k = r["n"], r["c1"], r["c2"], r["m"], r["k"]
    out_shape = (n, m // 4, 2 * r["ho"], 2 * r["wo"]) if r["d2s"] else (n, m, r["ho"], r["wo"])
    t = dict(x1=torch.randn(n, c1, r["hs"], r["ws"], generator=g_),
             x2=torch.randn(n, c2, r["hs"], r["ws"], generator=g_) if c2 else None)
    cout, cin = (m, c1 + c2) if r["mode"] == 0 else (c1, m)
    t["v"] = torch.randn(cout, cin, k, k, generator=g_) * 0.2
    t["g"] = torch.rand(cout, 1, 1, 1, generator=g_) + 0.5
    t["bias"] = torch.randn(cout, generator=g_) * 0.1
    t["gamma"] = 1.0 + 0.3 * torch.randn(1, cout, 1, 1, generator=g_)
    t["beta"] = 0.2 * torch.randn(1, cout, 1, 1, generator=g_)
    t["res"] = torch.randn(out_shape, generator=g_) if r["res"] else None
    t["aux"] = torch.randn(out_shape, generator=g_) if r["aux_act"] is not None else None
    t["ymask"] = torch.randn(n, c1, r["hs"], r["ws"], generator=g_) if r["masked"] else None
    return t


def make_desc(ops, r, mpad):
    return ops.ConvDesc(N=r["n"], C1=r["c1"], C2=r["c2"], Hs=r["hs"], Ws=r["ws"], M=r["m"], m_off=0, Mpad=mpad, Ho=r["ho"],
                        Wo=r["wo"], KH=r["k"], KW=r["k"], stride=r["stride"], pad=r["pad"], mode=r["mode"], in_act=r["in_act"],
                        in_slope=r["slope"], drop_p=r["drop"], drop_seed=SEED, out_act=r["out_act"], d2s=r["d2s"],
                        aux_act=r["aux_act"] or 0, aux_slope=0.0, aux_drop_p=r["aux_drop"], aux_drop_seed=AUX_SEED)


def _variant(ops, d, has_aux):
    buf = ctypes.create_string_buffer(96)
    assert ops._lib.lib().vunet_conv2d_gather_variant(ctypes.byref(d), int(has_aux), buf, 96) == 0
    return buf.value.decode()


def _route_name(ops, r):
    """What the router calls the kernel of row ``r`` (host logic).  vunet_conv2d_dgrad_relu has no name query: its kernel is
    the unmasked data gradient's with prologue code 4 (ops._gather_key spells it the same way)."""
    ops.set_tuning("tiled_force_nt", r["nt"])
    name = _variant(ops, make_desc(ops, r, _r32(r["m"])), r["aux_act"] is not None)
    return name.replace(", 1, 0, ", ", 1, 4, ") if r["masked"] else name


def _want_splitk(c1, m, npix, taps):
    """want_splitk of conv_x6.hip, restated for the phase rows: which form a parity launch of ``npix`` pixels takes."""
    tiles = ((npix + 31) // 32) * ((m + 31) // 32)
    kpairs = (c1 + 1) // 2
    return (tiles <= 768 and kpairs >= 32) or (tiles <= 2048 and kpairs * taps >= 288)


class Layer:
    """One row on the device: packed weights, descriptor, inputs; ``run`` launches into a NaN-filled output."""

    def __init__(self, ops, r, seed, edit=None):
        self.ops, self.r = ops, r
        t = make_inputs(r, seed)
        if edit is not None:
            edit(t)
        self.cpu = t
        self.dev = {k_: (None if v is None else v.cuda()) for k_, v in t.items()}
        dv = self.dev
        if r["mode"] == 0:
            pk = ops.pack_weights(dv["v"], dv["g"], dv["bias"], dv["gamma"], dv["beta"], r["c1"], r["c2"], 0, False)
            self.wt, self.shift = pk[0], pk[3]
        else:
            pk = ops.pack_weights(dv["v"], dv["g"], dv["bias"], dv["gamma"], dv["beta"], r["m"], 0, 0, True)
            self.wt, self.shift = pk[1], None
        self.w_eff = dv["v"] * pk[2].view(-1, 1, 1, 1)      # one fp32 product, as wn_pack_kernel forms it
        self.desc = make_desc(ops, r, self.wt.shape[1])
        self.out_shape = tuple(t["res"].shape) if t["res"] is not None else (
            (r["n"], r["m"] // 4, 2 * r["ho"], 2 * r["wo"]) if r["d2s"] else (r["n"], r["m"], r["ho"], r["wo"]))

    def new_out(self):
        numel = 1
        for s in self.out_shape:
            numel *= s
        buf = torch.full((numel + self.r["yoff"],), float("nan"), device="cuda")
        return buf, buf[self.r["yoff"]:].view(self.out_shape)

    def reference(self):
        c = self.cpu
        return ref_conv64(self.desc, c["x1"], c["x2"], self.w_eff, self.shift, c["res"], c["aux"], relu_mask=c["ymask"])


def _ratio(got, ref, bound):
    err = (got.detach().double().cpu() - ref).abs()
    ok = torch.isfinite(err) & (bound > 0)
    return float((err[ok] / bound[ok]).max())


# ------------------------------------------------------------------------------------------------ without a GPU
def test_table_covers_every_instantiation():
    """The names of GATHER_EVERY are exactly the instantiations written out above (none unreachable so far)."""
    assert len(set(ALL_INSTANTIATIONS)) == len(ALL_INSTANTIATIONS) == 102
    assert set(UNREACHABLE) <= set(ALL_INSTANTIATIONS)
    assert {r["name"] for r in GATHER_EVERY} == set(ALL_INSTANTIATIONS) - set(UNREACHABLE)
    assert sum(r["masked"] for r in GATHER_EVERY) == 10
    assert SEED2_OFFSET == _ops().SEED2_OFFSET


def test_every_row_is_routed_to_the_kernel_it_names():
    """Host logic, no GPU: vunet_conv2d_gather_variant answers every row with the row's own name under the row's tuning; the
    phase rows' parity launches are of the form the row says (one shape all split-K, another all one-wave); the refused
    masked row is one the LDS-tiled kernel does not take."""
    ops = _ops()
    for r in GATHER_EVERY:
        assert _route_name(ops, r) == r["name"], _id(r)
        if r["parity"]:
            forms = {_want_splitk(r["c1"], r["m"], r["n"] * ((r["ho"] - ph + 1) // 2) * ((r["wo"] - pw + 1) // 2), r["k"] ** 2)
                     for ph in (0, 1) for pw in (0, 1)}
            assert forms == {r["parity"] == "splitk"}, _id(r)
    assert {r["parity"] for r in _PHASE_ROWS} == {"splitk", "onewave"}
    assert not _route_name(ops, REFUSED_MASKED).startswith("conv_tiled_kernel")
    for r in list(PUBLISHERS.values()) + list(SILENT.values()):
        assert _route_name(ops, r) == r["name"], _id(r)


TEETH_ROWS = ["conv_tiled_kernel<2, 1, 8, 0, 2, 32, 1>", "conv_gather_kernel<2, 2, 2, 3>",
              "conv_gather_splitk_kernel<16, 2, 0>"]


def _standin(r, t, w, shift, seed2=None, keep=None):
    """An fp32 convolution on the CPU in the kernels' place: ELU and the dropout of each source, F.conv2d, shift, residual."""
    ks = torch.tensor(keep_scale(r["drop"]), dtype=torch.float32)
    seeds = (SEED, (SEED + SEED2_OFFSET) & 0xFFFFFFFF if seed2 is None else seed2)
    a = torch.cat([F.elu(x) * dropout_keep_mask(tuple(x.shape), r["drop"], s) * ks for x, s in zip((t["x1"], t["x2"]), seeds)],
                  dim=1)
    y = F.conv2d(a, w, None, stride=r["stride"], padding=r["pad"]) + shift.view(1, -1, 1, 1)
    return y + t["res"]


@pytest.mark.parametrize("name", TEETH_ROWS)
def test_the_bound_rejects_five_mutations_of_a_standin_kernel(name):
    """The evidence that the GPU tests would notice a subtly wrong kernel: at three of the table's shapes (two sources, ELU +
    dropout, ragged M, residual) an fp32 F.conv2d on the CPU passes the derived bound as it is and fails it with
      (1) one tap's weight zeroed for the last output column only (a halo error),
      (2) one 8-channel K chunk of the second source dropped,
      (3) the second source's dropout mask drawn with the first source's seed,
      (4) the last valid output channel of the ragged M written with the shift of channel 0,
      (5) one output row shifted by one pixel."""
    ops = _ops()
    r = next(x for x in GATHER_EVERY if x["name"] == name)
    assert r["mode"] == 0 and r["c2"] >= 8 and r["drop"] > 0 and r["in_act"] == ACT_ELU and r["res"] and r["m"] % 32
    assert r["out_act"] == ACT_NONE and not r["d2s"]
    t = make_inputs(r, 7)
    scale = (t["gamma"].view(-1) * t["g"].view(-1) / t["v"].flatten(1).norm(dim=1))
    shift = t["gamma"].view(-1) * t["bias"] + t["beta"].view(-1)
    w = t["v"] * scale.view(-1, 1, 1, 1)
    ref, bound = ref_conv64(make_desc(ops, r, _r32(r["m"])), t["x1"], t["x2"], w, shift, t["res"], None)
    good = _standin(r, t, w, shift)
    assert_ulps(good, ref, bound, "stand-in")
    print("%s: stand-in |got - ref| / bound <= %.3f" % (name, _ratio(good, ref, bound)))

    mutants = {}
    w1 = w.clone()
    w1[:, :, 1, 0] = 0.0
    halo = good.clone()
    halo[..., -1] = _standin(r, t, w1, shift)[..., -1]
    mutants["halo tap"] = halo
    w2 = w.clone()
    w2[:, r["c1"]:r["c1"] + 8] = 0.0
    mutants["K chunk"] = _standin(r, t, w2, shift)
    mutants["seed"] = _standin(r, t, w, shift, seed2=SEED)
    sh = good.clone()
    sh[:, -1] += shift[0] - shift[-1]
    mutants["shift of channel 0"] = sh
    row = good.clone()
    row[:, :, 1, :] = torch.roll(good[:, :, 1, :], 1, dims=-1)
    mutants["row shifted"] = row
    for what, bad in mutants.items():
        with pytest.raises(AssertionError):
            assert_ulps(bad, ref, bound, what)


# ------------------------------------------------------------------------------------------------ every instantiation
@pytest.fixture
def f32_scheme():
    """The scheme this family is the whole of (pack_weights then builds no split weight images)."""
    ops = _ops()
    before = ops.conv_precision()
    ops.set_conv_precision("f32")
    yield ops
    ops.set_conv_precision(before)


def _gather(ops, ly, y, x1=None):
    dv = ly.dev
    return ops._lib.lib().vunet_conv2d_gather(ctypes.byref(ly.desc), ops._p(dv["x1"] if x1 is None else x1), ops._p(dv["x2"]),
                                              ops._p(ly.wt), ops._p(ly.shift), ops._p(dv["res"]), ops._p(dv["aux"]),
                                              ops._p(y), ops._stream())


@gpu
@pytest.mark.parametrize("r", [x for x in GATHER_EVERY if not x["masked"]], ids=_id)
def test_every_gather_family_instantiation_vs_float64(r, f32_scheme):
    """vunet_conv2d_gather on the row's shape: the router names the row's kernel, the launch writes every output element
    (NaN pre-fill) and nothing in front of an offset view, and the result is within the derived bound of float64."""
    ops = f32_scheme
    ly = Layer(ops, r, 1000 + GATHER_EVERY.index(r))
    ops.set_tuning("tiled_force_nt", r["nt"])
    assert _variant(ops, ly.desc, r["aux_act"] is not None) == r["name"]
    buf, y = ly.new_out()
    assert _gather(ops, ly, y) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(y).any(), "output elements left unwritten"
    assert torch.isnan(buf[:r["yoff"]]).all()
    ref, bound = ly.reference()
    print("gather-family-ratio %s %s %.4f" % (_family(r["name"]), _id(r), _ratio(y, ref, bound)))
    assert_ulps(y, ref, bound, r["name"])


@gpu
@pytest.mark.parametrize("r", [x for x in GATHER_EVERY if x["masked"]], ids=_id)
def test_masked_data_gradient_vs_float64_and_two_passes(r, f32_scheme):
    """vunet_conv2d_dgrad_relu, dx = dgrad(dy * [y > 0]) (+ res): accepted (code 0), every element written, within the bound
    of the float64 value -- and so is the two-pass route (vunet_act_bwd_from_out, then vunet_conv2d_gather mode 1): the mask
    is a select, both compute the same sum."""
    ops = f32_scheme
    ly = Layer(ops, r, 1000 + GATHER_EVERY.index(r))
    ops.set_tuning("tiled_force_nt", r["nt"])
    assert _variant(ops, ly.desc, False).replace(", 1, 0, ", ", 1, 4, ") == r["name"]
    dv = ly.dev
    _, dx = ly.new_out()
    rc = ops._lib.lib().vunet_conv2d_dgrad_relu(ctypes.byref(ly.desc), ops._p(dv["x1"]), ops._p(dv["ymask"]), ops._p(ly.wt),
                                                ops._p(dv["res"]), ops._p(dx), ops._stream())
    assert rc == 0
    dym = torch.empty_like(dv["x1"])
    ops._call("vunet_act_bwd_from_out", ops._p(dv["ymask"]), ops._p(dv["x1"]), ops._p(dym), ACT_RELU, 0.0, dym.numel(),
              ops._stream())
    _, dx2 = ly.new_out()
    assert _gather(ops, ly, dx2, x1=dym) == 0
    torch.cuda.synchronize()
    assert not torch.isnan(dx).any() and not torch.isnan(dx2).any()
    ref, bound = ly.reference()
    print("gather-family-ratio tiled-masked %s %.4f" % (_id(r), max(_ratio(dx, ref, bound), _ratio(dx2, ref, bound))))
    assert_ulps(dx, ref, bound, r["name"])
    assert_ulps(dx2, ref, bound, r["name"] + " in two passes")


@gpu
def test_masked_data_gradient_refuses_what_the_tiled_kernel_does_not_take(f32_scheme):
    """A 9-wide map: VUNET_ERR_UNSUPPORTED and dx untouched (the caller then takes the two-pass route)."""
    ops = f32_scheme
    ly = Layer(ops, REFUSED_MASKED, 5)
    ops.set_tuning("tiled_force_nt", 1)
    dv = ly.dev
    dx = torch.full(ly.out_shape, 7.0, device="cuda")
    rc = ops._lib.lib().vunet_conv2d_dgrad_relu(ctypes.byref(ly.desc), ops._p(dv["x1"]), ops._p(dv["ymask"]), ops._p(ly.wt),
                                                ops._p(dv["res"]), ops._p(dx), ops._stream())
    torch.cuda.synchronize()
    assert rc == UNSUPPORTED
    assert bool((dx == 7.0).all())


# ------------------------------------------------------------------------------------------------ the published maxima
# vunet_conv2d with wx = NULL and an amax_out of 1024 floats: the fp32 producers whose |y| maxima the consumer's fp16 scale trusts
PUBLISHERS = {
    "1x1": _row("conv_1x1_kernel<1, 0, 0>", 2, 32, 0, 35, 8, 40, k=1, pad=0, res=True),        # the 16-byte epilogue, ragged M
    "tiled": _row("conv_tiled_kernel<2, 1, 8, 0, 0, 32, 1>", 2, 24, 0, 40, 4, 32, res=True, nt=1),
    "splitk": _row("conv_gather_splitk_kernel<16, 0, 3>", 2, 64, 0, 35, 5, 5, res=True),        # 50 pixels: a ragged pixel tile
    "thin_k": _row("conv_thin_k_kernel<3, 3>", 14, 3, 0, 40, 28, 176),
    "thin_kv": _row("conv_thin_kv_kernel<3, 4>", 11, 3, 0, 40, 36, 176, out_act=R_),
}
SILENT = {
    "gather": _row("conv_gather_kernel<2, 2, 0, 3>", 2, 33, 0, 35, 5, 9, res=True),
    "thin_m": _row("conv_thin_m_kernel<0>", 14, 8, 0, 3, 28, 176),
    "thin_mv": _row("conv_thin_mv_kernel<0, 4>", 11, 8, 0, 4, 36, 176),
    "phase": _PHASE_ROWS[0],
    "1x1-d2s": _row("conv_1x1_kernel<1, 0, 0>", 2, 32, 0, 32, 8, 8, k=1, pad=0, d2s=1),
    "tiled-d2s": _row("conv_tiled_kernel<1, 1, 8, 0, 0, 32, 1>", 2, 24, 0, 32, 4, 32, d2s=1, nt=1),
    "splitk-d2s": _row("conv_gather_splitk_kernel<16, 0, 3>", 2, 64, 0, 32, 4, 4, d2s=1),
}


def _conv2d_amax(ops, ly, amax, y=None):
    """vunet_conv2d, fp32 kernels only (wx = NULL), with ``amax`` as amax_out -> y."""
    if y is None:
        _, y = ly.new_out()
    dv = ly.dev
    ops._call("vunet_conv2d", ctypes.byref(ly.desc), ops._p(dv["x1"]), ops._p(dv["x2"]), ops._p(ly.wt), None, ops._p(ly.shift),
              ops._p(dv["res"]), ops._p(dv["aux"]), ops._p(y), None, ops._p(amax), ops._stream())
    torch.cuda.synchronize()
    return y


def _publishes(ops, ly):
    return ops._lib.lib().vunet_conv2d_publishes_amax(ctypes.byref(ly.desc), int(ly.dev["aux"] is not None),
                                                      int(ly.dev["res"] is not None), 0)


def _check_published(amax, y):
    assert float(amax[:512].max()) == float(torch.nan_to_num(y, nan=0.0).abs().max())   # exact: fp32 values of stored elements
    assert bool((amax[512:] == -1.0).all()), "the second source's half was touched"


def _amax_buf():
    a = torch.zeros(1024, device="cuda")
    a[512:] = -1.0
    return a


@gpu
@pytest.mark.parametrize("fam", list(PUBLISHERS))
def test_fp32_producers_publish_the_maximum_of_what_they_store(fam, f32_scheme):
    """One row per publishing family.  The query says 1; the first 512 floats hold max |y| of the stored tensor exactly, the
    other 512 stay.  With a residual larger than the convolution the maximum is that of the sum; one NaN in x is ignored
    (as vunet_absmax_partials ignores it); one +inf in the residual is published; a buffer that already holds a larger
    value keeps it (atomic max)."""
    ops = f32_scheme
    r = PUBLISHERS[fam]
    ops.set_tuning("tiled_force_nt", r["nt"])
    ly = Layer(ops, r, 77)
    assert _variant(ops, ly.desc, False) == r["name"]
    assert _publishes(ops, ly) == 1
    amax = _amax_buf()
    y = _conv2d_amax(ops, ly, amax)
    assert not torch.isnan(y).any()
    _check_published(amax, y)
    # a buffer that holds a larger value keeps it
    amax = _amax_buf()
    big = 2.0 * float(y.abs().max())
    amax[3] = big
    _conv2d_amax(ops, ly, amax)
    assert float(amax[:512].max()) == big
    # one NaN in x: it travels with the data, not with the scale
    ly.dev["x1"].view(-1)[ly.dev["x1"].numel() // 2] = float("nan")
    amax = _amax_buf()
    y = _conv2d_amax(ops, ly, amax)
    assert bool(torch.isnan(y).any()) == (r["out_act"] != ACT_RELU)   # (a ReLU epilogue, v > 0 ? v : 0, stores 0 for a NaN)
    _check_published(amax, y)
    ly.dev["x1"].copy_(ly.cpu["x1"])
    if r["res"]:
        ly.dev["res"].mul_(100.0)        # the residual dominates: the maximum is that of what is stored
        amax = _amax_buf()
        y = _conv2d_amax(ops, ly, amax)
        assert float(y.abs().max()) > 50.0
        _check_published(amax, y)
        ly.dev["res"].view(-1)[11] = float("inf")
        amax = _amax_buf()
        y = _conv2d_amax(ops, ly, amax)
        assert float(amax[:512].max()) == float("inf") and bool((amax[512:] == -1.0).all())


@gpu
@pytest.mark.parametrize("fam", ["1x1", "tiled", "splitk"])
def test_padded_rows_and_pixels_do_not_count_towards_the_maximum(fam, f32_scheme):
    """Ragged M (35 / 40) with shift[0] = 1e6: the padding rows of the last m-tile evaluate to 0 + shift[0] (load_tile_side4
    reads shift[ok ? ch : 0]), so a kernel that counted them would publish 1e6.  So that no STORED element is that large,
    channel 0 is built to cancel its shift exactly: its only weight is -1 on source channel 0 (centre tap), which no other
    channel reads and which holds 1e6 - j / 16 (exact in fp32), so y[:, 0] = j / 16 < 1.  The split-K row's 50 pixels leave a
    ragged pixel tile as well."""
    ops = f32_scheme
    r = dict(PUBLISHERS[fam], res=False)
    ops.set_tuning("tiled_force_nt", r["nt"])

    def edit(t):
        c = r["k"] // 2
        t["v"][:, 0] = 0.0
        t["v"][0] = 0.0
        t["v"][0, 0, c, c] = -1.0
        t["g"][0], t["gamma"][0, 0], t["beta"][0, 0], t["bias"][0] = 1.0, 1.0, 0.0, 1.0e6
        t["x1"][:, 0] = 1.0e6 - torch.randint(0, 16, t["x1"][:, 0].shape).float() / 16.0

    ly = Layer(ops, r, 78, edit)
    assert float(ly.shift[0]) == 1.0e6 and float(ly.w_eff[0, 0, r["k"] // 2, r["k"] // 2]) == -1.0
    assert _publishes(ops, ly) == 1
    amax = _amax_buf()
    y = _conv2d_amax(ops, ly, amax)
    assert float(y[:, 0].abs().max()) < 1.0 and float(y.abs().max()) < 100.0
    _check_published(amax, y)


@gpu
@pytest.mark.parametrize("fam", list(SILENT))
def test_kernels_that_do_not_publish_say_so_and_leave_the_buffer(fam, f32_scheme):
    """The one-wave gather kernel, conv_thin_m / conv_thin_mv, the phase launches and every depth-to-space store: the query
    answers 0 and an amax_out handed over all the same keeps its sentinel."""
    ops = f32_scheme
    r = SILENT[fam]
    ops.set_tuning("tiled_force_nt", r["nt"])
    ly = Layer(ops, r, 79)
    assert _variant(ops, ly.desc, False) == r["name"]
    assert _publishes(ops, ly) == 0
    amax = torch.full((1024,), -1.0, device="cuda")
    y = _conv2d_amax(ops, ly, amax)
    assert not torch.isnan(y).any()
    assert bool((amax == -1.0).all())


@gpu
def test_a_1x1_producers_tag_serves_the_h2_consumer():
    """A 1x1 NormConv2d feeds a 3x3 NormConv2d of the fp16 scheme.  The 1x1 layer has no split kernel in any scheme: it runs
    conv_1x1_kernel of the fp32 family, whose published maxima ops tags y with, and the consumer then launches no
    vunet_absmax_partials of its own.  The chain is within test_hip_x6.py's 3e-6 of float64.

    ops asks a producer for maxima only while the process-wide scheme is "h2" (ops._conv_gather), so the producer runs under
    "h2" here.  Under set_conv_precision("f32") it leaves y untagged -- nothing is published that a later consumer could
    trust by mistake -- and the consumer makes its one pass: asserted as well, with the same accuracy."""
    ops = _ops()
    from behavior_driven_video_synthesis_amd.lib.modules import NormConv2d
    torch.manual_seed(12)
    conv1 = NormConv2d(32, 64, 1).cuda()
    conv2 = NormConv2d(64, 64, 3, padding=1).cuda()
    x = torch.randn(8, 32, 64, 64, device="cuda") * 3.0

    def chain64():
        def wn(c):
            v, g = c.conv.weight_v.detach().double().cpu(), c.conv.weight_g.detach().double().cpu()
            w = v * (g / v.flatten(1).norm(dim=1).view(-1, 1, 1, 1))
            return w, c.conv.bias.detach().double().cpu(), c.gamma.detach().double().cpu(), c.beta.detach().double().cpu()
        t = x.double().cpu()
        for c, pad in ((conv1, 0), (conv2, 1)):
            w, b, gm, be = wn(c)
            t = gm * F.conv2d(t, w, b, padding=pad) + be
        return t

    ref = chain64()
    before = ops.conv_precision()
    calls = []
    orig = ops.absmax_partials
    ops.absmax_partials = lambda *a: (calls.append(1), orig(*a))[1]
    try:
        for producer, passes in (("h2", 0), ("f32", 1)):
            with torch.no_grad():
                ops.set_conv_precision(producer)
                ops.profile_start()
                y = conv1(x)
                kernels = ops.profile_stop(by_kernel=True)
                assert any(k_.startswith("conv_1x1_kernel<") for k_ in kernels), kernels
                tag = ops._tagged_amax(y)
                if producer == "h2":
                    assert tag is not None and float(tag[:512].max()) == float(y.abs().max()) and float(tag[512:].max()) == 0.0
                else:
                    assert tag is None
                ops.set_conv_precision("h2")
                del calls[:]
                ops.profile_start()
                z = conv2(y)
                kernels = ops.profile_stop(by_kernel=True)
                assert any(k_.startswith("conv_h2_kernel<") for k_ in kernels), kernels
                assert len(calls) == passes
            assert float((z.double().cpu() - ref).abs().max()) <= 3e-6 * max(float(ref.abs().max()), 1.0)
            assert_close(z, ref.float(), rtol=1e-4, atol=1e-4 * max(float(ref.abs().max()), 1.0), name="chain")
    finally:
        ops.absmax_partials = orig
        ops.set_conv_precision(before)
