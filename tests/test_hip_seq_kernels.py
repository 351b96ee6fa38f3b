"""-m gpu: the behaviour path's sequence kernels (csrc/seq.hip, csrc/seq_bptt.hip, csrc/seq_train.hip) one entry point at a time,
through the C ABI, against float64 torch on the CPU computing the formula in the kernel's comment.

Conventions (those of tests/test_hip_pointwise.py; U = 2^-24, the unit roundoff of fp32):
  * index and copy ops: bit-exact;
  * reductions: c * U * sum|terms|, c = the depth of the kernel's summation chain, written out at each test;
  * transcendentals: OCML's float functions are built to the OpenCL full-profile accuracy table (ROCm-Device-Libs doc/OCML.md;
    OpenCL C 1.2 section 7.4): exp <= 3 ulp, log <= 3 ulp, tanh <= 5 ulp, sqrt <= 3 ulp, x / y <= 2.5 ulp.  One ulp of a result r
    is at most 2 U |r|, so: expf 6 U, logf 6 U, tanhf 10 U, sqrtf 6 U, division 5 U, relative to the result.
    sigmoid_f(x) = 1 / (1 + expf(-x)): e = expf(-x) carries 6 U e, the sum U (1 + e), the division 5 U: at most 12 U relative.
  * every output is pre-filled with NaN (an unwritten element shows) and followed by a guard band of 256 sentinels;
  * kernels that work on Bp = ceil16(B) rows run with the padding rows of every input at 0 and at NaN: rows < B of every output
    are bit-equal between the two (a batch row never depends on another);
  * float64 backward references come from torch.autograd on the float64 forward formula;
  * tile-major images are built and read back by ``to_tiles`` / ``from_tiles`` below, written from the index formula of
    include/vunet_seq_tiled.h -- never by the kernel under test.

The census in tests/test_cabi_and_host.py requires every ``extern "C" int vunet_*`` of the three files to be named here or listed
in NOT_HELD with a reason.
"""
import ctypes
import math
import random

import pytest
import torch

from hip_parity_utils import (DIV_U, ERR_ARG, ERR_UNSUPPORTED, EXP_U, LOG_U, NAN, SIG_U, SQRT_U, TANH_U, TINY, U, Outs, _adam64,
                              _adam_hp, _d, _f32, _refused, assert_same, assert_ulps)

pytestmark = pytest.mark.gpu

SLOPE = float(torch.tensor(0.01, dtype=torch.float32))   # 0.01f, the kernels' LeakyReLU slope

NOT_HELD = {
    "vunet_seq_dw": "held by tests/test_hip_seq_train.py::test_dw_kernel_write_mode_vs_float64 (alone, against float64)",
}


def _m():
    from behavior_driven_video_synthesis_amd import ops, seq, seq_train
    return ops, seq, seq_train


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def _up16(b):
    return (b + 15) // 16 * 16


def _cdiv(a, b):
    return (a + b - 1) // b


# (Outs, assert_same, _d, _refused, the constants, _adam_hp and _adam64 live in tests/hip_parity_utils.py: tests/
# test_hip_cls_reg_kernels.py works under the same conventions)


# ------------------------------------------------------------------------------------------------ tile-major images
def to_tiles(w):
    """include/vunet_seq_tiled.h: wt[mt][c][h][l][e] = w[16 mt + (l & 15)][32 c + 8 (l >> 4) + 4 h + e], flat.
    Row 16 mt + i, column 32 c + 8 s + 4 h + e  ->  [mt][c][h][16 s + i][e]."""
    m, k = w.shape
    return w.reshape(m // 16, 16, k // 32, 4, 2, 4).permute(0, 2, 4, 3, 1, 5).reshape(-1).contiguous()


def from_tiles(t, m, k):
    return t.reshape(m // 16, k // 32, 2, 4, 16, 4).permute(0, 4, 1, 3, 2, 5).reshape(m, k).contiguous()


def test_tile_helpers_follow_the_index_formula():
    """The helpers against the header's formula spelled out element by element (host arithmetic only)."""
    m, k = 32, 96
    w = torch.arange(m * k, dtype=torch.float32).reshape(m, k)
    t = to_tiles(w).reshape(m // 16, k // 32, 2, 64, 4)
    for (mt, c, h, l, e) in ((0, 0, 0, 0, 0), (1, 2, 1, 63, 3), (0, 1, 1, 17, 2), (1, 0, 0, 40, 1)):
        assert t[mt, c, h, l, e] == w[16 * mt + (l & 15), 32 * c + 8 * (l >> 4) + 4 * h + e]
    assert torch.equal(from_tiles(t.reshape(-1), m, k), w)


# ================================================================================================ a. index and copy ops
@pytest.mark.parametrize("M,K,ld", [(16, 32, 32), (48, 96, 100), (64, 1088, 1088)])
def test_pack_tiles_bit_exact(M, K, ld):
    """vunet_seq_pack_tiles against ``to_tiles``; columns K .. ld of the source are not read into the image."""
    ops, _, _ = _m()
    w = _randn(_gen(M + K), M, ld)
    o = Outs()
    wt = o.new(M * K)
    ops._call("vunet_seq_pack_tiles", ops._p(_d(w)), ld, M, K, ops._p(wt), ops._stream())
    o.check()
    assert_same(wt, to_tiles(w[:, :K].contiguous()), "pack_tiles")


PACK_SHAPES = [(1, 1), (5, 51), (1, 257), (20, 51)]      # M K = 1, 255, 257, 4 * 51 * 5


@pytest.mark.parametrize("M,K", PACK_SHAPES)
@pytest.mark.parametrize("scaled", [False, True])
def test_pack_rows_bit_exact(M, K, scaled):
    """vunet_seq_pack_rows: dst[row_off + row_mul m][col_off + k] = src[m][k] (* row_scale[m]: one fp32 product, which
    (double product).float() is exactly); row_mul 1 and 4 with every row_off, col_off > 0; everything else stays NaN."""
    ops, _, _ = _m()
    g = _gen(M * K)
    src, scale = _randn(g, M, K), _randn(g, M)
    val = (src.double() * scale.double()[:, None]).float() if scaled else src
    for row_mul, row_off, col_off in [(1, 0, 0), (1, 2, 3)] + [(4, q, 5 * (q & 1)) for q in range(4)]:
        rows, ld = row_off + row_mul * (M - 1) + 1, col_off + K + 2
        o = Outs()
        dst = o.new(rows, ld)
        ops._call("vunet_seq_pack_rows", ops._p(_d(src)), M, K, ops._p(_d(scale) if scaled else None), ops._p(dst), ld, col_off,
                  row_off, row_mul, ops._stream())
        o.check()
        want = torch.full((rows, ld), NAN)
        want[row_off::row_mul, col_off:col_off + K] = val
        assert_same(dst, want, f"pack_rows mul {row_mul} off {row_off} col {col_off}")


@pytest.mark.parametrize("M,K", PACK_SHAPES)
@pytest.mark.parametrize("accumulate", [0, 1])
def test_unpack_rows_bit_exact(M, K, accumulate):
    """vunet_seq_unpack_rows: dst[m][k] = src[(row_off + row_mul m) ld + col_off + k], or one fp32 add onto dst."""
    ops, _, _ = _m()
    g = _gen(M * K + 1)
    for row_mul, row_off, col_off in [(1, 0, 0), (1, 2, 3)] + [(4, q, 5 * (q & 1)) for q in range(4)]:
        rows, ld = row_off + row_mul * (M - 1) + 1, col_off + K + 2
        src, dst0 = _randn(g, rows, ld), _randn(g, M, K)
        o = Outs()
        dst = o.load(_d(dst0)) if accumulate else o.new(M, K)
        ops._call("vunet_seq_unpack_rows", ops._p(_d(src)), ld, col_off, row_off, row_mul, ops._p(dst), M, K, accumulate,
                  ops._stream())
        o.check()
        v = src[row_off::row_mul, col_off:col_off + K]
        assert_same(dst, dst0 + v if accumulate else v, f"unpack_rows mul {row_mul} off {row_off} col {col_off}")


@pytest.mark.parametrize("H", [4, 63, 64])
@pytest.mark.parametrize("fold", [False, True])
def test_lstm_bias_bit_exact(H, fold):
    """vunet_seq_lstm_bias: out[4 j + q] = (b_ih[q H + j] + b_hh[q H + j]) (+ fold[q H + j]): fp32 adds in that order."""
    ops, _, _ = _m()
    g = _gen(H)
    bi, bh, fo = _randn(g, 4 * H), _randn(g, 4 * H), _randn(g, 4 * H)
    o = Outs()
    out = o.new(4 * H)
    ops._call("vunet_seq_lstm_bias", ops._p(_d(bi)), ops._p(_d(bh)), ops._p(_d(fo) if fold else None), H, ops._p(out),
              ops._stream())
    o.check()
    v = bi + bh
    if fold:
        v = v + fo
    assert_same(out, v.view(4, H).t().contiguous().view(-1), "lstm_bias")


@pytest.mark.parametrize("n,hoff,H,ldx", [(3, 4, 4, 9), (51, 64, 32, 96), (10, 12, 20, 40)])
def test_lstm_grads_unpack_bit_exact(n, hoff, H, ldx):
    """vunet_seq_lstm_grads_unpack: torch row q H + j <- image row 4 j + q; dW_ih from columns 0 .. n, dW_hh from hoff .. hoff + H,
    both bias gradients from the image's bias gradient."""
    ops, _, _ = _m()
    g = _gen(n + H)
    gimg, gb = _randn(g, 4 * H, ldx), _randn(g, 4 * H)
    o = Outs()
    dwih, dwhh, dbih, dbhh = o.new(4 * H, n), o.new(4 * H, H), o.new(4 * H), o.new(4 * H)
    ops._call("vunet_seq_lstm_grads_unpack", ops._p(_d(gimg)), ops._p(_d(gb)), ldx, hoff, n, H, ops._p(dwih), ops._p(dwhh),
              ops._p(dbih), ops._p(dbhh), ops._stream())
    o.check()
    perm = gimg.view(H, 4, ldx).permute(1, 0, 2).reshape(4 * H, ldx)          # row q H + j <- row 4 j + q
    assert_same(dwih, perm[:, :n], "dW_ih")
    assert_same(dwhh, perm[:, hoff:hoff + H], "dW_hh")
    pb = gb.view(H, 4).t().reshape(-1)
    assert_same(dbih, pb, "db_ih")
    assert_same(dbhh, pb, "db_hh")


@pytest.mark.parametrize("H", [4, 300])
@pytest.mark.parametrize("given", [(True, True, True), (False, False, False), (True, False, True), (False, True, False)])
def test_seq_start_bit_exact(H, given):
    """vunet_seq_start: xh[b] = [x0 | . | h0 or 0], c = c0 or 0, xraw = x0 (x0 rows x0_stride > n apart); the columns between
    n and hoff, beyond hoff + H and beyond n of xraw are not written."""
    ops, _, _ = _m()
    h0_on, c0_on, raw_on = given
    B, n, stride, hoff, ldraw = 3, 51, 60, 56, 53
    ldx = hoff + H + 2
    g = _gen(H)
    x0, h0, c0 = _randn(g, B, stride), _randn(g, B, H), _randn(g, B, H)
    o = Outs()
    xh, c, xraw = o.new(B, ldx), o.new(B, H), o.new(B, ldraw)
    ops._call("vunet_seq_start", ops._p(_d(x0)), stride, ops._p(_d(h0) if h0_on else None), ops._p(_d(c0) if c0_on else None),
              ops._p(xraw if raw_on else None), ldraw, ops._p(xh), ldx, hoff, ops._p(c), B, n, H, ops._stream())
    o.check()
    want = torch.full((B, ldx), NAN)
    want[:, :n] = x0[:, :n]
    want[:, hoff:hoff + H] = h0 if h0_on else 0.0
    assert_same(xh, want, "xh")
    assert_same(c, c0 if c0_on else torch.zeros(B, H), "c")
    wraw = torch.full((B, ldraw), NAN)
    if raw_on:
        wraw[:, :n] = x0[:, :n]
    assert_same(xraw, wraw, "xraw")


# ================================================================================================ b. the skinny linear layer
def _waves(B, kb):
    return 16 if kb >= 512 and B <= 32 else 4                     # seq_linear_launch: ``wide``


def _lin_c(B, kb):
    """Chain of one output: a wave adds its ceil(nchunk / WAVES) chunks of 32 products one after the other, the WAVES partials
    are added in wave order, then the bias; + 2 for the products' own roundings in the matrix unit."""
    w = _waves(B, kb)
    return 32 * _cdiv(kb // 32, w) + w + 2


def _act64(v, act):
    if act == 1:
        return torch.maximum(v, SLOPE * v)
    if act == 2:
        return torch.tanh(v)
    if act == 3:
        return torch.clamp_min(v, 0.0)
    return v


def _act_bound(pre_bound, ref, act):
    """Every activation is 1-Lipschitz: the pre-activation bound carries over; + LeakyReLU's product (U), + tanhf (TANH_U)."""
    return pre_bound + {0: 0.0, 1: U, 2: TANH_U, 3: 0.0}[act] * ref.abs() + TINY


LINEAR_CASES = ([(b, k) for k in (32, 160, 480) for b in (1, 17)]              # four waves, 1 - 2 batch tiles
                + [(b, k) for k in (512, 544, 1088) for b in (16, 32)] + [(5, 3584)]   # sixteen waves
                + [(b, k) for k in (32, 64, 160, 352, 1088, 2048) for b in (33, 64)])  # four waves with the ring
# nets, shared_in, (act0, act1), index of the NULL bias (None: both given)
LINEAR_VARIANTS = [(1, 1, (1, 0), None), (2, 1, (2, 0), 1), (2, 0, (0, 3), 0), (1, 1, (3, 0), 0), (2, 0, (1, 2), None),
                   (2, 1, (3, 1), None)]


def _linear_operands(seed, B, M, K, nets, nin):
    g = _gen(seed)
    ldx = K + 8
    x = _randn(g, nin, _up16(B), ldx)                     # (columns K .. ldx: not the layer's)
    w = _randn(g, nets, M, K, scale=1.0 / math.sqrt(K))
    bias = _randn(g, nets, M)
    return x, w, bias, ldx


def _run_linear(ops, S, layout, B, M, K, ldx, var, x, w, bias, pad, split=1, rowmajor_copy=False):
    """One launch; returns (y as [nets][split][Bp][M] row-major -- un-tiled by ``from_tiles`` with bit 4 --, y_rowmajor)."""
    nets, shared, acts, nobias = var
    Bp = _up16(B)
    xp = x.clone()
    xp[:, B:] = pad
    xop = torch.stack([to_tiles(xi[:, :K].contiguous()) for xi in xp]) if layout & 2 else xp
    wop = [to_tiles(w[n]) if layout & 1 else w[n] for n in range(nets)]
    wd = [_d(t) for t in wop]
    bd = [None if nobias == n else _d(bias[n]) for n in range(nets)]
    o = Outs()
    y = o.new(nets, split, Bp, M)
    y2 = o.new(nets, Bp, M) if rowmajor_copy else None
    d = S.SeqLinearDesc(B, M, K, ldx, acts[0], acts[1], nets, shared, split)
    xd = _d(xop)
    if layout == 0:
        ops._call("vunet_seq_linear", ctypes.byref(d), ops._p(wd[0]), ops._p(wd[1] if nets > 1 else None), ops._p(xd), ops._p(bd[0]),
                  ops._p(bd[1] if nets > 1 else None), ops._p(y), ops._stream())
    else:
        ops._call("vunet_seq_linear_tiled", ctypes.byref(d), layout, ops._p(wd[0]), ops._p(wd[1] if nets > 1 else None), ops._p(xd),
                  ops._p(bd[0]), ops._p(bd[1] if nets > 1 else None), ops._p(y), ops._p(y2), ops._stream())
    o.check()
    y = y.cpu()
    if layout & 4:
        y = torch.stack([from_tiles(y[n].reshape(-1), Bp, M) for n in range(nets)]).view(nets, 1, Bp, M)
    return y, (None if y2 is None else y2.cpu())


@pytest.mark.parametrize("B,K", LINEAR_CASES)
def test_linear_every_layout_vs_float64(B, K):
    """vunet_seq_linear and vunet_seq_linear_tiled (layouts 2 - 7): act(x w^T + b) against float64 within
    (32 ceil(nchunk / WAVES) + WAVES + 2) U (sum_k |x_k w_k| + |b|) carried through the activation; every layout bit-equal to
    layout 0 after un-tiling (the header's promise), y_rowmajor bit-equal to the tile-major output; padding rows at 0 and at
    NaN leave rows < B bit-equal.  M = 16, 48 (no bit 4), 32, 64 (every layout); the variants rotate nets / shared_in / the
    four activations / a NULL bias over the cases."""
    ops, S, _ = _m()
    case = LINEAR_CASES.index((B, K))
    Bp = _up16(B)
    for mi, M in enumerate((16, 48, 32, 64)):
        var = LINEAR_VARIANTS[(case * 4 + mi) % len(LINEAR_VARIANTS)]
        nets, shared, acts, nobias = var
        nin = 1 if (shared or nets == 1) else nets
        x, w, bias, ldx = _linear_operands(1000 * case + M, B, M, K, nets, nin)
        refs = []
        for n in range(nets):
            xi = x[n if nin > 1 else 0][:B, :K].double()
            b64 = torch.zeros(M, dtype=torch.float64) if nobias == n else bias[n].double()
            pre = xi @ w[n].double().t() + b64
            mag = xi.abs() @ w[n].double().abs().t() + b64.abs()
            ref = _act64(pre, acts[n])
            refs.append((ref, _act_bound(_lin_c(B, K) * U * mag, ref, acts[n])))
        base = None
        for layout in ((0, 2, 3) if M % 32 else (0, 2, 3, 4, 5, 6, 7)):
            copy = bool(layout & 4) and layout != 5                      # y_rowmajor given (4, 6, 7) and NULL (5)
            y0, y20 = _run_linear(ops, S, layout, B, M, K, ldx, var, x, w, bias, 0.0, rowmajor_copy=copy)
            yn, y2n = _run_linear(ops, S, layout, B, M, K, ldx, var, x, w, bias, NAN, rowmajor_copy=copy)
            tag = f"B {B} M {M} K {K} layout {layout} {var}"
            assert not torch.isnan(y0).any(), f"{tag}: unwritten output"
            assert_same(yn[:, :, :B], y0[:, :, :B], f"{tag}: rows < B depend on the padding rows")
            if copy:
                assert_same(y20, y0.view(nets, Bp, M), f"{tag}: y_rowmajor")
                assert_same(y2n[:, :B], y0.view(nets, Bp, M)[:, :B], f"{tag}: y_rowmajor, NaN padding")
            if base is None:
                base = y0
                for n in range(nets):
                    assert_ulps(y0[n, 0, :B], refs[n][0], refs[n][1], f"{tag} net {n}")
            else:
                assert_same(y0, base, f"{tag}: differs from layout 0")


@pytest.mark.parametrize("K,split", [(2048, 4), (512, 8), (128, 2)])
@pytest.mark.parametrize("B", [16, 64])
def test_linear_split_k_slabs_vs_float64(B, K, split):
    """S > 1 (layouts 0, 2, 3): y = [nets][S][Bp][M] RAW slabs -- slab s is the product over columns s K / S .. (s + 1) K / S,
    no bias (given here: it must not be added), no activation (tanh asked for: it must not be applied).  Bound as above with
    nchunk = K / S / 32."""
    ops, S, _ = _m()
    kb = K // split
    for M, var in ((16, (1, 1, (2, 0), None)), (64, (2, 1, (2, 1), None)), (48, (2, 0, (0, 2), 1))):
        nets, shared, _, _ = var
        nin = 1 if (shared or nets == 1) else nets
        x, w, bias, ldx = _linear_operands(B + K + M, B, M, K, nets, nin)
        base = None
        for layout in (0, 2, 3):
            y0, _ = _run_linear(ops, S, layout, B, M, K, ldx, var, x, w, bias, 0.0, split=split)
            yn, _ = _run_linear(ops, S, layout, B, M, K, ldx, var, x, w, bias, NAN, split=split)
            tag = f"B {B} M {M} K {K} S {split} layout {layout}"
            assert not torch.isnan(y0).any(), f"{tag}: unwritten output"
            assert_same(yn[:, :, :B], y0[:, :, :B], f"{tag}: rows < B depend on the padding rows")
            if base is not None:
                assert_same(y0, base, f"{tag}: differs from layout 0")
                continue
            base = y0
            for n in range(nets):
                for s in range(split):
                    xi = x[n if nin > 1 else 0][:B, s * kb:(s + 1) * kb].double()
                    ws = w[n][:, s * kb:(s + 1) * kb].double()
                    assert_ulps(y0[n, s, :B], xi @ ws.t(), _lin_c(B, kb) * U * (xi.abs() @ ws.abs().t()) + TINY, f"{tag} net {n} slab {s}")


def test_linear_refusals():
    """What seq_linear_launch documents, all before any launch: layout 1 -> UNSUPPORTED; bit 4 with S > 1 or M % 32, B = 65,
    K % (32 S), y_rowmajor without bit 4 -> ARG."""
    ops, S, _ = _m()
    buf = torch.zeros(1 << 16, device="cuda")
    p, st = ops._p(buf), ops._stream()

    def tiled(code, layout, B, M, K, split, y2):
        d = S.SeqLinearDesc(B, M, K, K, 0, 0, 1, 1, split)
        _refused(ops, code, "vunet_seq_linear_tiled", ctypes.byref(d), layout, p, None, p, p, None, p, y2, st)

    tiled(ERR_UNSUPPORTED, 1, 16, 32, 64, 1, None)
    tiled(ERR_ARG, 4, 16, 32, 64, 2, None)
    tiled(ERR_ARG, 6, 16, 48, 64, 1, None)
    tiled(ERR_ARG, 2, 65, 32, 64, 1, None)
    tiled(ERR_ARG, 3, 16, 32, 96, 2, None)
    tiled(ERR_ARG, 2, 16, 32, 64, 1, p)
    d = S.SeqLinearDesc(65, 32, 64, 64, 0, 0, 1, 1, 1)
    _refused(ops, ERR_ARG, "vunet_seq_linear", ctypes.byref(d), p, None, p, p, None, p, st)
    d = S.SeqLinearDesc(16, 32, 80, 80, 0, 0, 1, 1, 1)
    _refused(ops, ERR_ARG, "vunet_seq_linear", ctypes.byref(d), p, None, p, p, None, p, st)


# ================================================================================================ c. the LSTM step
def _lstm_problem(n, hoff, H, B, seed):
    g = _gen(seed)
    ldx, Bp = hoff + H, _up16(B)
    return dict(n=n, hoff=hoff, H=H, B=B, Bp=Bp, ldx=ldx, stride=n + 3,
                w=_randn(g, 4 * H, ldx, scale=2.0 / math.sqrt(ldx)), bias=_randn(g, 4 * H), xh=_randn(g, Bp, ldx),
                c=_randn(g, Bp, H), x_next=_randn(g, B, n + 3))


def _lstm_ref(p):
    """torch.nn.LSTMCell's arithmetic in float64 on the gate-interleaved image (row 4 j + q = gate q of unit j: i, f, g, o), and
    the bounds.  e: the pre-activation bound of the linear kernel (K = ldx).  sigmoid is 1/4-Lipschitz, tanh 1-Lipschitz."""
    B, H = p["B"], p["H"]
    x, w, b, c = p["xh"][:B].double(), p["w"].double(), p["bias"].double(), p["c"][:B].double()
    pre = (x @ w.t() + b).view(B, H, 4)
    e = (_lin_c(B, p["ldx"]) * U * (x.abs() @ w.abs().t() + b.abs())).view(B, H, 4)
    si, sf, tg, so = pre[..., 0].sigmoid(), pre[..., 1].sigmoid(), pre[..., 2].tanh(), pre[..., 3].sigmoid()
    dsi, dsf, dso = (e[..., q] / 4 + SIG_U * s for q, s in ((0, si), (1, sf), (3, so)))
    dtg = e[..., 2] + TANH_U * tg.abs()
    c2 = sf * c + si * tg
    # two products and a sum on top of the factors' errors: 3 U (|sf c| + |si tg|)
    dc2 = c.abs() * dsf + tg.abs() * dsi + si * dtg + 3 * U * ((sf * c).abs() + (si * tg).abs())
    tc = c2.tanh()
    h = so * tc
    dh = tc.abs() * dso + so * (dc2 + TANH_U * tc.abs()) + 2 * U * h.abs()
    gates = torch.stack([si, sf, tg, so], dim=-1)
    dgates = torch.stack([dsi, dsf, dtg, dso], dim=-1)
    return dict(c=c2, dc=dc2 + TINY, h=h, dh=dh + TINY, gates=gates, dgates=dgates + TINY)


def _run_lstm(ops, S, p, entry, pad, ht_in=False, ht_out=False, with_h_out=True, with_x_next=True):
    B, Bp, H, n, hoff, ldx = p["B"], p["Bp"], p["H"], p["n"], p["hoff"], p["ldx"]
    xh, c = p["xh"].clone(), p["c"].clone()
    xh[B:], c[B:] = pad, pad
    tiled = entry in ("vunet_seq_lstm_gates_tiled", "vunet_seq_lstm_gates_tiled_h")
    wd = (to_tiles(p["w"]) if tiled else p["w"]).cuda()
    o = Outs()
    c_out, xh_next = o.new(Bp, H), o.new(Bp, ldx)
    h_out = o.new(Bp, H) if with_h_out else None
    gates = o.new(Bp, H, 4) if entry != "vunet_seq_lstm_gates" else None
    hto = o.new(Bp * H) if ht_out else None
    hti = to_tiles(xh[:, hoff:].contiguous()).cuda() if ht_in else None
    xn = _d(p["x_next"]) if with_x_next else None
    d = S.SeqLstmDesc(B, H, ldx, hoff, n, n, p["stride"])
    a = [ctypes.byref(d), ops._p(wd), ops._p(_d(xh))]
    if entry == "vunet_seq_lstm_gates_tiled_h":
        a.append(ops._p(hti))
    a += [ops._p(_d(p["bias"])), ops._p(_d(c)), ops._p(c_out), ops._p(xh_next)]
    if entry == "vunet_seq_lstm_gates_tiled_h":
        a.append(ops._p(hto))
    a += [ops._p(h_out), ops._p(xn)]
    if entry != "vunet_seq_lstm_gates":
        a.append(ops._p(gates))
    ops._call(entry, *a, ops._stream())
    o.check()
    return dict(c=c_out.cpu(), xh_next=xh_next.cpu(), h_out=None if h_out is None else h_out.cpu(),
                gates=None if gates is None else gates.cpu(), ht=None if hto is None else from_tiles(hto.cpu(), Bp, H))


LSTM_CASES = ([(51, 64, 32, b) for b in (1, 17, 33, 48, 64)]       # 3 chunks; 8 workgroups: the x_next loop wraps for B > 8
              + [(51, 64, 448, b) for b in (16, 32, 64)]            # 16 chunks: sixteen waves (B <= 32), the ring (64)
              + [(51, 64, 1024, 64)]                                # ldx = 1088: 34 chunks, ch0 = 2 (LAY = 25 with h tiles)
              + [(10, 12, 20, b) for b in (5, 40)])                 # hoff % 32 != 0: row-major operand only


@pytest.mark.parametrize("n,hoff,H,B", LSTM_CASES)
def test_lstm_step_every_entry_point_vs_float64(n, hoff, H, B):
    """vunet_seq_lstm_gates, vunet_seq_lstm_gates_train, vunet_seq_lstm_gates_tiled and vunet_seq_lstm_gates_tiled_h (first
    step: h_tiles_in NULL; later step: h_tiles_in given -- read at 48 / 64 rows, ignored at <= 32) on the same inputs: c', h (in
    xh_next at hoff, in h_out, in h_tiles_out un-tiled), the kept gates in the order sig(i), sig(f), tanh(g), sig(o), the copy
    of x_next into xh_next[:B, :n].  All entry points agree bit for bit; the first is held to float64."""
    ops, S, _ = _m()
    p = _lstm_problem(n, hoff, H, B, 7 * H + B)
    ref = _lstm_ref(p)
    tiles_ok = hoff % 32 == 0 and H % 32 == 0
    runs = [("vunet_seq_lstm_gates", {}), ("vunet_seq_lstm_gates", dict(with_h_out=False, with_x_next=False)),
            ("vunet_seq_lstm_gates_train", {}), ("vunet_seq_lstm_gates_tiled", {}),
            ("vunet_seq_lstm_gates_tiled_h", dict(ht_out=tiles_ok)), ("vunet_seq_lstm_gates_tiled_h", dict(ht_in=tiles_ok, ht_out=tiles_ok))]
    base = None
    for entry, kw in runs:
        r0 = _run_lstm(ops, S, p, entry, 0.0, **kw)
        rn = _run_lstm(ops, S, p, entry, NAN, **kw)
        tag = f"{entry} {kw} n {n} hoff {hoff} H {H} B {B}"
        hcol = r0["xh_next"][:, hoff:]
        assert not torch.isnan(r0["c"]).any() and not torch.isnan(hcol).any(), f"{tag}: unwritten output"
        for k in ("c", "xh_next", "h_out", "gates", "ht"):
            if r0[k] is not None:
                assert_same(rn[k][:B], r0[k][:B], f"{tag}: rows < B of {k} depend on the padding rows")
        want_x = torch.full((p["Bp"], hoff), NAN)
        if kw.get("with_x_next", True):
            want_x[:B, :n] = p["x_next"][:, :n]
        assert_same(r0["xh_next"][:, :hoff], want_x, f"{tag}: the x part of xh_next")
        if r0["h_out"] is not None:
            assert_same(r0["h_out"], hcol, f"{tag}: h_out")
        if r0["ht"] is not None:
            assert_same(r0["ht"], hcol, f"{tag}: h_tiles_out")
        if base is None:
            base = r0
            assert_ulps(r0["c"][:B], ref["c"], ref["dc"], f"{tag} c'")
            assert_ulps(hcol[:B], ref["h"], ref["dh"], f"{tag} h")
        else:
            assert_same(r0["c"], base["c"], f"{tag}: c' differs from vunet_seq_lstm_gates")
            assert_same(hcol, base["xh_next"][:, hoff:], f"{tag}: h differs from vunet_seq_lstm_gates")
        if r0["gates"] is not None:
            assert_ulps(r0["gates"][:B], ref["gates"], ref["dgates"], f"{tag} gates")
            if base.get("gates") is None:
                base["gates"] = r0["gates"]
            assert_same(r0["gates"], base["gates"], f"{tag}: gates differ between entry points")


def test_lstm_refusals():
    """c_in == c_out, xh_next == xh, ldx % 32, h tiles with H % 32: VUNET_ERR_ARG before any launch."""
    ops, S, _ = _m()
    a, b, c, e = (torch.zeros(1 << 14, device="cuda") for _ in range(4))
    pa, pb, pc, pe, st = ops._p(a), ops._p(b), ops._p(c), ops._p(e), ops._stream()
    ok = S.SeqLstmDesc(4, 32, 96, 64, 51, 51, 51)
    _refused(ops, ERR_ARG, "vunet_seq_lstm_gates", ctypes.byref(ok), pa, pb, pa, pc, pc, pe, None, None, st)
    _refused(ops, ERR_ARG, "vunet_seq_lstm_gates", ctypes.byref(ok), pa, pb, pa, pc, pe, pb, None, None, st)
    _refused(ops, ERR_ARG, "vunet_seq_lstm_gates_train", ctypes.byref(ok), pa, pb, pa, pc, pe, pb, None, None, pa, st)
    _refused(ops, ERR_ARG, "vunet_seq_lstm_gates_tiled", ctypes.byref(ok), pa, pb, pa, pc, pc, pe, None, None, None, st)
    bad_ld = S.SeqLstmDesc(4, 20, 40, 12, 10, 10, 10)
    d2 = torch.zeros(1 << 14, device="cuda")
    for entry, extra in (("vunet_seq_lstm_gates", ()), ("vunet_seq_lstm_gates_tiled", (None,))):
        _refused(ops, ERR_ARG, entry, ctypes.byref(bad_ld), pa, pb, pa, pc, pe, ops._p(d2), None, None, *extra, st)
    bad_h = S.SeqLstmDesc(4, 20, 64, 32, 10, 10, 10)                # H % 32 != 0 with tiles wanted
    _refused(ops, ERR_ARG, "vunet_seq_lstm_gates_tiled_h", ctypes.byref(bad_h), pa, pb, None, pa, pc, pe, ops._p(d2), pa, None, None,
             None, st)
    _refused(ops, ERR_ARG, "vunet_seq_lstm_gates_tiled_h", ctypes.byref(ok), pa, pb, pa, pa, pc, pc, ops._p(d2), None, None, None,
             None, st)


# ================================================================================================ d. the coupling step
def _heads64(st, bias_s, bias_t, S, B, q):
    """(pre-tanh z or None, s, t, |terms| of z, |terms| of t) of the first q head columns, float64."""
    if S == 1:
        s, t = st[0, 0, :B, :q].double(), st[1, 0, :B, :q].double()
        return None, s, t, torch.zeros_like(s), torch.zeros_like(t)
    z = st[0, :, :B, :q].double().sum(0) + bias_s[:q].double()
    t = st[1, :, :B, :q].double().sum(0) + bias_t[:q].double()
    return z, z.tanh(), t, st[0, :, :B, :q].double().abs().sum(0) + bias_s[:q].double().abs(), \
        st[1, :, :B, :q].double().abs().sum(0) + bias_t[:q].double().abs()


def _head_err(S, z_mag, t_mag, s):
    """S > 1: S - 1 slab adds and the bias in slab order (S U sum|terms|), tanhf on top for the scale net; S = 1: finished values."""
    if S == 1:
        return torch.zeros_like(s), torch.zeros_like(s)
    return S * U * z_mag + TANH_U * s.abs(), S * U * t_mag


def _coupling_ref(x, st, bias_s, bias_t, S, cmap, scale, loc, c1, reverse, on_src, B, C, ld0):
    """v = couple(in); out[c] = affine(v[map[c]]) in float64 with its bound, and the log-determinant with its terms."""
    v = x[:B, :C].double().clone()
    bv = torch.zeros_like(v)
    lsum = torch.zeros(B, dtype=torch.float64)
    lmag, lerr, nterm = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.float64), 0
    q = C - c1
    if st is not None and q > 0:
        _, s, t, zm, tm = _heads64(st, bias_s, bias_t, S, B, q)
        ds, dt = _head_err(S, zm, tm, s)
        xk = v[:, c1:].clone()
        if reverse:      # (x - t) expf(-s): the difference U (|x| + |t|) + dt, expf 6 U + its argument's error, the product U
            v[:, c1:] = (xk - t) * torch.exp(-s)
            bv[:, c1:] = torch.exp(-s) * (dt + U * (xk.abs() + t.abs())) + v[:, c1:].abs() * (1.01 * ds + EXP_U + 2 * U)
        else:            # x expf(s) + t
            v[:, c1:] = xk * torch.exp(s) + t
            bv[:, c1:] = (xk * torch.exp(s)).abs() * (1.01 * ds + EXP_U + 2 * U) + dt + U * ((xk * torch.exp(s)).abs() + t.abs())
            lsum += s.sum(1)
            lmag += s.abs().sum(1)
            lerr += ds.sum(1)
            nterm += 1
    idx = torch.arange(C) if cmap is None else cmap.long()
    u, bu = v[:, idx], bv[:, idx]
    if scale is not None:
        pi = idx if on_src else torch.arange(C)
        sc, lo = scale[pi].double(), loc[pi].double()
        if reverse:      # x / sc - lo: the division 5 U, the difference U
            out = u / sc - lo
            bu = bu / sc.abs() + (DIV_U + U) * (u / sc).abs() + U * lo.abs()
        else:            # sc (x + lo)
            out = sc * (u + lo)
            bu = sc.abs() * (bu + 2 * U * (u.abs() + lo.abs()))
            lg = sc.abs().log()
            lsum += lg.sum()
            lmag += lg.abs().sum()
            lerr += LOG_U * lg.abs().sum()
            nterm += 1
    else:
        out = u
    # logdet: a thread adds nterm terms for each of its ceil(C / 256) channels, then 6 shuffle levels, 4 LDS terms and the += onto
    # the value already there
    chain = nterm * _cdiv(C, 256) + 6 + 4 + 1
    return out, bu + TINY, ld0[:B].double() + lsum, chain * U * (lmag + ld0[:B].double().abs()) + lerr + TINY


def _call_coupling(ops, S_, B, C, c1, ld_in, ld_out, Mp, reverse, on_src, S, x, st, bias_s, bias_t, cmap, scale, loc, out, logdet):
    d = S_.SeqCouplingDesc(B, C, c1, ld_in, ld_out, Mp, reverse, on_src, S)
    ops._call("vunet_seq_coupling", ctypes.byref(d), ops._p(x), ops._p(st), ops._p(bias_s), ops._p(bias_t), ops._p(cmap),
              ops._p(scale), ops._p(loc), ops._p(out), ops._p(logdet), ops._stream())


def _coupling_inputs(g, B, C, c1, S):
    Bp, Mp = _up16(B), C - c1 + 3
    x = _randn(g, B, C + 5)
    st = _randn(g, 2, max(S, 1), Bp, Mp, scale=0.5)
    if S == 1:
        st[0] = torch.tanh(st[0])                       # finished heads: s already through tanh
    bias_s, bias_t = _randn(g, Mp, scale=0.3), _randn(g, Mp, scale=0.3)
    scale = (0.5 + torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.3, -1.0, 1.0)   # some negative
    loc = _randn(g, C)
    cmap = torch.randperm(C, generator=g).to(torch.int32)
    return Mp, x, st, bias_s, bias_t, scale, loc, cmap


@pytest.mark.parametrize("C", [1, 255, 257, 1030])
@pytest.mark.parametrize("reverse", [0, 1])
def test_coupling_vs_float64(C, reverse):
    """vunet_seq_coupling over c1 in {0, C / 2, C} x heads {none, finished (S = 1), raw slabs S = 2 and 8} x map {none,
    permutation} x ActNorm {none, by destination, by source}, B drawn from {1, 17}, ld_in / ld_out > C, Mp > C - c1; forward
    with the log-determinant added onto a non-zero value (one workgroup per row: C = 1030 walks the four-channel unroll with a
    partial last group), reverse and the forward without a log-determinant on gridDim.y = ceil(C / 256) workgroups."""
    ops, S_, _ = _m()
    g = _gen(C + reverse)
    rng = random.Random(C + reverse)
    for c1 in sorted({0, C // 2, C}):
        for S in (0, 1, 2, 8):
            for with_map in (False, True):
                for aff in (None, 0, 1):
                    for with_ld in ((True, False) if not reverse and S == 2 else (True,)):
                        B = rng.choice((1, 17))
                        Mp, x, st, bias_s, bias_t, scale, loc, cmap = _coupling_inputs(g, B, C, c1, S)
                        ld0 = _randn(g, B) + 3.0
                        res = {}
                        for pad in (0.0, NAN):
                            stp = st.clone()
                            stp[:, :, B:] = pad
                            o = Outs()
                            out = o.new(B, C + 2)
                            ld = o.load(_d(ld0)) if with_ld else None
                            _call_coupling(ops, S_, B, C, c1, C + 5, C + 2, Mp, reverse, aff or 0, max(S, 1), _d(x),
                                           _d(stp) if S else None, _d(bias_s) if S > 1 else None, _d(bias_t) if S > 1 else None,
                                           _d(cmap) if with_map else None, _d(scale) if aff is not None else None,
                                           _d(loc) if aff is not None else None, out, ld)
                            o.check()
                            res[pad] = (out.cpu(), None if ld is None else ld.cpu())
                        tag = f"C {C} c1 {c1} S {S} map {with_map} affine {aff} B {B} reverse {reverse} logdet {with_ld}"
                        assert_same(res[NAN][0], res[0.0][0], f"{tag}: depends on the padding rows of the heads")
                        want, bound, wld, bld = _coupling_ref(x, st if S else None, bias_s, bias_t, max(S, 1), cmap if with_map else None,
                                                              scale if aff is not None else None, loc, c1, reverse, aff, B, C, ld0)
                        got = res[0.0][0]
                        assert torch.isnan(got[:, C:]).all(), f"{tag}: wrote beyond C"
                        assert_ulps(got[:, :C], want, bound, tag)
                        if with_ld:
                            if reverse:
                                assert_same(res[0.0][1], ld0, f"{tag}: the reverse pass touched logdet")
                            else:
                                assert_ulps(res[0.0][1], wld, bld, f"{tag} logdet")


@pytest.mark.parametrize("C,B", [(257, 17), (1030, 1)])
def test_coupling_round_trip(C, B):
    """Forward (raw slabs S = 8, a shuffle, ActNorm by destination, the log-determinant kept), then its inverse as two reverse
    launches (ActNorm by source through the inverse map; then the coupling alone): the input comes back within the reverse
    launches' own bounds plus the forward bound through the inverse's slope exp(-s) / |scale|."""
    ops, S_, _ = _m()
    g = _gen(C)
    c1, S = C // 2, 8
    Mp, x, st, bias_s, bias_t, scale, loc, cmap = _coupling_inputs(g, B, C, c1, S)
    inv = torch.empty(C, dtype=torch.int32)
    inv[cmap.long()] = torch.arange(C, dtype=torch.int32)
    o = Outs()
    y, v, back, ld = o.new(B, C), o.new(B, C), o.new(B, C), o.load(torch.zeros(B, device="cuda"))
    dev = [_d(t) for t in (x, st, bias_s, bias_t, scale, loc)]
    _call_coupling(ops, S_, B, C, c1, C + 5, C, Mp, 0, 0, S, dev[0], dev[1], dev[2], dev[3], _d(cmap), dev[4], dev[5], y, ld)
    _call_coupling(ops, S_, B, C, c1, C, C, Mp, 1, 1, 1, y, None, None, None, _d(inv), dev[4], dev[5], v, None)
    _call_coupling(ops, S_, B, C, c1, C, C, Mp, 1, 0, S, v, dev[1], dev[2], dev[3], None, None, None, back, None)
    o.check()
    _, bf, _, _ = _coupling_ref(x, st, bias_s, bias_t, S, cmap, scale, loc, c1, 0, 0, B, C, torch.zeros(B))
    y64 = y.cpu()
    _, b1, _, _ = _coupling_ref(y64, None, None, None, 1, inv, scale, loc, c1, 1, 1, B, C, torch.zeros(B))
    _, b2, _, _ = _coupling_ref(v.cpu(), st, bias_s, bias_t, S, None, None, None, c1, 1, 0, B, C, torch.zeros(B))
    _, s, _, _, _ = _heads64(st, bias_s, bias_t, S, B, C - c1)
    slope = torch.ones(B, C, dtype=torch.float64)
    slope[:, c1:] = torch.exp(-s)
    # the forward error of y[c] reaches v[map[c]] through 1 / |scale[c]|, then the input through exp(-s); launch 2's own error
    # through exp(-s); launch 3's own
    through = (bf / scale.double().abs())[:, inv.long()] + b1
    assert_ulps(back, x[:, :C].double(), slope * through + b2, "round trip")


def test_coupling_refuses_a_gather_in_place():
    ops, S_, _ = _m()
    x = torch.zeros(4, 8, device="cuda")
    cmap = torch.arange(8, dtype=torch.int32, device="cuda")
    d = S_.SeqCouplingDesc(4, 8, 4, 8, 8, 4, 0, 0, 1)
    _refused(ops, ERR_ARG, "vunet_seq_coupling", ctypes.byref(d), ops._p(x), None, None, None, ops._p(cmap), None, None, ops._p(x), None,
             ops._stream())


@pytest.mark.parametrize("C", [1, 255, 257, 1030])
def test_coupling_bwd_vs_autograd(C):
    """vunet_seq_coupling_bwd against torch.autograd of the float64 forward step out[c] = scale[c] (couple(in)[map[c]] + loc[c]),
    logdet = sum s: the loss sum(g out) + sum_b dld[b] logdet[b] with g = gbase + the n_sl slabs on columns < c1s.  gfull = g;
    gout = d / d in; dzh[0] = d / d (the scale head before its tanh), dzh[1] = d / d t.  n_sl 1 / 8 / 11 / none, gfull given / NULL
    and B 1 / 17 are drawn (seeded) over the grid c1 x heads x map x scale."""
    ops, _, T = _m()
    g = _gen(C + 5)
    rng = random.Random(C)            # 48 configurations per C: every value of the rotated options turns up
    for c1 in sorted({0, C // 2, C}):
        for S in (0, 1, 2, 8):
            for with_map in (False, True):
                for with_scale in (False, True):
                    B, n_sl, with_full = rng.choice((1, 17)), rng.choice((0, 1, 8, 11)), rng.choice((False, True))
                    Bp, q = _up16(B), C - c1
                    Mp, x, st, bias_s, bias_t, scale, loc, cmap = _coupling_inputs(g, B, C, c1, S)
                    c1s, ld_sl = c1, c1 + 3
                    gbase, gsl, dld = _randn(g, B, C + 1), _randn(g, max(n_sl, 1), Bp, ld_sl), _randn(g, B)
                    inv = torch.empty(C, dtype=torch.int32)
                    inv[cmap.long()] = torch.arange(C, dtype=torch.int32)
                    res = {}
                    for pad in (0.0, NAN):
                        stp, gslp = st.clone(), gsl.clone()
                        stp[:, :, B:] = pad
                        gslp[:, B:] = pad
                        o = Outs()
                        gout, dzh = o.new(B, C + 4), o.new(2, Bp, Mp)
                        gfull = o.new(B, C + 2) if with_full else None
                        d = T.SeqCouplingBwdDesc(B, C, c1, C + 1, C + 5, C + 4, C + 2, Mp, max(S, 1), n_sl, ld_sl, c1s)
                        ops._call("vunet_seq_coupling_bwd", ctypes.byref(d), ops._p(_d(gbase)), ops._p(_d(gslp) if n_sl else None),
                                  ops._p(_d(inv) if with_map else None), ops._p(_d(scale) if with_scale else None), ops._p(_d(x)),
                                  ops._p(_d(stp) if S else None), ops._p(_d(bias_s) if S > 1 else None),
                                  ops._p(_d(bias_t) if S > 1 else None), ops._p(_d(dld)), ops._p(gfull), ops._p(gout), ops._p(dzh),
                                  ops._stream())
                        o.check()
                        res[pad] = (gout.cpu(), dzh.cpu(), None if gfull is None else gfull.cpu())
                    tag = f"C {C} c1 {c1} S {S} map {with_map} scale {with_scale} B {B} n_sl {n_sl} gfull {with_full}"
                    assert_same(res[NAN][0], res[0.0][0], f"{tag}: gout depends on the padding rows")
                    assert_same(res[NAN][1][:, :B], res[0.0][1][:, :B], f"{tag}: dzh depends on the padding rows")
                    gout, dzh, gfull = res[0.0]
                    # ---- float64 forward, autograd
                    idx = cmap.long() if with_map else torch.arange(C)
                    sc = scale.double() if with_scale else torch.ones(C, dtype=torch.float64)
                    gt = gbase[:, :C].double().clone()
                    gmag = gt.abs()
                    if n_sl and c1s:
                        gt[:, :c1s] += gsl[:, :B, :c1s].double().sum(0)
                        gmag[:, :c1s] += gsl[:, :B, :c1s].double().abs().sum(0)
                    dg = n_sl * U * gmag                                     # n_sl adds onto gbase in slab order
                    xin = x[:, :C].double().clone().requires_grad_(True)
                    coupled = bool(S) and q > 0
                    if coupled:
                        z, s0, t0, zm, tm = _heads64(st, bias_s, bias_t, max(S, 1), B, q)
                        zl = (torch.atanh(s0) if z is None else z).clone().requires_grad_(True)     # the head before its tanh
                        tl = t0.clone().requires_grad_(True)
                        s = torch.tanh(zl)
                        v = torch.cat([xin[:, :c1], xin[:, c1:] * torch.exp(s) + tl], dim=1)
                        logdet = s.sum(1)
                    else:
                        v, logdet = xin, torch.zeros(B, dtype=torch.float64)
                    out = sc * (v[:, idx] + (loc.double() if with_scale else 0.0))
                    loss = (gt * out).sum() + (dld.double() * logdet).sum()
                    grads = torch.autograd.grad(loss, [xin] + ([zl, tl] if coupled else []))
                    # ---- bounds: dv[j] = g[c] scale[c], c = inv_map[j]: the sum's error times |scale|, and the product
                    cj = inv.long() if with_map else torch.arange(C)
                    dv = (gt * sc)[:, cj]
                    ddv = (dg * sc.abs())[:, cj] + U * dv.abs()
                    if gfull is not None:
                        assert torch.isnan(gfull[:, C:]).all(), f"{tag}: gfull beyond C"
                        assert_ulps(gfull[:, :C], gt, dg + TINY, f"{tag} gfull")
                    assert torch.isnan(gout[:, C:]).all(), f"{tag}: gout beyond C"
                    bg = ddv.clone()
                    if coupled:
                        sd = s.detach()
                        ds, _ = _head_err(max(S, 1), zm, tm, sd)
                        e = torch.exp(sd)
                        xk = x[:, c1:C].double()
                        rel_e = 1.01 * ds + EXP_U                            # expf of an argument off by ds
                        bg[:, c1:] = e * ddv[:, c1:] + (dv[:, c1:] * e).abs() * (rel_e + U)
                        a = dv[:, c1:] * xk * e                              # (g xk) e: two products
                        da = (xk * e).abs() * ddv[:, c1:] + a.abs() * (rel_e + 2 * U)
                        dsum = a + dld.double()[:, None]
                        ddsum = da + U * (a.abs() + dld.double().abs()[:, None])
                        w1 = 1 - sd * sd                                     # 1 - s s: the square U, the difference U, s off by ds
                        dw1 = 2 * sd.abs() * ds + 2 * U
                        bz = w1.abs() * ddsum + dsum.abs() * dw1 + U * (dsum * w1).abs()
                        assert_ulps(dzh[0, :B, :q], grads[1], bz + TINY, f"{tag} dzh scale head")
                        assert_ulps(dzh[1, :B, :q], grads[2], ddv[:, c1:] + TINY, f"{tag} dzh translation head")
                    assert torch.isnan(dzh[:, :B, q if coupled else 0:]).all() and torch.isnan(dzh[:, B:]).all(), f"{tag}: dzh beyond its columns"
                    assert_ulps(gout[:, :C], grads[0], bg + TINY, f"{tag} gout")


# ================================================================================================ e. the remainder
@pytest.mark.parametrize("H", [4, 64, 100, 1024])
def test_decoder_out_vs_float64(H):
    """vunet_seq_decoder_out: x' = (w_out h + b_out) + x for n in {1, 7, 8, 9, 51} (wave w of workgroup y owns rows 8 y + w and
    8 y + w + 4) and B in {1, 5}.  A lane adds ceil(H / 64) products, then 6 shuffle levels, the bias and the residual:
    (ceil(H / 64) + 1 + 6 + 2) U (sum |w h| + |b| + |x|).  The same x' goes to xs, xraw and xh[:, :n]; cs gets the old xraw; nothing
    else of xraw / xh changes."""
    ops, S, _ = _m()
    g = _gen(H)
    for n in (1, 7, 8, 9, 51):
        for B in (1, 5):
            hoff, ldraw, stride = n + 2, n + 1, n + 5
            ldx = hoff + H + 1
            xh0, w, b, xraw0 = _randn(g, B, ldx), _randn(g, n, H, scale=1 / math.sqrt(H)), _randn(g, n), _randn(g, B, ldraw)
            o = Outs()
            xh, xraw, xs, cs = o.load(_d(xh0)), o.load(_d(xraw0)), o.new(B, stride), o.new(B, stride)
            d = S.SeqLstmDesc(B, H, ldx, hoff, n, ldraw, stride)
            ops._call("vunet_seq_decoder_out", ctypes.byref(d), ops._p(xh), ops._p(_d(w)), ops._p(_d(b)), ops._p(xraw), ops._p(xs),
                      ops._p(cs), ops._stream())
            o.check()
            tag = f"H {H} n {n} B {B}"
            h = xh0[:, hoff:hoff + H].double()
            want = h @ w.double().t() + b.double() + xraw0[:, :n].double()
            mag = h.abs() @ w.double().abs().t() + b.double().abs() + xraw0[:, :n].double().abs()
            xs, cs, xh, xraw = xs.cpu(), cs.cpu(), xh.cpu(), xraw.cpu()
            assert_ulps(xs[:, :n], want, (_cdiv(H, 64) + 9) * U * mag + TINY, tag)
            assert torch.isnan(xs[:, n:]).all() and torch.isnan(cs[:, n:]).all(), f"{tag}: wrote beyond n"
            assert_same(cs[:, :n], xraw0[:, :n], f"{tag}: cs")
            assert_same(xraw[:, :n], xs[:, :n], f"{tag}: xraw")
            assert_same(xraw[:, n:], xraw0[:, n:], f"{tag}: xraw beyond n")
            assert_same(xh[:, :n], xs[:, :n], f"{tag}: xh")
            assert_same(xh[:, n:], xh0[:, n:], f"{tag}: xh beyond n")


@pytest.mark.parametrize("M,n", [(4, 1), (128, 51)])
def test_fold_input_vs_float64(M, n):
    """vunet_seq_fold_input: w_fold = w_ih w_in, bias_fold = w_ih b_in, n products added one after the other: (n + 1) U sum|terms|."""
    ops, _, _ = _m()
    g = _gen(M)
    wih, win, bin_ = _randn(g, M, n), _randn(g, n, n), _randn(g, n)
    o = Outs()
    wf, bf = o.new(M, n), o.new(M)
    ops._call("vunet_seq_fold_input", ops._p(_d(wih)), ops._p(_d(win)), ops._p(_d(bin_)), M, n, ops._p(wf), ops._p(bf),
              ops._stream())
    o.check()
    a, b, c = wih.double(), win.double(), bin_.double()
    assert_ulps(wf, a @ b, (n + 1) * U * (a.abs() @ b.abs()) + TINY, "w_fold")
    assert_ulps(bf, a @ c, (n + 1) * U * (a.abs() @ c.abs()) + TINY, "bias_fold")


@pytest.mark.parametrize("with_eps,with_b", [(True, True), (False, True), (True, False)])
def test_bottleneck_vs_float64(with_eps, with_b):
    """vunet_seq_bottleneck: mu / logstd copied out of the heads [2][Bp][Mp] bit for bit; b = eps expf(logstd) + mu: expf 6 U, the
    product U, the sum U (eps NULL: b = mu exactly)."""
    ops, _, _ = _m()
    B, H, Mp = 17, 5, 8
    Bp = _up16(B)
    g = _gen(3)
    heads, eps = _randn(g, 2, Bp, Mp), _randn(g, B, H)
    res = {}
    for pad in (0.0, NAN):
        hp = heads.clone()
        hp[:, B:] = pad
        o = Outs()
        mu, ls = o.new(B, H), o.new(B, H)
        bo = o.new(B, H) if with_b else None
        ops._call("vunet_seq_bottleneck", ops._p(_d(hp)), Mp, ops._p(_d(eps) if with_eps else None), ops._p(mu), ops._p(ls), ops._p(bo), B,
                  H, ops._stream())
        o.check()
        res[pad] = (mu.cpu(), ls.cpu(), None if bo is None else bo.cpu())
    for a, b in zip(res[0.0], res[NAN]):
        if a is not None:
            assert_same(a, b, "depends on the padding rows")
    mu, ls, bo = res[0.0]
    assert_same(mu, heads[0, :B, :H], "mu")
    assert_same(ls, heads[1, :B, :H], "logstd")
    if with_b and with_eps:
        t = eps.double() * torch.exp(ls.double())
        assert_ulps(bo, t + mu.double(), (EXP_U + 2 * U) * t.abs() + U * mu.double().abs() + TINY, "b")
    elif with_b:
        assert_same(bo, mu, "b without eps")


@pytest.mark.parametrize("with_eps,with_d", [(True, True), (False, True), (True, False)])
def test_bottleneck_bwd_vs_autograd(with_eps, with_d):
    """vunet_seq_bottleneck_bwd against autograd of b = eps exp(logstd) + mu under the loss sum(G b) + sum(dmu mu) + sum(dlogstd
    logstd), G = the n_sl slabs added in slab order + gc ((n_sl + 1) U sum|terms|)."""
    ops, _, _ = _m()
    B, H, n_sl, ld_sl, hoff = 17, 70, 3, 80, 6
    Bp = _up16(B)
    g = _gen(4)
    hsl, gc, eps, ls, dmu, dls = _randn(g, n_sl, Bp, ld_sl), _randn(g, B, H), _randn(g, B, H), _randn(g, B, H), _randn(g, B, H), _randn(g, B, H)
    res = {}
    for pad in (0.0, NAN):
        hp = hsl.clone()
        hp[:, B:] = pad
        o = Outs()
        dy = o.new(2, Bp, H)
        ops._call("vunet_seq_bottleneck_bwd", ops._p(_d(hp)), n_sl, ld_sl, hoff, ops._p(_d(gc)), ops._p(_d(eps) if with_eps else None),
                  ops._p(_d(ls)), ops._p(_d(dmu) if with_d else None), ops._p(_d(dls) if with_d else None), ops._p(dy), B, H,
                  ops._stream())
        o.check()
        res[pad] = dy.cpu()
    assert_same(res[NAN][:, :B], res[0.0][:, :B], "depends on the padding rows")
    dy = res[0.0]
    assert torch.isnan(dy[:, B:]).all()
    terms = torch.cat([hsl[:, :B, hoff:hoff + H].double(), gc.double()[None]])
    G, dG = terms.sum(0), (n_sl + 1) * U * terms.abs().sum(0)
    mu64, ls64 = torch.zeros(B, H, dtype=torch.float64, requires_grad=True), ls.double().requires_grad_(True)
    e64 = eps.double() if with_eps else torch.zeros(B, H, dtype=torch.float64)
    b = (e64 * torch.exp(ls64) + mu64) if with_eps else mu64 + 0 * ls64
    z = torch.zeros(B, H, dtype=torch.float64)
    d0, d1 = (dmu.double(), dls.double()) if with_d else (z, z)
    gm, gl = torch.autograd.grad((G * b).sum() + (d0 * mu64).sum() + (d1 * ls64).sum(), [mu64, ls64])
    assert_ulps(dy[0, :B], gm, dG + U * (d0.abs() + G.abs()) + TINY, "dy mu")
    t = G * e64 * torch.exp(ls.double())
    bt = (e64 * torch.exp(ls.double())).abs() * dG + t.abs() * (EXP_U + 2 * U)
    assert_ulps(dy[1, :B], gl, bt + U * (d1.abs() + t.abs()) + TINY, "dy logstd")


NORMLINEAR_SHAPES = [(1, 1), (5, 63), (7, 130)]


def _norm_chain(K):
    """sum of squares of a row: a lane adds ceil(K / 64) products, then 6 shuffle levels."""
    return _cdiv(K, 64) + 1 + 6


@pytest.mark.parametrize("M,K", NORMLINEAR_SHAPES)
def test_normlinear_rows_vs_float64(M, K):
    """vunet_seq_normlinear_rows: row_scale = gamma (g / sqrtf(sum v^2)): the sum c U (all terms positive), through the root
    half of it + sqrtf 6 U, the division 5 U, the product U; bias_eff = gamma bias + beta: 2 U (|gamma bias| + |beta|)."""
    ops, _, _ = _m()
    gn = _gen(K)
    v, g, bias, gamma, beta = _randn(gn, M, K), _randn(gn, M), _randn(gn, M), _randn(gn, M), _randn(gn, M)
    o = Outs()
    rs, be = o.new(M), o.new(M)
    ops._call("vunet_seq_normlinear_rows", *(ops._p(_d(t)) for t in (v, g, bias, gamma, beta)), M, K, ops._p(rs), ops._p(be),
              ops._stream())
    o.check()
    want = gamma.double() * g.double() / v.double().norm(dim=1)
    assert_ulps(rs, want, (0.5 * _norm_chain(K) * U + SQRT_U + DIV_U + U) * want.abs() + TINY, "row_scale")
    wb = gamma.double() * bias.double() + beta.double()
    assert_ulps(be, wb, 2 * U * ((gamma.double() * bias.double()).abs() + beta.double().abs()) + TINY, "bias_eff")


@pytest.mark.parametrize("M,K", NORMLINEAR_SHAPES)
def test_normlinear_bwd_vs_autograd(M, K):
    """vunet_seq_normlinear_bwd against autograd through W_eff = gamma g v / ||v||, b_eff = gamma bias + beta under the loss
    sum(dW_eff W_eff) + sum(db_eff b_eff).  c = the row reductions' chain; inv = 1 / sqrtf(nn) carries ri = c U / 2 + sqrtf + the
    division; proj = dot inv carries P = (c U + ri + U) sum|v dW| / ||v||."""
    ops, _, _ = _m()
    gn = _gen(K + 1)
    dw, db, v, g, bias, gamma = _randn(gn, M, K), _randn(gn, M), _randn(gn, M, K), _randn(gn, M), _randn(gn, M), _randn(gn, M)
    o = Outs()
    dv, dg, dbias, dgamma, dbeta = o.new(M, K), o.new(M), o.new(M), o.new(M), o.new(M)
    ops._call("vunet_seq_normlinear_bwd", *(ops._p(_d(t)) for t in (dw, db, v, g, bias, gamma)), M, K, ops._p(dv), ops._p(dg),
              ops._p(dbias), ops._p(dgamma), ops._p(dbeta), ops._stream())
    o.check()
    leaves = [t.double().requires_grad_(True) for t in (v, g, bias, gamma)]
    beta = torch.zeros(M, dtype=torch.float64, requires_grad=True)
    v64, g64, b64, ga64 = leaves
    weff = (ga64 * g64)[:, None] * v64 / v64.norm(dim=1, keepdim=True)
    loss = (dw.double() * weff).sum() + (db.double() * (ga64 * b64 + beta)).sum()
    rv, rg, rb, rga, rbeta = torch.autograd.grad(loss, leaves + [beta])
    assert_same(dbeta, rbeta.float(), "dbeta")
    c = _norm_chain(K)
    ri = 0.5 * c * U + SQRT_U + DIV_U
    vd, dwd, gd, gad, bd, dbd = v.double(), dw.double(), g.double(), gamma.double(), bias.double(), db.double()
    inv = 1 / vd.norm(dim=1)
    proj = (vd * dwd).sum(1) * inv
    P = (c * U + ri + U) * (vd * dwd).abs().sum(1) * inv
    assert_ulps(dg, rg, gad.abs() * P + U * (gad * proj).abs() + TINY, "dg")
    assert_ulps(dgamma, rga, gd.abs() * P + 2 * U * ((gd * proj).abs() + (bd * dbd).abs()) + TINY, "dgamma")
    assert_ulps(dbias, rb, U * rb.abs() + TINY, "dbias")
    # dv = rs (dW - proj inv v), rs = gamma g inv: the second term carries P and two factors of inv, the difference U, rs ri + 2 U
    t2 = (proj * inv)[:, None] * vd
    dt2 = (inv[:, None] * vd).abs() * P[:, None] + t2.abs() * (ri + 2 * U)
    rs = (gad * gd * inv).abs()[:, None]
    assert_ulps(dv, rv, rs * (dt2 + U * (dwd.abs() + t2.abs())) + rs * (dwd.abs() + t2.abs()) * (ri + 3 * U) + TINY, "dv")


@pytest.mark.parametrize("B", [2, 64])
@pytest.mark.parametrize("C", [1, 300])
def test_actnorm_init_vs_float64(B, C):
    """vunet_seq_actnorm_init: loc = -mean, scale = 1 / (std + 1e-6), unbiased std over the B rows, one thread per channel adding
    the rows one after the other.  mean: (B + 1) U sum|x| / B; d = x - mean: the mean's error + U |d|; the sum of squares: 2 |d|
    times d's error + (B + 2) U sum d^2; then the division by B - 1 (5 U), the root, the sum with 1e-6f and the reciprocal.  The
    last channel is constant: variance exactly 0, scale = 1 / 1e-6f."""
    ops, _, _ = _m()
    g = _gen(B + C)
    ld = C + 3
    x = _randn(g, B, ld) + 0.5
    x[:, C - 1] = 0.5
    o = Outs()
    loc, scale = o.new(C), o.new(C)
    ops._call("vunet_seq_actnorm_init", ops._p(_d(x)), ld, B, C, ops._p(loc), ops._p(scale), ops._stream())
    o.check()
    xd = x[:, :C].double()
    m = xd.mean(0)
    dm = (B + 1) * U * xd.abs().sum(0) / B
    dm[C - 1] = 0.0                                     # B halves add up exactly and divide exactly
    assert_ulps(loc, -m, dm + TINY, "loc")
    d = xd - m
    dd = dm + U * d.abs()
    dd[:, C - 1] = 0.0
    ss = (d * d).sum(0)
    dss = (2 * d.abs() * dd).sum(0) + (B + 2) * U * ss
    var = ss / (B - 1)
    dvar = dss / (B - 1) + DIV_U * var
    std = var.sqrt()
    dstd = torch.where(std > 0, dvar / (2 * std.clamp_min(TINY)), dvar.sqrt()) + SQRT_U * std
    eps = float(torch.tensor(1e-6, dtype=torch.float32))
    want = 1 / (std + eps)
    assert_ulps(scale, want, want * want * (dstd + U * (std + eps)) + DIV_U * want + TINY, "scale")


@pytest.mark.parametrize("step", [0, 999])
def test_adam_tick_vs_float64(step):
    """vunet_seq_adam_tick: ++step; resolved = {lr / (1 - b1^t), 1 / sqrt(1 - b2^t)} formed in double and rounded to fp32 once:
    U |ref| (+ 1e-13 relative for the double pow / sqrt).  resolved NULL: the step alone."""
    ops, _, _ = _m()
    lr, b1, b2 = 1e-3 / 3, 0.5, 0.9
    o = Outs()
    st = o.load(torch.tensor([step], dtype=torch.int64, device="cuda"))
    res = o.new(2)
    lrd = torch.tensor([lr], dtype=torch.float64, device="cuda")
    ops._call("vunet_seq_adam_tick", ops._p(st), ops._p(lrd), b1, b2, ops._p(res), ops._stream())
    o.check()
    t = step + 1
    assert int(st.item()) == t
    want = torch.tensor([lr / (1 - _f32(b1) ** t), 1 / math.sqrt(1 - _f32(b2) ** t)], dtype=torch.float64)
    assert_ulps(res, want, (U + 1e-13) * want.abs(), "resolved")
    ops._call("vunet_seq_adam_tick", ops._p(st), None, b1, b2, None, ops._stream())
    o.check()
    assert int(st.item()) == t + 1


@pytest.mark.parametrize("C", [1, 65, 130])
@pytest.mark.parametrize("B", [1, 6, 64])
def test_actnorm_bwd_vs_autograd(C, B):
    """vunet_seq_actnorm_bwd, two layers in one table, against autograd of out = scale (u + loc), logdet = sum_c log|scale| on
    every row, loss = sum(gfull out) + sum_b dld[b] logdet.  Row group rg adds rows rg, rg + 4, ... (ceil(B / 4) terms), the four
    groups meet in LDS (3 adds): d loc = scale s0 with (ceil(B / 4) + 3) U sum|g| on s0; d scale = (s1 + sum dld) / scale with one
    more for the product in s1, B U sum|dld| on the serial sum of dld, the sum and the division.  Without hp: the gradients;
    with hp: one Adam step of scale / loc from the constants vunet_seq_adam_tick resolved, against float64 Adam."""
    ops, _, T = _m()
    g = _gen(C * 100 + B)
    ld = C + 2
    lr, b1, b2, eps, wd = 1e-3 / 3, 0.5, 0.9, 1e-8, 1e-4
    layers = []
    for _ in range(2):
        layers.append(dict(scale=(0.5 + torch.rand(C, generator=g)) * torch.where(torch.rand(C, generator=g) < 0.3, -1.0, 1.0),
                           loc=_randn(g, C), gfull=_randn(g, B, ld), out=_randn(g, B, ld),
                           sm=_randn(g, C, scale=1e-2), sv=torch.rand(C, generator=g) * 1e-2, lm=_randn(g, C, scale=1e-2),
                           lv=torch.rand(C, generator=g) * 1e-2))
    dld = _randn(g, B)
    chain = _cdiv(B, 4) + 3
    for adam in (False, True):
        o = Outs()
        dev, entries = [], []
        for L in layers:
            d = {k: o.load(_d(L[k])) for k in ("scale", "loc", "sm", "sv", "lm", "lv")}
            d["gs"], d["gl"] = o.new(C), o.new(C)
            d["gfull"], d["out"] = _d(L["gfull"]), _d(L["out"])
            dev.append(d)
            entries.append(T.SeqActnormLayer(*(d[k].data_ptr() for k in ("scale", "loc", "sm", "sv", "lm", "lv", "gs", "gl", "gfull", "out")),
                                             ld, 0))
        tab = T._table(entries, "cuda")
        hp, keep = _adam_hp(T, lr, 6, b1, b2, eps, wd)
        if adam:
            ops._call("vunet_seq_adam_tick", ops._p(keep[1]), ops._p(keep[0]), b1, b2, ops._p(keep[2]), ops._stream())
        ops._call("vunet_seq_actnorm_bwd", ops._p(tab), 2, C, B, ops._p(_d(dld)), ctypes.byref(hp) if adam else None, ops._stream())
        o.check()
        for li, (L, d) in enumerate(zip(layers, dev)):
            sc = L["scale"].double().requires_grad_(True)
            lo = L["loc"].double().requires_grad_(True)
            gf, out = L["gfull"][:, :C].double(), L["out"][:, :C].double()
            u = out / L["scale"].double() - L["loc"].double()
            loss = (gf * (sc * (u + lo))).sum() + dld.double().sum() * sc.abs().log().sum()
            rs, rl = torch.autograd.grad(loss, [sc, lo])
            s1, sld = (gf * out).sum(0), dld.double().sum()
            a = L["scale"].double().abs()
            ds1 = (chain + 1) * U * (gf * out).abs().sum(0) + B * U * dld.double().abs().sum() + U * (s1.abs() + abs(sld))
            brs = ds1 / a + DIV_U * rs.abs() + TINY
            brl = a * chain * U * gf.abs().sum(0) + U * rl.abs() + TINY
            tag = f"layer {li} C {C} B {B}"
            if not adam:
                assert_ulps(d["gs"], rs, brs, f"{tag} d scale")
                assert_ulps(d["gl"], rl, brl, f"{tag} d loc")
                for k in ("scale", "loc", "sm", "sv", "lm", "lv"):
                    assert_same(d[k], L[k], f"{tag}: write mode changed {k}")
                continue
            assert int(keep[1].item()) == 7
            step_size, k2 = (float(t) for t in keep[2].cpu().double())
            for (pk, mk, vk, gr, bgr) in (("scale", "sm", "sv", rs, brs), ("loc", "lm", "lv", rl, brl)):
                (p2, dp), (m2, dm), (v2, dv) = _adam64(L[pk], gr, L[mk], L[vk], step_size, k2, b1, b2, eps, wd, bgr)
                assert_ulps(d[mk], m2, dm, f"{tag} Adam {mk}")
                assert_ulps(d[vk], v2, dv, f"{tag} Adam {vk}")
                assert_ulps(d[pk], p2, dp, f"{tag} Adam {pk}")
            assert torch.isnan(d["gs"]).all() and torch.isnan(d["gl"]).all(), f"{tag}: Adam mode wrote gradients"


@pytest.mark.parametrize("B", [1, 17, 64])
@pytest.mark.parametrize("C,pad_ld", [(8, 0), (300, 0), (51, 0), (300, 1)])
def test_flow_loss_vs_float64(B, C, pad_ld):
    """vunet_seq_flow_loss: the 16-byte path (C % 4 == 0, leading dimensions % 4 == 0) and the scalar one (C = 51; ld = C + 1);
    noise / dz / dld given and NULL.  A row's sum of squares: at most ceil(C / 64) serial terms per lane (the vector form adds a
    tree of four per step), 6 shuffle levels, then 6 more over the rows, the products, 0.5 (exact) and 1 / B (two roundings):
    (ceil(C / 64) + 16) U nll, all terms positive.  nlogdet: 6 levels + 3.  dz = z (1 / B): 2 U; rows B .. Bp of dz and dld are
    zeroed."""
    ops, _, _ = _m()
    Bp, ldz, ld_dz = _up16(B), C + pad_ld, C + 4 * (1 - pad_ld) + pad_ld
    g = _gen(B + C)
    z, logdet, noise = _randn(g, B, ldz), _randn(g, B) * 3, _randn(g, B, C)
    zz, ee, ld64 = z[:, :C].double(), noise.double(), logdet.double()
    nll, ref_nll, nld = 0.5 * (zz * zz).sum() / B, 0.5 * (ee * ee).sum() / B, -ld64.sum() / B
    c = _cdiv(C, 64) + 16
    for with_noise, with_dz, with_dld in ((True, True, True), (False, True, True), (True, False, False), (True, True, False)):
        o = Outs()
        scal = o.new(4)
        dz = o.new(Bp, ld_dz) if with_dz else None
        dld = o.new(Bp) if with_dld else None
        ops._call("vunet_seq_flow_loss", ops._p(_d(z)), ldz, ops._p(_d(logdet)), ops._p(_d(noise) if with_noise else None), B, C,
                  ops._p(scal), ops._p(dz), ld_dz, ops._p(dld), ops._stream())
        o.check()
        tag = f"B {B} C {C} ld {ldz} noise {with_noise} dz {with_dz} dld {with_dld}"
        bn, bl = c * U * nll, 9 * U * ld64.abs().sum() / B
        want = torch.stack([nll + nld, ref_nll if with_noise else torch.zeros((), dtype=torch.float64), nld, nll])
        bound = torch.stack([bn + bl + U * (nll + nld.abs()), c * U * ref_nll, bl, bn]) + TINY
        assert_ulps(scal, want, bound, f"{tag} scalars")
        if with_dz:
            dz = dz.cpu()
            assert_ulps(dz[:B, :C], zz / B, 2 * U * zz.abs() / B + TINY, f"{tag} dz")
            assert_same(dz[B:, :C], torch.zeros(Bp - B, C), f"{tag}: dz rows B .. Bp")
            assert torch.isnan(dz[:, C:]).all(), f"{tag}: dz beyond C"
        if with_dld:
            dld = dld.cpu()
            assert_ulps(dld[:B], torch.full((B,), -1.0 / B, dtype=torch.float64), U / B, f"{tag} dld")
            assert_same(dld[B:], torch.zeros(Bp - B), f"{tag}: dld rows B .. Bp")


@pytest.mark.parametrize("B,T,n,H", [(1, 1, 1, 1), (5, 3, 51, 300), (64, 70, 51, 64)])
@pytest.mark.parametrize("entry", ["vunet_seq_vae_loss", "vunet_seq_vae_loss_w"])
def test_vae_loss_vs_float64(entry, B, T, n, H):
    """vunet_seq_vae_loss and vunet_seq_vae_loss_w (the KL weight from its own device scalar while gamma still advances).
    A step's squared error: ceil(B n / 256) serial terms per thread + the product + 6 shuffle levels + 3 LDS adds (chain cp);
    recon adds ceil(T / 64) + 6 more over the steps and a division.  A row's KL: every term -l + 0.5 (expf(l)^2 + m^2) carries
    16 U (|l| + 0.5 (e^2l + m^2)) (expf twice, the square, the sums), then ceil(H / 256) + 9, the - 0.5 H, ceil(B / 64) + 6 over
    the rows and the division.  gamma: unchanged with gamma_step = 0, advanced and clamped at 0 otherwise.  T = 70 > 64 lanes."""
    ops, _, _ = _m()
    g = _gen(B + T + H)
    xs, tg, mu, ls = _randn(g, B, T, n), _randn(g, B, T, n), _randn(g, B, H), _randn(g, B, H, scale=0.5)
    rw, wkl = 1.5, 0.75
    e = (xs - tg).double()                                          # (the fp32 difference: U |e|, inside the chains' room)
    part = (e * e).sum(dim=(0, 2))
    cp = _cdiv(B * n, 256) + 1 + 9 + 2                              # + the difference's rounding, squared: 2 U
    recon, per_seq = part.sum() / (B * T * n), part / (B * n)
    drecon = (cp + _cdiv(T, 64) + 6 + DIV_U / U) * U * recon
    m64, l64 = mu.double(), ls.double()
    a = l64.abs() + 0.5 * (torch.exp(2 * l64) + m64 * m64)
    rows = (-l64 + 0.5 * (torch.exp(2 * l64) + m64 * m64)).sum(1)
    kl = (rows - 0.5 * H).sum() / B
    dkl = (16 + _cdiv(H, 256) + 9 + 1 + _cdiv(B, 64) + 6 + DIV_U / U) * U * (a.sum() + 0.5 * H * B) / B
    cm = (_cdiv(H, 256) + 9 + _cdiv(B, 64) + 6 + DIV_U / U) * U / (B * H)
    for gamma0, imax, gstep, grads in ((0.25, 5.0, 0.0, True), (0.25, 1e4, 1e-3, True), (0.25, -1e4, 1e-3, False)):
        o = Outs()
        gamma = o.load(torch.tensor([gamma0], device="cuda"))
        scal, per, part_d = o.new(6), o.new(T), o.new(T + 3 * B)
        dxs, dmu, dls = (o.new(B, T, n), o.new(B, H), o.new(B, H)) if grads else (None, None, None)
        args = [ops._p(_d(t)) for t in (xs, tg, mu, ls)] + [B, T, n, H, rw]
        w = gamma0
        if entry == "vunet_seq_vae_loss_w":
            w = wkl
            args.append(ops._p(_d(torch.tensor([wkl]))))
        args += [ops._p(gamma), ops._p(_d(torch.tensor([imax]))), gstep, ops._p(part_d), ops._p(scal), ops._p(per), ops._p(dxs),
                 ops._p(dmu), ops._p(dls)]
        ops._call(entry, *args, ops._stream())
        o.check()
        tag = f"{entry} B {B} T {T} n {n} H {H} gamma_step {gstep} imax {imax}"
        w = _f32(w)
        want = torch.stack([rw * recon + w * kl, recon, kl, torch.tensor(w, dtype=torch.float64), m64.mean(), l64.mean()])
        bound = torch.stack([rw * drecon + w * dkl + 3 * U * (rw * recon + w * kl.abs()), drecon, dkl, torch.zeros((), dtype=torch.float64),
                             cm * m64.abs().sum(), cm * l64.abs().sum()]) + TINY
        assert_ulps(scal, want, bound, f"{tag} scalars")
        assert_ulps(per, per_seq, (cp + DIV_U / U) * U * per_seq + TINY, f"{tag} per_seq")
        g0 = _f32(gamma0)
        if gstep == 0.0:
            assert_same(gamma, torch.tensor([g0]), f"{tag}: gamma moved")
        else:
            gs32, im32 = _f32(gstep), _f32(imax)
            raw = g0 - gs32 * (im32 - kl)
            braw = gs32 * (dkl + U * (abs(im32) + kl.abs())) + U * abs(gs32 * (im32 - kl)) + U * (g0 + abs(gs32 * (im32 - kl))) + TINY
            assert_ulps(gamma, raw.clamp_min(0.0).reshape(1), braw.reshape(1), f"{tag} gamma")
            assert (float(raw) < 0) == (imax > 0), "the two cases: one clamps, one does not"
        if grads:
            # k = rw 2 / (B T n) in fp32 (three roundings), the difference, the product: 6 U
            ref = rw * 2.0 / (B * T * n) * e
            assert_ulps(dxs, ref, 6 * U * ref.abs() + TINY, f"{tag} dxs")
            assert_ulps(dmu, w / B * m64, 3 * U * (w / B * m64).abs() + TINY, f"{tag} dmu")
            e2 = torch.exp(2 * l64)
            assert_ulps(dls, w / B * (e2 - 1), abs(w / B) * ((2 * EXP_U + U) * e2 + U * (e2 - 1).abs()) + 2 * U * (w / B * (e2 - 1)).abs() + TINY,
                        f"{tag} dlogstd")


@pytest.mark.parametrize("T,J", [(1, 1), (257, 1), (7, 17)])
@pytest.mark.parametrize("f32_math", [0, 1])
def test_pose_project_vs_float64(T, J, f32_math):
    """vunet_seq_pose_project: un-normalise (dims_to_use with gaps: the others hold 0 std + mean), [R | t], the pinhole projection
    and the rescale, in double on the device and rounded to fp32 once: U |ref| (+ 1e-12 for the double arithmetic).  f32_math: the
    un-normalisation is fp32 (a product and a sum, or one fused: 2 U (|v std| + |mean|) on p), carried through the projection
    linearly: dc = |R| dp, d(X / Z) = dX / |Z| + |X| dZ / Z^2."""
    ops, _, _ = _m()
    g = _gen(T * J + f32_math)
    D = 3 * J + 2
    dims = torch.tensor([d for d in range(3 * J) if d % 5 != 1], dtype=torch.int32)
    n_use = dims.numel()
    x = _randn(g, T, n_use)
    mean, std = torch.randn(D, generator=g, dtype=torch.float64), torch.rand(D, generator=g, dtype=torch.float64) + 0.5
    R = torch.linalg.qr(torch.randn(3, 3, generator=g, dtype=torch.float64))[0]
    t = torch.tensor([0.1, -0.2, 12.0], dtype=torch.float64)       # the subject well in front of the camera
    cam = torch.cat([torch.cat([R, t[:, None]], dim=1).reshape(-1), torch.tensor([1100.0, 512.3, 1090.0, 500.9, 0.25, 0.125], dtype=torch.float64)])
    o = Outs()
    kps = o.new(T, J, 2)
    ops._call("vunet_seq_pose_project", ops._p(_d(x)), n_use, ops._p(_d(dims)), ops._p(_d(mean)), ops._p(_d(std)), D, f32_math,
              ops._p(_d(cam)), ops._p(kps), T, J, ops._stream())
    o.check()
    full = torch.zeros(T, 3 * J, dtype=torch.float64)
    full[:, dims.long()] = x.double()
    if f32_math:
        s32, m32 = std[:3 * J].float().double(), mean[:3 * J].float().double()
        p = full * s32 + m32
        dp = 2 * U * ((full * s32).abs() + m32.abs())
    else:
        p = full * std[:3 * J] + mean[:3 * J]
        dp = torch.zeros_like(p)
    p, dp = p.view(T, J, 3), dp.view(T, J, 3)
    c = p @ R.t() + t
    dc = dp @ R.abs().t()
    u = torch.stack([c[..., 0] / c[..., 2] * cam[12] + cam[13], c[..., 1] / c[..., 2] * cam[14] + cam[15]], dim=-1) * cam[16:18]
    z = c[..., 2].abs()
    du = torch.stack([(dc[..., 0] / z + c[..., 0].abs() * dc[..., 2] / (z * z)) * cam[12],
                      (dc[..., 1] / z + c[..., 1].abs() * dc[..., 2] / (z * z)) * cam[14]], dim=-1) * cam[16:18]
    assert_ulps(kps, u, (U + 1e-12) * u.abs() + du + TINY, f"T {T} J {J} f32 {f32_math}")


# ================================================================================================ the backward pass's other kernels
@pytest.mark.parametrize("nets,S,Bp,K", [(1, 1, 16, 4), (2, 4, 48, 68), (2, 11, 64, 256)])
def test_dz_finish_vs_float64(nets, S, Bp, K):
    """vunet_seq_dz_finish: dz = (the S slabs added in slab order: S U sum|terms|) * (y > 0 ? 1 : slope), one more product; S = 11
    runs past the eight slabs held in registers; all Bp rows."""
    ops, _, _ = _m()
    g = _gen(S + K)
    raw, y = _randn(g, nets, S, Bp, K), _randn(g, nets, Bp, K)
    y[0, 0, 0] = 0.0                                                # y == 0 takes the slope
    o = Outs()
    dz = o.new(nets, Bp, K)
    ops._call("vunet_seq_dz_finish", ops._p(_d(raw)), ops._p(_d(y)), ops._p(dz), nets, S, Bp, K, SLOPE, ops._stream())
    o.check()
    f = torch.where(y.double() > 0, 1.0, SLOPE)
    assert_ulps(dz, raw.double().sum(1) * f, (S + 1) * U * raw.double().abs().sum(1) * f + TINY, "dz_finish")


@pytest.mark.parametrize("B,M,K,nets,S", [(17, 64, 64, 1, 2), (64, 256, 128, 2, 4), (33, 1024, 192, 2, 9), (16, 4096, 64, 1, 1)])
def test_dx_finish_bit_equal_to_dx_then_dz_finish(B, M, K, nets, S):
    """vunet_seq_dx_finish against the two launches it replaces -- vunet_seq_dx (every raw slab against the float64 product over
    its own rows of W, as tests/test_hip_seq_train.py does at the training shapes) and vunet_seq_dz_finish (above): the raw
    slabs and dz_prev bit for bit, the arrival counters back at zero, twice in a row; padding rows of dz at 0 and at NaN leave
    rows < B alone."""
    ops, _, T = _m()
    g = _gen(B + M + K)
    Bp = _up16(B)
    w = [_randn(g, M, K, scale=1 / math.sqrt(M)).cuda() for _ in range(nets)]
    dz0, y = _randn(g, nets, Bp, M), _randn(g, nets, Bp, K).cuda()
    d = T.SeqDxDesc(B, M, K, nets, S, 0)
    res = {}
    for pad in (0.0, NAN):
        dz = dz0.clone()
        dz[:, B:] = pad
        dz = _d(dz)
        o = Outs()
        raw_a, raw_b, prev_a, prev_b = o.new(nets, S, Bp, K), o.new(nets, S, Bp, K), o.new(nets, Bp, K), o.new(nets, Bp, K)
        cnt = o.load(torch.zeros(nets * (K // 64), dtype=torch.int32, device="cuda"))
        ops._call("vunet_seq_dx", ctypes.byref(d), ops._p(w[0]), ops._p(w[1] if nets > 1 else None), ops._p(dz), ops._p(raw_a), ops._stream())
        ops._call("vunet_seq_dz_finish", ops._p(raw_a), ops._p(y), ops._p(prev_a), nets, S, Bp, K, SLOPE, ops._stream())
        for _ in range(2):
            ops._call("vunet_seq_dx_finish", ctypes.byref(d), ops._p(w[0]), ops._p(w[1] if nets > 1 else None), ops._p(dz), ops._p(raw_b),
                      ops._p(y), ops._p(prev_b), ops._p(cnt), SLOPE, ops._stream())
            o.check()
            assert int(cnt.abs().sum()) == 0, "arrival counters not back at zero"
            assert_same(raw_b[:, :, :B], raw_a[:, :, :B], f"raw slabs, padding {pad}")
            assert_same(prev_b[:, :B], prev_a[:, :B], f"dz_prev, padding {pad}")
        res[pad] = prev_b.cpu()
        if pad == 0.0:
            assert not torch.isnan(res[pad]).any(), "unwritten dz_prev"
            want = torch.stack([dz0[n, :B].double() @ w[n].cpu().double() for n in range(nets)])
            mag = torch.stack([dz0[n, :B].double().abs() @ w[n].cpu().double().abs() for n in range(nets)])
            f = torch.where(y.cpu()[:, :B].double() > 0, 1.0, SLOPE)
            # a slab's chain: M / S rows (+ the waves' partials); the S slabs; the product
            assert_ulps(res[pad][:, :B], want * f, (M // S + 16 + S + 1) * U * mag * f + TINY, "dz_prev vs float64")
            G = M // 16                                             # slab s: W's 16-row groups [s G / S, (s + 1) G / S)
            for n in range(nets):
                for s_ in range(S):
                    r = slice(16 * (s_ * G // S), 16 * ((s_ + 1) * G // S))
                    dzs, ws = dz0[n, :B, r].double(), w[n].cpu()[r].double()
                    assert_ulps(raw_a[n, s_, :B], dzs @ ws, (r.stop - r.start + 16) * U * (dzs.abs() @ ws.abs()) + TINY, f"vunet_seq_dx slab {s_}")
    assert_same(res[NAN][:, :B], res[0.0][:, :B], "rows < B depend on the padding rows")


@pytest.mark.parametrize("B", [7, 40])
def test_dwx_write_mode_vs_float64(B):
    """vunet_seq_dwx without Adam: dW = dZ^T X per 64 x 64 tile (the reduction runs over the Bp rows: (Bp + 1) U sum|terms|; the
    columns >= kv forced to zero), the bias gradient (Bp serial terms), and dx_raw[tm] = dZ[:, rows of tile tm] . W[those rows]
    (128-row tiles, the last one short: (rows + 1) U sum|terms|).  Rows >= B of dZ are zero by the kernel's contract."""
    ops, _, T = _m()
    g = _gen(B)
    Bp, M, K, ldx, kv, nch = _up16(B), 192, 128, 136, 100, 2
    dz, x = torch.zeros(Bp, M), torch.zeros(Bp, ldx)
    dz[:B], x[:B] = _randn(g, B, M), _randn(g, B, ldx)
    w, bias = _randn(g, M, K), _randn(g, M)
    tiles_m = _cdiv(M, 64 * nch)
    o = Outs()
    gw, gb, dxr = o.new(M, K), o.new(M), o.new(tiles_m, Bp, K)
    wd, bd, dzd, xd = _d(w), _d(bias), _d(dz), _d(x)
    ent = T.SeqDwLayer(wd.data_ptr(), None, None, gw.data_ptr(), bd.data_ptr(), None, None, gb.data_ptr(), dzd.data_ptr(), xd.data_ptr(),
                       M, K, M, ldx, 0, K // 64, kv, nch, 0, 0, dxr.data_ptr())
    tab = T._table([ent], "cuda")
    ops._call("vunet_seq_dwx", ops._p(tab), 1, 0, tiles_m * (K // 64), B, None, ops._stream())
    o.check()
    d64, x64, w64 = dz.double(), x[:, :K].double(), w.double()
    want, mag = d64.t() @ x64, d64.abs().t() @ x64.abs()
    want[:, kv:], mag[:, kv:] = 0, 0
    assert_ulps(gw, want, (Bp + 1) * U * mag + TINY, "dW")
    assert_ulps(gb, d64.sum(0), Bp * U * d64.abs().sum(0) + TINY, "d bias")
    assert_same(wd, w, "write mode changed W")
    for tm in range(tiles_m):
        r = slice(128 * tm, min(128 * (tm + 1), M))
        assert_ulps(dxr[tm], d64[:, r] @ w64[r], (r.stop - r.start + 1) * U * (d64[:, r].abs() @ w64[r].abs()) + TINY, f"dx_raw slab {tm}")


def test_dwx_adam_mode_vs_float64():
    """vunet_seq_dwx with Adam: W, exp_avg, exp_avg_sq and the bias triple after one update against float64 Adam (``_adam64``,
    the gradient's bound as in the write mode) from the constants vunet_seq_adam_tick resolved; dx_raw is formed from the
    weights as they were BEFORE the update; the padding columns (>= kv) see a zero gradient."""
    ops, _, T = _m()
    B = 40
    g = _gen(B + 1)
    Bp, M, K, ldx, kv, nch = _up16(B), 192, 128, 136, 100, 2
    lr, b1, b2, eps, wd_ = 1e-3 / 3, 0.5, 0.9, 1e-8, 1e-4
    dz, x = torch.zeros(Bp, M), torch.zeros(Bp, ldx)
    dz[:B], x[:B] = _randn(g, B, M), _randn(g, B, ldx)
    st0 = dict(w=_randn(g, M, K), m=_randn(g, M, K, scale=1e-2), v=torch.rand(M, K, generator=g) * 1e-2,
               bias=_randn(g, M), bm=_randn(g, M, scale=1e-2), bv=torch.rand(M, generator=g) * 1e-2)
    tiles_m = _cdiv(M, 64 * nch)
    o = Outs()
    dev = {k: o.load(_d(t)) for k, t in st0.items()}
    dxr = o.new(tiles_m, Bp, K)
    dzd, xd = _d(dz), _d(x)
    ent = T.SeqDwLayer(dev["w"].data_ptr(), dev["m"].data_ptr(), dev["v"].data_ptr(), None, dev["bias"].data_ptr(), dev["bm"].data_ptr(),
                       dev["bv"].data_ptr(), None, dzd.data_ptr(), xd.data_ptr(), M, K, M, ldx, 0, K // 64, kv, nch, 0, 0, dxr.data_ptr())
    tab = T._table([ent], "cuda")
    hp, keep = _adam_hp(T, lr, 2, b1, b2, eps, wd_)
    ops._call("vunet_seq_adam_tick", ops._p(keep[1]), ops._p(keep[0]), b1, b2, ops._p(keep[2]), ops._stream())
    ops._call("vunet_seq_dwx", ops._p(tab), 1, 0, tiles_m * (K // 64), B, ctypes.byref(hp), ops._stream())
    o.check()
    step_size, k2 = (float(t) for t in keep[2].cpu().double())
    d64, x64, w64 = dz.double(), x[:, :K].double(), st0["w"].double()
    gw, mag = d64.t() @ x64, d64.abs().t() @ x64.abs()
    gw[:, kv:], mag[:, kv:] = 0, 0
    for (pk, mk, vk, gr, bgr) in (("w", "m", "v", gw, (Bp + 1) * U * mag), ("bias", "bm", "bv", d64.sum(0), Bp * U * d64.abs().sum(0))):
        (p2, dp), (m2, dm), (v2, dv) = _adam64(st0[pk], gr, st0[mk], st0[vk], step_size, k2, b1, b2, eps, wd_, bgr)
        assert_ulps(dev[mk], m2, dm, f"Adam {mk}")
        assert_ulps(dev[vk], v2, dv, f"Adam {vk}")
        assert_ulps(dev[pk], p2, dp, f"Adam {pk}")
    for tm in range(tiles_m):
        r = slice(128 * tm, min(128 * (tm + 1), M))
        assert_ulps(dxr[tm], d64[:, r] @ w64[r], (r.stop - r.start + 1) * U * (d64[:, r].abs() @ w64[r].abs()) + TINY, f"dx_raw slab {tm}")


CELL_CASES = [(5, 32, 0, 3, 0), (17, 300, 51, 5, 0), (3, 64, 51, 17, 0), (4, 300, 7, 0, 1), (4, 40, 0, 2, 2), (64, 20, 51, 8, 0)]


@pytest.mark.parametrize("B,H,n,n_sl,first", CELL_CASES)
def test_cell_bwd_vs_autograd(B, H, n, n_sl, first):
    """vunet_seq_cell_bwd against autograd of one LSTM step in float64, c' = f c + i g, h = o tanh(c'), the gates functions of
    their pre-activations (the leaves; the kernel takes the kept activations), and for the decoder (n > 0) x' = W_out h + x:
    loss = sum(dh_later h) + sum(gc c') + sum(gx x'), dh_later = the n_sl slabs of the later step at hoff_sl, gx = gl + gx_next +
    the slabs' first n columns.  dgates = d / d pre-activations, gc <- d / d c.  n_sl = 17 runs past the 16 slabs in registers;
    first & 1: no later step; first & 2: gc taken as 0.  Chains: gx n_sl + 2; dh the slabs (n_sl) + the n products one after the
    other (n + 1) + 1."""
    ops, _, T = _m()
    g = _gen(B + H + n)
    Bp, hoff_sl = _up16(B), 64
    ld_sl = hoff_sl + H + 1
    later = not (first & 1)
    pre = _randn(g, B, H, 4)
    act64 = torch.stack([pre[..., 0].double().sigmoid(), pre[..., 1].double().sigmoid(), pre[..., 2].double().tanh(),
                         pre[..., 3].double().sigmoid()], dim=-1)
    gates = act64.float()                                        # what the forward kernel kept: the fp32 activations
    cp = _randn(g, B, H)
    a64 = gates.double()
    cn = (a64[..., 1] * cp.double() + a64[..., 0] * a64[..., 2]).float()
    hsl = _randn(g, max(n_sl, 1), Bp, ld_sl)
    w_out = _randn(g, max(n, 1), H, scale=1 / math.sqrt(H))
    gl, gxn, gc0 = _randn(g, B, n + 2), _randn(g, B, 64), _randn(g, B, H)
    res = {}
    for pad in (0.0, NAN):
        hp = hsl.clone()
        hp[:, B:] = pad
        o = Outs()
        gc, dgates = o.load(_d(gc0)), o.new(B, H, 4)
        gxo = o.new(B, 64) if n else None
        d = T.SeqCellBwdDesc(B, H, n, n_sl, ld_sl, hoff_sl, first, 0, n + 2)
        ops._call("vunet_seq_cell_bwd", ctypes.byref(d), ops._p(_d(hp) if n_sl else None), ops._p(_d(w_out) if n else None),
                  ops._p(_d(gl) if n else None), ops._p(_d(gxn) if n else None), ops._p(gxo), ops._p(_d(gates)), ops._p(_d(cp)),
                  ops._p(_d(cn)), ops._p(gc), ops._p(dgates), ops._stream())
        o.check()
        res[pad] = (gc.cpu(), dgates.cpu(), None if gxo is None else gxo.cpu())
    for a, b in zip(res[0.0], res[NAN]):
        if a is not None:
            assert_same(a, b, "depends on the padding rows of the slabs")
    gc, dgates, gxo = res[0.0]
    # ---- float64: leaves = the pre-activations that give exactly the kept fp32 activations, and c
    z = torch.stack([torch.logit(a64[..., 0]), torch.logit(a64[..., 1]), torch.atanh(a64[..., 2]), torch.logit(a64[..., 3])], dim=-1)
    z = z.clone().requires_grad_(True)
    c = cp.double().requires_grad_(True)
    i_, f_, g_, o_ = z[..., 0].sigmoid(), z[..., 1].sigmoid(), z[..., 2].tanh(), z[..., 3].sigmoid()
    c2 = f_ * c + i_ * g_
    h = o_ * torch.tanh(c2)
    use_sl = later and n_sl > 0
    sl = hsl[:, :B].double() if use_sl else torch.zeros(1, B, ld_sl, dtype=torch.float64)
    dh_later = sl[:, :, hoff_sl:hoff_sl + H].sum(0)
    dh_mag = sl[:, :, hoff_sl:hoff_sl + H].abs().sum(0)
    gc_in = torch.zeros(B, H, dtype=torch.float64) if first & 2 else gc0.double()
    loss = (dh_later * h).sum() + (gc_in * c2).sum()
    ddh = n_sl * U * dh_mag
    dh = dh_later.clone()
    if n:
        terms = [gl[:, :n].double()] + ([gxn[:, :n].double(), sl[:, :, :n].sum(0)] if later else [])
        gx = sum(terms)
        gx_mag = gl[:, :n].double().abs() + ((gxn[:, :n].double().abs() + sl[:, :, :n].abs().sum(0)) if later else 0)
        dgx = (n_sl + 2) * U * gx_mag
        assert_ulps(gxo[:, :n], gx, dgx + TINY, "gx_out")
        assert_same(gxo[:, n:], torch.zeros(B, 64 - n), "gx_out beyond n")
        wo = w_out.double()
        loss = loss + (gx * (h @ wo.t())).sum()
        acc, acc_mag = gx @ wo, gx.abs() @ wo.abs()
        ddh = (n_sl + 1) * U * (dh_mag + acc.abs()) + (n + 1) * U * acc_mag + dgx @ wo.abs()
        dh = dh + acc
    rz, rc = torch.autograd.grad(loss, [z, c])
    # ---- bounds.  tc = tanhf(c'): c' is the fp32 rounding of f c + i g (U |c'|) and tanhf's own error
    i_, f_, g_, o_, c2 = (t.detach() for t in (i_, f_, g_, o_, c2))
    tc = torch.tanh(c2)
    dtc = U * c2.abs() + TANH_U * tc.abs()
    w1 = 1 - tc * tc
    dw1 = 2 * tc.abs() * dtc + 2 * U
    t1 = dh * o_ * w1
    dt1 = (o_ * w1).abs() * ddh + (dh * o_).abs() * dw1 + 2 * U * t1.abs()
    dc = gc_in + t1
    ddc = dt1 + U * (gc_in.abs() + t1.abs())
    assert_ulps(gc, rc, f_ * ddc + U * (dc * f_).abs() + TINY, "gc")
    cpd = cp.double()
    # dc a b (1 - b): (1 - b) is off by U absolutely, the three products 3 U
    b0 = (g_ * i_ * (1 - i_)).abs() * ddc + (dc * g_ * i_).abs() * U + 4 * U * rz[..., 0].abs()
    b1 = (cpd * f_ * (1 - f_)).abs() * ddc + (dc * cpd * f_).abs() * U + 4 * U * rz[..., 1].abs()
    b2 = (i_ * (1 - g_ * g_)).abs() * ddc + (dc * i_).abs() * 2 * U + 4 * U * rz[..., 2].abs()
    b3 = (tc * o_ * (1 - o_)).abs() * ddh + (dh * o_ * (1 - o_)).abs() * dtc + (dh * tc * o_).abs() * U + 4 * U * rz[..., 3].abs()
    assert_ulps(dgates, rz, torch.stack([b0, b1, b2, b3], dim=-1) + TINY, "dgates")
