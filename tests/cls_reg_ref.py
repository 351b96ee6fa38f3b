"""Float64 restatements of the classifier-study kernels (csrc/seq_cls.hip) and of the adversarial pose regressor's
(csrc/seq_reg.hip), one per entry point, each with an elementwise bound on what an fp32 evaluation of the same formula may differ
by.  Host only: nothing here touches a GPU.  tests/test_cls_reg_ref.py holds each restatement to torch itself and each bound to an
fp32 stand-in and to a list of mutations; tests/test_hip_cls_reg_kernels.py holds the kernels to them.

Every ``ref_*`` takes what the kernel reads as given (fp32 tensors, widened), is written from the torch definition of the
operation, and returns {output: (float64 value, bound)}.  Bounds follow the conventions in the docstring of
tests/test_hip_seq_kernels.py: U = 2^-24; a correctly rounded +, -, * costs U relative to its result; expf 6 U, logf / log1pf 6 U,
tanhf 10 U, sqrtf 6 U, x / y 5 U, sigmoid_f 12 U; a sum of terms costs c U sum|terms| with c the depth of the kernel's summation
chain; an input's error goes through a later operation to first order (times the operation's derivative).  The compiler may
contract a * b + c into one rounding: wherever the kernel's expression allows that, the bound counts the product's rounding, so it
admits the fused and the unfused result.  TINY (the smallest normal) is added where a bound could be 0 next to a value that is
not: it stands for one rounding in the subnormal range.

``make_*`` build the inputs of one net of one case from a seed; the ``*_CASES`` lists are the cases the GPU tests run, so the host
tests check the bounds on exactly those.
"""
import math

import torch

from hip_parity_utils import DIV_U, EXP_U, LOG_U, NAN, SIG_U, SQRT_U, TANH_U, TINY, U, _f32

# include/vunet_seq_cls.h, include/vunet_seq_reg.h (tests/test_hip_cls_reg_kernels.py compares these with the package's)
NIN, KP, HID, G3 = 51, 64, 256, 768
OFF_WHH = G3 * KP
OFF_BIH = OFF_WHH + G3 * HID
OFF_BHH = OFF_BIH + G3
OFF_FCW = OFF_BHH + G3
OFF_FCB = OFF_FCW + HID
P = OFF_FCB + 4
MAX_BS = 1024
REG_T, REG_C = 50, 128
CLAMP_LO, CLAMP_HI = _f32(0.45), _f32(0.7)       # 0.45f, 0.7f


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g) * scale


def _cdiv(a, b):
    return (a + b - 1) // b


def _up16(b):
    return (b + 15) // 16 * 16


def _sig64(x):
    return 1.0 / (1.0 + torch.exp(-x))


# ================================================================================================ vunet_seq_cls_gather
GATHER_SHAPES = [(3, 51, 64), (1, 32, 32)]          # (T, n, ld); the second is the mu gather: ld == n
GATHER_BS = [1, 37]
GATHER_NB = 3
GATHER_ITS = [0, 2, 3, 10]                          # it % 3 = 0, 2, 0, 1


def make_gather(T, n, bs, with_real, seed):
    g = _gen(seed)
    fake = _randn(g, GATHER_NB * bs, T, n)
    real = _randn(g, GATHER_NB * bs, T, n) if with_real else None
    return dict(fake=fake, real=real)


def ref_gather(fake, real, T, n, ld, bs, nb, it):
    """dst[t][r][k] = set[b bs + r % bs][t][k] (fake rows, then real rows), b = it % nb; 0 for n <= k < ld.  A copy: bound 0."""
    b = it % nb
    rows = [fake[b * bs:(b + 1) * bs]] + ([] if real is None else [real[b * bs:(b + 1) * bs]])
    x = torch.cat(rows, 0).permute(1, 0, 2)                      # [T][R][n]
    dst = torch.zeros(T, x.shape[1], ld, dtype=fake.dtype)
    dst[:, :, :n] = x
    return {"dst": (dst, 0.0)}


# ================================================================================================ vunet_seq_cls_cell_fwd / _bwd
CELL_T = 3
CELL_STEPS = [0, 2]
CELL_ROWS = [1, 37]
CELL_SCALES = [1.0, 8.0]                            # at 8 the pre-activations reach +-30 and beyond: saturated gates


def make_cell_fwd(R, scale, seed):
    g = _gen(seed)
    return dict(gi=_randn(g, CELL_T, R, G3, scale=scale), gh=_randn(g, CELL_T, R, G3, scale=scale), h=_randn(g, CELL_T + 1, R, HID))


def ref_cell_fwd(gi, gh, hprev):
    """torch.nn.GRU's cell, gate order r, z, n: r = sig(gi_r + gh_r), z = sig(gi_z + gh_z), n = tanh(gi_n + r gh_n),
    h' = n + z (h - n) = (1 - z) n + z h.  gi, gh: [R][768], hprev: [R][256].

    a = gi + gh: one rounding, U |a|.  sig' = s (1 - s): ds = s (1 - s) U |a| + SIG_U s.
    arg = gi_n + r gh_n: r's error times |gh_n|, the product's rounding U |r gh_n| (none if contracted), the sum's U |arg|.
    tanh' = 1 - n^2: dn = (1 - n^2) darg + TANH_U |n|.
    h' = n + z d, d = h - n: d h' / d n = 1 - z (the computed n is used in both places), d h' / d z = d; d's rounding U |d| goes
    through z; the product's rounding U |z d| (none if contracted); the sum's U |h'|."""
    gi, gh, hprev = gi.double(), gh.double(), hprev.double()
    ir, iz, inn = gi[:, :HID], gi[:, HID:2 * HID], gi[:, 2 * HID:]
    hr, hz, hn = gh[:, :HID], gh[:, HID:2 * HID], gh[:, 2 * HID:]
    ar, az = ir + hr, iz + hz
    r, z = _sig64(ar), _sig64(az)
    dr = r * (1 - r) * U * ar.abs() + SIG_U * r
    dz = z * (1 - z) * U * az.abs() + SIG_U * z
    arg = inn + r * hn
    darg = dr * hn.abs() + U * (r * hn).abs() + U * arg.abs()
    n = torch.tanh(arg)
    dn = (1 - n * n) * darg + TANH_U * n.abs()
    d = hprev - n
    h2 = n + z * d
    dh2 = (1 - z) * dn + d.abs() * dz + z * U * d.abs() + U * (z * d).abs() + U * h2.abs()
    return {"gates": (torch.cat([r, z, n], 1), torch.cat([dr, dz, dn], 1) + TINY), "h": (h2, dh2 + TINY)}


def make_cell_bwd(R, seed):
    """Stored gates r, z in (0, 1) and n in (-1, 1), with values within 2 U of the ends planted in the first 8 units of row 0."""
    g = _gen(seed)
    gates = torch.cat([torch.sigmoid(_randn(g, CELL_T, R, 2 * HID, scale=3.0)), torch.tanh(_randn(g, CELL_T, R, HID, scale=1.5))], 2)
    ends = torch.tensor([U, 2 * U, 1 - U, 1 - 2 * U, 1 - U, U, 1 - 2 * U, 2 * U])
    for t in range(CELL_T):
        gates[t, 0, 0:8] = ends
        gates[t, 0, HID:HID + 8] = ends.flip(0)
        gates[t, 0, 2 * HID:2 * HID + 8] = torch.tensor([1 - U, -(1 - U), 1 - 2 * U, -(1 - 2 * U), U, -U, 1 - U, -(1 - 2 * U)])
    assert bool(((gates[..., :2 * HID] > 0) & (gates[..., :2 * HID] < 1)).all()) and bool((gates[..., 2 * HID:].abs() < 1).all())
    return dict(gates=gates, gi=_randn(g, CELL_T, R, G3), gh=_randn(g, CELL_T, R, G3), h=_randn(g, CELL_T + 1, R, HID),
                dh=_randn(g, R, HID))


def ref_cell_bwd(gates, ghn, hprev, dh):
    """Back through h' = (1 - z) n + z h with n = tanh(gi_n + r gh_n), r = sig(a_r), z = sig(a_z), from the stored gates:
      d n = dh (1 - z); d z = dh (h - n); da_n = d n (1 - n^2); da_r = da_n gh_n r (1 - r); da_z = d z z (1 - z);
      dgi = (da_r, da_z, da_n); dgh = (da_r, da_z, da_n r); the direct part of d h: dh z.
    gates: [R][768], ghn (the forward's gh_n): [R][256].

    d n: (1 - z) one rounding, the product one: 2 U |d n|.
    1 - n^2: n^2's rounding U n^2 (none if contracted) + the difference's U (1 - n^2), absolute: near |n| = 1 the first is all
    of it.  da_n: |d n| (U n^2 + U (1 - n^2)) + (2 U from d n + U for the product) |da_n|.
    da_r = ((da_n gh_n) r) (1 - r): da_n's error times |gh_n r (1 - r)|, + (1 - r) and three products: 4 U |da_r|.
    da_z = ((dh (h - n)) z) (1 - z): the difference, (1 - z), three products: 5 U |da_z|.
    da_n r: da_n's error times r + U.  dh z: one fp32 product (the GPU test wants it bit-equal)."""
    gates, ghn, hprev, dh = gates.double(), ghn.double(), hprev.double(), dh.double()
    r, z, n = gates[:, :HID], gates[:, HID:2 * HID], gates[:, 2 * HID:]
    dn = dh * (1 - z)
    dz = dh * (hprev - n)
    an = dn * (1 - n * n)
    dan = dn.abs() * (U * n * n + U * (1 - n * n)) + 3 * U * an.abs()
    ar = an * ghn * r * (1 - r)
    dar = (ghn * r * (1 - r)).abs() * dan + 4 * U * ar.abs()
    az = dz * z * (1 - z)
    daz = 5 * U * az.abs()
    anr = an * r
    danr = r * dan + U * anr.abs()
    return {"gi": (torch.cat([ar, az, an], 1), torch.cat([dar, daz, dan], 1) + TINY),
            "gh": (torch.cat([ar, az, anr], 1), torch.cat([dar, daz, danr], 1) + TINY),
            "dh_prev": (dh * z, U * (dh * z).abs() + TINY)}


# ================================================================================================ vunet_seq_cls_head
HEAD_BS = [1, 37, 256, 257, 1024]
HEAD_SCALES = [1.0, 10.0]                           # fc1.w ~ N(0, 1 / 256): the logits' spread is h's; 10 -> about +-30
HEAD_IT, HEAD_SLOT_OFF, HEAD_LD_CURVE = 5, 2, 11


def make_head(bs, with_real, scale, seed):
    """fc1.w[0] = 0.5, fc1.b = 0.25 and row 0 = (-0.5, 0, ...): its logit is fmaf(0.5, -0.5, 0) + 0.25 = 0 exactly."""
    g = _gen(seed)
    R = 2 * bs if with_real else bs
    w = _randn(g, HID, scale=1.0 / 16.0)
    w[0] = 0.5
    hT = _randn(g, R, HID, scale=scale)
    hT[0] = 0.0
    hT[0, 0] = -0.5
    return dict(hT=hT, w=w, fb=0.25)


def ref_head(hT, w, fb, bs, with_real):
    """logit = nn.Linear(256, 1)(h_T); loss = BCEWithLogits(logit[:bs], 0) + BCEWithLogits(logit[bs:], 1) (each a mean),
    acc = mean sigmoid(logit[:bs]); dlogit = sig / bs (fake), (sig - 1) / bs (real); dh = dlogit w; dfc1.w = sum_r dlogit[r] h_T[r];
    dfc1.b = sum_r dlogit[r].  BCEWithLogits(x, y) = (1 - y) x - log_sigmoid(x), log_sigmoid(x) = min(x, 0) - log1p(exp(-|x|)).

    x: 256 fmaf in a chain and the bias: dx = 257 U (sum |w h| + |fb|).
    sig: s (1 - s) dx + SIG_U s.
    e = expf(-|x|): e (dx + EXP_U);  l = log1pf(e): e's error / (1 + e) + LOG_U l;  ls = min(x, 0) - l: dx [x < 0] + dl + U |ls|.
    fake term x - ls: dx + dls + U |x - ls|; real term -ls: dls.
    A thread adds its ceil(R / 256) rows, then a tree of 8 levels: c = ceil(R / 256) + 8; the mean: inv = 1 / bs (DIV_U) and a
    product (U); loss = mean_f + mean_r: one more U (its products' roundings are counted whether it is contracted or not).
    dlogit: (sig - 1)'s rounding U |sig - 1| for real rows, then inv and the product: ds / bs + (DIV_U + U) |dlogit|.
    dh = dlogit w: dlogit's error times |w| + U.  dfc1.w: R fmaf in a chain: sum_r ddlogit |h| + R U sum |dlogit h|; dfc1.b:
    R adds in a chain."""
    hT, w = hT.double(), w.double()
    R = hT.shape[0]
    x = hT @ w + fb
    dx = 257 * U * (hT.abs() @ w.abs() + abs(fb))
    s = _sig64(x)
    ds = s * (1 - s) * dx + SIG_U * s
    e = torch.exp(-x.abs())
    lg = torch.log1p(e)
    dlg = e * (dx + EXP_U) / (1 + e) + LOG_U * lg
    ls = torch.clamp_max(x, 0.0) - lg
    dls = dx * (x < 0) + dlg + U * ls.abs()
    c = _cdiv(R, 256) + 8
    out = {}
    acc_sum = s[:bs].sum()
    acc = acc_sum / bs
    out["acc"] = (acc, (ds[:bs].sum() + c * U * acc_sum) / bs + (DIV_U + U) * acc + TINY)
    dl = s[:bs] / bs
    ddl = ds[:bs] / bs + (DIV_U + U) * dl
    if with_real:
        tf = x[:bs] - ls[:bs]
        dtf = dx[:bs] + dls[:bs] + U * tf.abs()
        tr = -ls[bs:]
        mf, mr = tf.sum() / bs, tr.sum() / bs
        dmf = (dtf.sum() + c * U * tf.abs().sum()) / bs + (DIV_U + U) * mf.abs()
        dmr = (dls[bs:].sum() + c * U * tr.abs().sum()) / bs + (DIV_U + U) * mr.abs()
        out["loss"] = (mf + mr, dmf + dmr + U * (mf + mr).abs() + TINY)
        dlr = (s[bs:] - 1) / bs
        ddlr = (ds[bs:] + U * (s[bs:] - 1).abs()) / bs + (DIV_U + U) * dlr.abs()
        dl, ddl = torch.cat([dl, dlr]), torch.cat([ddl, ddlr])
        dh = dl[:, None] * w[None, :]
        out["dh"] = (dh, ddl[:, None] * w.abs()[None, :] + U * dh.abs() + TINY)
        out["gw"] = (dl @ hT, ddl @ hT.abs() + R * U * (dl.abs() @ hT.abs()) + TINY)
        out["gb"] = (dl.sum(), ddl.sum() + R * U * dl.abs().sum() + TINY)
    return out


# ================================================================================================ vunet_seq_cls_sgd
SGD_S = [1, 8]
SGD_ITS = [0, 1]
SGD_LR, SGD_MOM = 1e-3, 0.9


def make_sgd(S, it, seed):
    """Slices >= 1 of the fc range are NaN (read from slice 0 only); at iteration 0 the buffer is NaN (it must be ignored)."""
    g = _gen(seed)
    grad = _randn(g, S, P)
    grad[1:, OFF_FCW:] = NAN
    buf = torch.full((P,), NAN) if it == 0 else _randn(g, P)
    return dict(params=_randn(g, P), grad=grad, buf=buf)


def sgd_fp32(params, grad, buf, it, lr=SGD_LR, mom=SGD_MOM):
    """The kernel's own order in fp32 (it pins every rounding: no contraction): g = slices added in slice order (the fc range:
    slice 0 alone); buf = g at iteration 0, else mom buf + g; p = p + (-lr) buf."""
    lr, mom = torch.tensor(lr, dtype=torch.float32), torch.tensor(mom, dtype=torch.float32)
    gv = grad[0].clone()
    for s in range(1, grad.shape[0]):
        gv[:OFF_FCW] = gv[:OFF_FCW] + grad[s, :OFF_FCW]
    b = gv if it == 0 else mom * buf + gv
    return params + (-lr) * b, b


def ref_sgd(params, grad, buf, it, lr=SGD_LR, mom=SGD_MOM):
    """torch.optim.SGD(lr, momentum) with dampening 0: buf = g on the first step, momentum buf + g after; p -= lr buf; lr and
    momentum are the fp32 values the kernel is handed.

    g: S - 1 adds in slice order: (S - 1) U sum_s |g_s| (none in the fc range).  buf: g's error, + the product's U |mom buf| and the
    sum's U |buf'| after the first step.  p: lr times buf's error, the product's U |lr buf'|, the sum's U |p'|."""
    lr, mom = _f32(lr), _f32(mom)
    S = grad.shape[0]
    params, grad = params.double(), grad.double()
    gv, mag = grad[0].clone(), torch.zeros(P, dtype=torch.float64)
    gv[:OFF_FCW] = grad[:, :OFF_FCW].sum(0)
    mag[:OFF_FCW] = grad[:, :OFF_FCW].abs().sum(0)
    dg = (S - 1) * U * mag
    if it == 0:
        b, db = gv, dg
    else:
        b = mom * buf.double() + gv
        db = dg + U * (mom * buf.double()).abs() + U * b.abs()
    p2 = params - lr * b
    return {"params": (p2, lr * db + U * (lr * b).abs() + U * p2.abs() + TINY), "buf": (b, db + TINY)}


# ================================================================================================ vunet_seq_cls_reg_loss
CRL_BS = [1, 37, 257]
CRL_LDP = [51, 64]
CRL_T, CRL_NB, CRL_IT = 4, 3, 4                     # batch 4 % 3 = 1
CRL_STARTS = [0, CRL_T - 1, 1]                      # per net


def make_cls_reg_sets(bs, with_xc, seed):
    """The pose sets every net of a launch shares: xo, and xc or None."""
    g = _gen(seed)
    return _randn(g, CRL_NB * bs, CRL_T, NIN), (_randn(g, CRL_NB * bs, CRL_T, NIN) if with_xc else None)


def make_cls_reg_loss(xo, xc, bs, ldp, start, seed):
    """One net: pred = target + noise; row bs // 2 IS the target (d_r = 0); columns 51 .. ldp of pred are NaN (not read)."""
    g = _gen(seed)
    b = CRL_IT % CRL_NB
    pred = torch.full((bs, ldp), NAN)
    pred[:, :NIN] = xo[b * bs:(b + 1) * bs, start] + _randn(g, bs, NIN, scale=0.5)
    pred[bs // 2, :NIN] = xo[b * bs + bs // 2, start]
    return dict(pred=pred, xo=xo, xc=xc)


def _row_norm(u):
    """||u|| over 51 columns as the kernel forms it: u = a - b (U |u|), q = 51 fmaf in a chain: 2 U q from u's roundings + 51 U q;
    sqrtf: half of q's relative error + SQRT_U."""
    nr = u.norm(dim=1)
    return nr, (0.5 * (2 + NIN) * U + SQRT_U) * nr


def ref_cls_reg_loss(pred, xo, xc, bs, nb, it, start):
    """loss = torch.mean(torch.norm(pred - target, dim=1)), target = xo[b bs + r][start], b = it % nb; dpred = its gradient:
    (pred - target) / (d_r bs), 0 where d_r = 0 (torch.norm's backward); de = the same mean for xc against the target.

    The mean: a thread adds its ceil(bs / 256) rows, a tree of 8 levels, then inv = 1 / bs (DIV_U) and the product (U).
    dpred = u sc, sc = inv / d_r: u (U), inv (DIV_U), d_r's relative error, the quotient (DIV_U), the product (U)."""
    b = it % nb
    tg = xo[b * bs:(b + 1) * bs, start].double()
    u = pred[:, :NIN].double() - tg
    nr, dnr = _row_norm(u)
    c = _cdiv(bs, 256) + 8
    loss = nr.sum() / bs
    out = {"loss": (loss, (dnr.sum() + c * U * nr.sum()) / bs + (DIV_U + U) * loss + TINY)}
    safe = torch.where(nr > 0, nr, torch.ones_like(nr))
    dp = torch.where(nr[:, None] > 0, u / (safe[:, None] * bs), torch.zeros_like(u))
    out["dpred"] = (dp, dp.abs() * (2 * U + 2 * DIV_U + (dnr / safe)[:, None]) + TINY * (nr[:, None] > 0))
    if xc is not None:
        n2, dn2 = _row_norm(xc[b * bs:(b + 1) * bs, start].double() - tg)
        de = n2.sum() / bs
        out["de"] = (de, (dn2.sum() + c * U * n2.sum()) / bs + (DIV_U + U) * de + TINY)
    return out


# ================================================================================================ vunet_seq_cls_adam
ADAM_N = [1, 300]
ADAM_STEPS = [1, 1000]
ADAM_LR, ADAM_B1, ADAM_B2, ADAM_EPS = 1e-3, 0.9, 0.999, 1e-8


def make_adam(n, seed):
    """Every third element has g = 0, every sixth also v = 0 (the update's denominator is eps alone)."""
    g = _gen(seed)
    gr, v = _randn(g, n), torch.rand(n, generator=g) * 1e-2
    gr[::3] = 0.0
    v[::6] = 0.0
    return dict(p=_randn(g, n), m=_randn(g, n, scale=1e-1), v=v, g=gr)


def adam_constants(lr, step, b1, b2):
    """{lr / (1 - b1^t), 1 / sqrt(1 - b2^t)} formed in double from the fp32 betas and rounded to fp32 once (seq_adam.h)."""
    return _f32(lr / (1.0 - _f32(b1) ** step)), _f32(1.0 / math.sqrt(1.0 - _f32(b2) ** step))


def ref_adam(p, m, v, g, step_size, inv_sqrt_bc2, b1, b2, eps, dg=0.0, own_constants=False):
    """torch.optim.Adam's update (``_adam64``: float64 Adam on the fp32 state with the bound of seq_adam.h's arithmetic).
    own_constants: the kernel forms the two constants itself (resolved_dev NULL) with the device's pow and sqrt in double; their
    final rounding to fp32 may fall the other way than the host's: one U each on the update."""
    from hip_parity_utils import _adam64
    (p2, dp), (m2, dm), (v2, dv) = _adam64(p, g, m, v, step_size, inv_sqrt_bc2, b1, b2, eps, 0.0, dg)
    if own_constants:
        dp = dp + 2 * U * (p.double() - p2).abs()
    return {"p": (p2, dp), "m": (m2, dm), "v": (v2, dv)}


# ================================================================================================ vunet_seq_reg_gather
RG_B = [1, 5, 16, 17, 64]
RG_H4 = [4, 300]
RG_N = [3, 51]
RG_IDX = [0, 49, -1, 50, 17]                        # idx_dev[0 .. 4]: both ends, both clamped, one inside


def make_reg_gather(B, H4, n, seed):
    """h3's padding rows hold values and a NaN per row: cat carries them.  seq rows are 50 n + 3 apart."""
    g = _gen(seed)
    Bp = _up16(B)
    h3 = _randn(g, Bp, H4)
    h3[B:, 0] = NAN
    return dict(w4=_randn(g, REG_C, REG_T), b4=_randn(g, REG_C), h3=h3, seq=_randn(g, B, REG_T * n + 3))


def ref_reg_gather(w4, b4, h3, seq, idx, n, B):
    """cat = [h3 | relu(fc4(onehot(idx)))] on every padded row (fc4 of a one-hot: column idx of W4 plus b4), tgt = seq[:, idx] on
    rows < B and 0 below; idx clamped into [0, 50).  Copies: bound 0; the fc4 column: one add, U |w + b| (the GPU test also wants
    it bit-equal to the fp32 sum)."""
    idx = min(max(idx, 0), REG_T - 1)
    Bp = h3.shape[0]
    pre = w4[:, idx].double() + b4.double()
    col = torch.clamp_min(pre, 0.0)
    tgt = torch.zeros(Bp, n, dtype=seq.dtype)
    tgt[:B] = seq[:, idx * n:(idx + 1) * n]
    return {"h3": (h3, 0.0), "fc4": (col, U * pre.abs()), "tgt": (tgt, 0.0)}


# ================================================================================================ vunet_seq_reg_loss
RL_B = [1, 5, 64]
RL_N = [3, 51]
RL_LDP = 64
RL_W, RL_S0 = 0.37, 1.25
RL_TARGETS = [None, 0.3, 0.55, 0.9]                 # without scalars; L below 0.45, between 0.45 and 0.7, above 0.7


def make_reg_loss(B, n, target_L, seed):
    """pred = tgt + noise, the noise scaled so that L is target_L (to rounding); padding rows and columns of pred and padding rows
    of tgt are NaN (not read)."""
    g = _gen(seed)
    Bp = _up16(B)
    tgt = torch.full((Bp, n), NAN)
    tgt[:B] = _randn(g, B, n)
    r = _randn(g, B, n)
    if target_L is not None:
        r = r * math.sqrt(target_L / float(r.double().square().mean()))
    pred = torch.full((Bp, RL_LDP), NAN)
    pred[:B, :n] = tgt[:B] + r
    return dict(pred=pred, tgt=tgt)


def ref_reg_loss(pred, tgt, B, n, ldp, w, s0=None):
    """L = F.mse_loss(pred, tgt) over B x n; dpred = 2 (pred - tgt) / (B n), 0 on padding rows and columns.  With s0 (the fifth
    step): loss = s0 - w clamp(L, max=0.45) - w clamp(L, max=0.7); reg5 = d loss / d L = -w ([L <= 0.45] + [L <= 0.7]) (clamp's
    backward keeps the boundary).

    r = pred - tgt: U |r|, so 2 U r^2 on each square; the sum: a thread adds ceil(Bp ldp / 256) squares (each product's rounding: 1,
    none if contracted), a wave's 6 shuffle levels, (a + b) + (c + d): 2; L = sum / (B n): DIV_U.
    dpred = scale r, scale = 2 / (B n): DIV_U, r's U, the product's U.
    loss: L's error times w for each clamp that passes L on; each product U |w min|, each difference U |partial|."""
    w = _f32(w)
    Bp = pred.shape[0]
    r = pred[:B, :n].double() - tgt[:B].double()
    L = r.square().mean()
    c = 2 + _cdiv(Bp * ldp, 256) + 1 + 6 + 2
    dL = (c * U + DIV_U) * L + TINY
    dp = torch.zeros(Bp, ldp, dtype=torch.float64)
    dp[:B, :n] = 2 * r / (B * n)
    out = {"L": (L, dL), "dpred": (dp, dp.abs() * (DIV_U + 2 * U) + TINY * (dp != 0))}
    if s0 is not None:
        m1, m2 = min(float(L), CLAMP_LO), min(float(L), CLAMP_HI)
        l1 = s0 - m1 * w
        l2 = l1 - m2 * w
        k = (1.0 if float(L) <= CLAMP_LO else 0.0) + (1.0 if float(L) <= CLAMP_HI else 0.0)
        out["reg5"] = (torch.tensor(-w * k, dtype=torch.float64), 0.0)
        out["loss"] = (torch.tensor(l2, dtype=torch.float64), k * w * dL + U * (abs(m1 * w) + abs(l1) + abs(m2 * w) + abs(l2)))
    return out


# ================================================================================================ vunet_seq_reg_cat_bwd
CB_S = [1, 3]
CB_BP = [16, 64]
CB_H4 = [4, 256]


def make_cat_bwd(S, Bp, H4, seed):
    """cat holds positive and negative values and, in its first columns of both parts, +0 and -0."""
    g = _gen(seed)
    K5 = H4 + REG_C
    cat = _randn(g, Bp, K5)
    cat[:, 0], cat[:, 1], cat[:, H4], cat[:, H4 + 1] = 0.0, -0.0, -0.0, 0.0
    return dict(raw=_randn(g, S, Bp, K5), cat=cat)


def cat_bwd_fp32(raw, cat, H4):
    """The kernel's order in fp32: slabs added in slab order, times the mask (0 or 1): bit for bit."""
    v = raw[0].clone()
    for s in range(1, raw.shape[0]):
        v = v + raw[s]
    v = v * (cat > 0).float()
    return v[:, :H4].contiguous(), v[:, H4:].contiguous()


def ref_cat_bwd(raw, cat, H4):
    """d / d pre of cat = relu(pre) given d / d cat = the slabs' sum: the sum where cat > 0, 0 elsewhere, split at H4.
    S - 1 adds in slab order: (S - 1) U sum_s |raw_s|."""
    S = raw.shape[0]
    v = raw.double().sum(0) * (cat > 0)
    dv = (S - 1) * U * raw.double().abs().sum(0) * (cat > 0)
    return {"dz3": (v[:, :H4], dv[:, :H4]), "dzc": (v[:, H4:], dv[:, H4:])}


# ================================================================================================ vunet_seq_reg_fc4_adam
FA_BP = [16, 64]
FA_STEPS = [1, 7]
FA_IDX = [0, 49, -3, 50, 23]                        # idx_dev[0 .. 4]; -3 and 50 are clamped to 0 and 49
FA_LR, FA_B1, FA_B2, FA_EPS = 1e-4, 0.9, 0.999, 1e-8


def make_fc4_adam(Bp, seed):
    g = _gen(seed)
    return dict(dzc=_randn(g, Bp, REG_C), w4=_randn(g, REG_C, REG_T), b4=_randn(g, REG_C),
                m4=_randn(g, REG_C, REG_T, scale=1e-1), v4=torch.rand(REG_C, REG_T, generator=g) * 1e-2,
                bm4=_randn(g, REG_C, scale=1e-1), bv4=torch.rand(REG_C, generator=g) * 1e-2)


def ref_fc4_adam(dzc, w4, b4, m4, v4, bm4, bv4, idx, step_size, inv_sqrt_bc2, b1, b2, eps):
    """fc4 = nn.Linear(50, 128) on a one-hot at idx (clamped into [0, 50)): dW4 = dzc^T onehot is dense with one non-zero column,
    g[c] = sum_b dzc[b][c], and db4 = g; torch.optim.Adam moves every column (the others by their moments alone).
    g: a 64-lane butterfly, 6 levels: 6 U sum_b |dzc[b][c]|."""
    idx = min(max(idx, 0), REG_T - 1)
    g = dzc.double().sum(0)
    dg = 6 * U * dzc.double().abs().sum(0)
    gw, dgw = torch.zeros(REG_C, REG_T, dtype=torch.float64), torch.zeros(REG_C, REG_T, dtype=torch.float64)
    gw[:, idx], dgw[:, idx] = g, dg
    W = ref_adam(w4, m4, v4, gw, step_size, inv_sqrt_bc2, b1, b2, eps, dgw)
    Bb = ref_adam(b4, bm4, bv4, g, step_size, inv_sqrt_bc2, b1, b2, eps, dg)
    return {"w4": W["p"], "m4": W["m"], "v4": W["v"], "b4": Bb["p"], "bm4": Bb["m"], "bv4": Bb["v"]}


# ================================================================================================ vunet_seq_reg_adv
ADV_SHAPES = [(5, 96), (64, 256)]
ADV_S = [1, 3]
ADV_REG5 = -0.74


def make_adv(B, H, S, seed):
    """raw's padding rows and reg[0 .. 4] are NaN (not read); gmu's padding rows are NaN (not written)."""
    g = _gen(seed)
    Bp = _up16(B)
    raw = _randn(g, S, Bp, H)
    raw[:, B:] = NAN
    gmu = _randn(g, Bp, H)
    gmu[B:] = NAN
    reg = torch.full((6,), NAN)
    reg[5] = ADV_REG5
    return dict(raw=raw, reg=reg, gmu=gmu)


def ref_adv(raw, reg, gmu, B):
    """a = reg[5] sum_s raw[s] on rows < B; gmu += a; adv = a.  S - 1 adds in slab order, the product (U |a|; counted for gmu too, so
    the contracted v reg5 + gmu is admitted), the sum onto gmu (U |gmu'|)."""
    S = raw.shape[0]
    k = float(reg[5])
    v = raw[:, :B].double().sum(0)
    a = v * k
    da = (S - 1) * U * raw[:, :B].double().abs().sum(0) * abs(k) + U * a.abs()
    g2 = gmu[:B].double() + a
    return {"adv": (a, da + TINY), "gmu": (g2, da + U * g2.abs() + TINY)}
