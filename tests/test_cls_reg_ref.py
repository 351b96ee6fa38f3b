"""Host tests of tests/cls_reg_ref.py, the float64 restatements and bounds that tests/test_hip_cls_reg_kernels.py holds the
classifier-study and regressor kernels to.  No GPU.

  a. each restatement against torch itself in float64 (nn.GRUCell, autograd, nn.Linear + BCEWithLogitsLoss, optim.SGD, optim.Adam,
     torch.norm, mse_loss, clamp), so a restatement is not the kernel's formula copied;
  b. a plain fp32 torch stand-in of each formula lies inside the bound on every case the GPU tests use (a bound is not too tight;
     the worst stand-in error / bound is printed per entry point and output: ``ratio host <entry> <output> <value>``);
  c. the bound rejects each listed mutation of the stand-in (a bound is not too loose to see a wrong formula).
"""
import math

import pytest
import torch
import torch.nn.functional as F

import cls_reg_ref as R
from cls_reg_ref import HID, NIN, OFF_FCW, P, REG_C, REG_T
from hip_parity_utils import U, _f32

F64 = torch.float64


def ratio(got, ref, bound):
    """max |got - ref| / bound over the elements (a zero bound wants equality: inf otherwise)."""
    got, ref = torch.as_tensor(got).detach().double().reshape(-1), torch.as_tensor(ref).double().reshape(-1)
    b = torch.as_tensor(bound).double().reshape(-1).expand_as(ref) if torch.is_tensor(bound) else torch.full_like(ref, float(bound))
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()) and bool(torch.isfinite(ref).all())
    err = (got - ref).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / b)       # x / 0 = inf for x > 0
    return float(q.max()) if q.numel() else 0.0


def ratios(got, ref):
    return {k: ratio(got[k], *ref[k]) for k in ref}


def report(entry, worst):
    for k, v in worst.items():
        print(f"ratio host {entry} {k} {v:.3f}")


def merge(worst, new):
    for k, v in new.items():
        worst[k] = max(worst.get(k, 0.0), v)


def inside(entry, worst):
    report(entry, worst)
    assert all(v <= 1.0 for v in worst.values()), (entry, worst)


def rejected(entry, got, ref):
    r = ratios(got, ref)
    print(f"mutation {entry}: " + " ".join(f"{k} {v:.3g}" for k, v in r.items()))
    assert max(r.values()) > 1.0, (entry, r)


# ================================================================================================ the fp32 stand-ins
def std_cell_fwd(gi, gh, hprev, mut=None):
    ir, iz, inn = gi[:, :HID], gi[:, HID:2 * HID], gi[:, 2 * HID:]
    hr, hz, hn = gh[:, :HID], gh[:, HID:2 * HID], gh[:, 2 * HID:]
    if mut == "zrn":
        ir, iz, hr, hz = iz, ir, hz, hr
    r, z = torch.sigmoid(ir + hr), torch.sigmoid(iz + hz)
    n = torch.tanh(r * inn + hn) if mut == "r_on_gi" else torch.tanh(inn + r * hn)
    h2 = hprev + z * (n - hprev) if mut == "h_plus" else n + z * (hprev - n)
    return {"gates": torch.cat([r, z, n], 1), "h": h2}


def std_cell_bwd(gates, ghn, hprev, dh):
    r, z, n = gates[:, :HID], gates[:, HID:2 * HID], gates[:, 2 * HID:]
    dn, dz = dh * (1 - z), dh * (hprev - n)
    an = dn * (1 - n * n)
    ar, az = an * ghn * r * (1 - r), dz * z * (1 - z)
    return {"gi": torch.cat([ar, az, an], 1), "gh": torch.cat([ar, az, an * r], 1), "dh_prev": dh * z}


def std_head(hT, w, fb, bs, with_real, mut=None):
    x = hT @ w + fb
    s = torch.sigmoid(x)
    out = {"acc": s[:bs].mean()}
    if with_real:
        y = torch.cat([torch.zeros(bs), torch.ones(bs)])
        if mut == "swap":
            y = 1 - y
        out["loss"] = F.binary_cross_entropy_with_logits(x[:bs], y[:bs]) + F.binary_cross_entropy_with_logits(x[bs:], y[bs:])
        dl = (s - y) if mut == "no_bs" else (s - y) / bs
        out["dh"] = dl[:, None] * w[None, :]
        out["gw"] = dl @ hT
        out["gb"] = dl.sum()
    return out


def std_sgd(params, grad, buf, it, mut=None):
    lr, mom = torch.tensor(R.SGD_LR), torch.tensor(R.SGD_MOM)
    gv = grad[0].clone()
    gv[:OFF_FCW] = grad[:, :OFF_FCW].sum(0)
    b = gv if (it == 0 and mut != "mom_at_0") else mom * buf + gv
    return {"params": params - lr * b, "buf": b}


def std_cls_reg_loss(pred, xo, xc, bs, nb, it, start, mut=None):
    b = it % nb
    tg = xo[b * bs:(b + 1) * bs, start]
    u = pred[:, :NIN] - tg
    nr = u.norm(dim=1)
    den = nr * nr * bs if mut == "sq" else nr * bs
    out = {"loss": nr.mean(), "dpred": torch.where(nr[:, None] > 0, u / den[:, None], torch.zeros_like(u))}
    if xc is not None:
        out["de"] = (xc[b * bs:(b + 1) * bs, start] - tg).norm(dim=1).mean()
    return out


def std_adam(p, m, v, g, step_size, k2, b1, b2, eps, mut=None):
    step_size, k2, b1, b2, eps = (torch.tensor(x, dtype=torch.float32) for x in (step_size, 1.0 if mut == "no_bc2" else k2, b1, b2, eps))
    g = g.float()
    m2 = b1 * m + (1 - b1) * g
    v2 = b2 * v + (1 - b2) * g * g
    return {"p": p - step_size * (m2 / (v2.sqrt() * k2 + eps)), "m": m2, "v": v2}


def std_reg_gather(w4, b4, h3, seq, idx, n, B):
    idx = min(max(idx, 0), REG_T - 1)
    return {"fc4": torch.clamp_min(w4[:, idx] + b4, 0.0)}


def std_reg_loss(pred, tgt, B, n, ldp, w, s0=None, mut=None):
    w, lo, hi = torch.tensor(w), torch.tensor(R.CLAMP_LO), torch.tensor(R.CLAMP_HI)
    r = pred[:B, :n] - tgt[:B]
    L = (r * r).mean()
    dp = torch.zeros(pred.shape[0], ldp)
    dp[:B, :n] = (1.0 if mut == "half" else 2.0) * r / (B * n)
    out = {"L": L, "dpred": dp}
    if s0 is not None:
        k = ((L < lo).float() + (L < hi).float()) if mut == "lt" else ((L <= lo).float() + (L <= hi).float())
        out["reg5"] = -w * k
        out["loss"] = torch.tensor(s0) - torch.minimum(L, lo) * w - torch.minimum(L, hi) * w
    return out


def std_cat_bwd(raw, cat, H4, mut=None):
    v = raw.sum(0)
    v = v * ((v if mut == "mask_raw" else cat) > 0).float()
    return {"dz3": v[:, :H4], "dzc": v[:, H4:]}


def std_fc4_adam(dzc, w4, b4, m4, v4, bm4, bv4, idx, step_size, k2, b1, b2, eps, mut=None):
    idx = min(max(idx, 0), REG_T - 1)
    g = dzc.sum(0)
    gw = torch.zeros(REG_C, REG_T)
    gw[:, (idx + 1) % REG_T if mut == "next_col" else idx] = g
    W, Bb = std_adam(w4, m4, v4, gw, step_size, k2, b1, b2, eps), std_adam(b4, bm4, bv4, g, step_size, k2, b1, b2, eps)
    return {"w4": W["p"], "m4": W["m"], "v4": W["v"], "b4": Bb["p"], "bm4": Bb["m"], "bv4": Bb["v"]}


def std_adv(raw, reg, gmu, B):
    a = raw[:, :B].sum(0) * reg[5]
    return {"adv": a, "gmu": gmu[:B] + a}


# ================================================================================================ a. against torch in float64
def _rel(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def test_gather_restatement_follows_the_header_formula():
    """ref_gather against dst[t][r][k] = set[b bs + r % bs][t][k] spelled out element by element."""
    T, n, ld, bs, nb = 3, 5, 8, 2, 3
    d = dict(fake=torch.arange(nb * bs * T * n, dtype=torch.float32).view(nb * bs, T, n), real=None)
    d["real"] = -d["fake"] - 1
    for it in (0, 4):
        dst = R.ref_gather(d["fake"], d["real"], T, n, ld, bs, nb, it)["dst"][0]
        b = it % nb
        for t in range(T):
            for r in range(2 * bs):
                for k in range(ld):
                    want = 0.0 if k >= n else float((d["fake"] if r < bs else d["real"])[b * bs + r % bs, t, k])
                    assert float(dst[t, r, k]) == want
        assert R.ref_gather(d["fake"], None, T, n, ld, bs, nb, it)["dst"][0].shape == (T, bs, ld)


def _gru_cell(seed):
    torch.manual_seed(seed)
    cell = torch.nn.GRUCell(NIN, HID).double()                       # weights packed in gate order r, z, n
    x, h = torch.randn(7, NIN, dtype=F64), torch.randn(7, HID, dtype=F64)
    gi = x @ cell.weight_ih.t() + cell.bias_ih
    gh = h @ cell.weight_hh.t() + cell.bias_hh
    return cell, x, h, gi.detach(), gh.detach()


def test_cell_fwd_restatement_vs_gru_cell():
    cell, x, h, gi, gh = _gru_cell(1)
    out = R.ref_cell_fwd(gi, gh, h)
    assert _rel(out["h"][0], cell(x, h).detach()) < 1e-13
    one = torch.nn.GRU(NIN, HID, batch_first=True).double()
    one.load_state_dict({k + "_l0": v for k, v in cell.state_dict().items()})
    assert _rel(out["h"][0], one(x[:, None, :], h[None])[0][:, 0].detach()) < 1e-13


def test_cell_bwd_restatement_vs_autograd():
    """Autograd of the step with gi, gh and h as leaves (the recurrent product is the GEMM's business): d / d gi, d / d gh and the
    direct d / d h."""
    _, _, h, gi, gh = _gru_cell(2)
    gi, gh, h = (t.clone().requires_grad_(True) for t in (gi, gh, h))
    r = torch.sigmoid(gi[:, :HID] + gh[:, :HID])
    z = torch.sigmoid(gi[:, HID:2 * HID] + gh[:, HID:2 * HID])
    n = torch.tanh(gi[:, 2 * HID:] + r * gh[:, 2 * HID:])
    h2 = (1 - z) * n + z * h
    dh = torch.randn(7, HID, dtype=F64)
    dgi, dgh, dhp = torch.autograd.grad((h2 * dh).sum(), [gi, gh, h])
    out = R.ref_cell_bwd(torch.cat([r, z, n], 1).detach(), gh[:, 2 * HID:].detach(), h.detach(), dh)
    assert _rel(out["gi"][0], dgi) < 1e-13 and _rel(out["gh"][0], dgh) < 1e-13 and _rel(out["dh_prev"][0], dhp) < 1e-13


def test_head_restatement_vs_linear_and_bce():
    torch.manual_seed(3)
    bs = 9
    fc = torch.nn.Linear(HID, 1).double()
    hT = (torch.randn(2 * bs, HID, dtype=F64) * 4).requires_grad_(True)
    logit = fc(hT)[:, 0]
    bce = torch.nn.BCEWithLogitsLoss()
    loss = bce(logit[:bs], torch.zeros(bs, dtype=F64)) + bce(logit[bs:], torch.ones(bs, dtype=F64))
    dh, gw, gb = torch.autograd.grad(loss, [hT, fc.weight, fc.bias])
    out = R.ref_head(hT.detach(), fc.weight.detach()[0], float(fc.bias.detach()), bs, 1)
    assert _rel(out["loss"][0], loss.detach()) < 1e-13 and _rel(out["acc"][0], torch.sigmoid(logit[:bs]).mean().detach()) < 1e-13
    assert _rel(out["dh"][0], dh) < 1e-13 and _rel(out["gw"][0], gw[0]) < 1e-13 and _rel(out["gb"][0], gb[0]) < 1e-13
    alone = R.ref_head(hT.detach()[:bs], fc.weight.detach()[0], float(fc.bias.detach()), bs, 0)
    assert set(alone) == {"acc"} and _rel(alone["acc"][0], out["acc"][0]) < 1e-15


def test_sgd_restatement_vs_torch_optim_sgd_over_three_steps():
    g = torch.Generator().manual_seed(4)
    S = 3
    p = torch.randn(P, generator=g)
    ref_p, buf = p.clone(), torch.full((P,), float("nan"))
    tp = p.double().clone().requires_grad_(True)
    opt = torch.optim.SGD([tp], lr=_f32(R.SGD_LR), momentum=_f32(R.SGD_MOM))
    for it in range(3):
        grad = torch.randn(S, P, generator=g)
        grad[1:, OFF_FCW:] = float("nan")
        gv = grad[0].double().clone()
        gv[:OFF_FCW] = grad[:, :OFF_FCW].double().sum(0)
        tp.grad = gv
        opt.step()
        out = R.ref_sgd(ref_p, grad, buf, it)
        assert _rel(out["buf"][0], opt.state[tp]["momentum_buffer"]) < 1e-13
        # the restatement restarts from the fp32 state each step: compare one step from the same state
        step_from = ref_p.double() - _f32(R.SGD_LR) * opt.state[tp]["momentum_buffer"]
        assert _rel(out["params"][0], step_from) < 1e-13
        f32p, f32b = R.sgd_fp32(ref_p, grad, buf, it)
        assert ratio(f32p, *out["params"]) <= 1 and ratio(f32b, *out["buf"]) <= 1
        ref_p, buf = out["params"][0].float(), out["buf"][0].float()
        with torch.no_grad():
            tp.copy_(ref_p.double())
            opt.state[tp]["momentum_buffer"].copy_(buf.double())


def test_cls_reg_loss_restatement_vs_torch_norm():
    d = R.make_cls_reg_loss(*R.make_cls_reg_sets(6, True, 5), 6, 64, 2, 5)
    b = R.CRL_IT % R.CRL_NB
    tg = d["xo"][b * 6:(b + 1) * 6, 2].double()
    pred = d["pred"][:, :NIN].double().requires_grad_(True)
    loss = torch.mean(torch.norm(pred - tg, dim=1))
    (dp,) = torch.autograd.grad(loss, [pred])
    out = R.ref_cls_reg_loss(d["pred"], d["xo"], d["xc"], 6, R.CRL_NB, R.CRL_IT, 2)
    assert float((pred[3] - tg[3]).detach().abs().max()) == 0.0 and not torch.isnan(dp).any() and bool((dp[3] == 0).all())
    assert _rel(out["loss"][0], loss.detach()) < 1e-13 and _rel(out["dpred"][0], dp) < 1e-13
    assert bool((out["dpred"][0][3] == 0).all()) and bool((out["dpred"][1][3] == 0).all())
    de = torch.mean(torch.norm(d["xc"][b * 6:(b + 1) * 6, 2].double() - tg, dim=1))
    assert _rel(out["de"][0], de) < 1e-13


def _threshold_case():
    """B = 1, n = 4, tgt = 0, pred = 2 b_i / 2^12 with sum b_i^2 = 2^24 0.45f: L = sum pred^2 / 4 IS 0.45f, in float64 and in fp32
    (every square and partial sum is an integer below 2^24 over a power of two)."""
    N = R.CLAMP_LO * 2.0 ** 24
    assert N == int(N)
    N = int(N)
    for a in range(math.isqrt(N), 0, -1):
        for b in range(math.isqrt(N - a * a), -1, -1):
            rem = N - a * a - b * b
            c = math.isqrt(rem)
            if c * c == rem:
                pred = torch.zeros(16, R.RL_LDP)
                pred[0, :4] = torch.tensor([a, b, c, 0], dtype=torch.float32) * 2 / 4096
                return dict(pred=pred, tgt=torch.zeros(16, 4))
    raise AssertionError("no three squares")


def test_reg_loss_restatement_vs_mse_and_clamp():
    w, s0 = _f32(R.RL_W), R.RL_S0
    cases = [R.make_reg_loss(5, 51, t, 6) for t in (0.3, 0.55, 0.9)] + [_threshold_case()]
    for i, d in enumerate(cases):
        B, n = (5, 51) if i < 3 else (1, 4)
        pred = d["pred"][:B, :n].double().requires_grad_(True)
        L = F.mse_loss(pred, d["tgt"][:B].double())
        (dp,) = torch.autograd.grad(L, [pred])
        Lq = L.detach().clone().requires_grad_(True)
        loss = s0 - w * torch.clamp(Lq, max=R.CLAMP_LO) - w * torch.clamp(Lq, max=R.CLAMP_HI)
        (coef,) = torch.autograd.grad(loss, [Lq])
        out = R.ref_reg_loss(d["pred"], d["tgt"], B, n, R.RL_LDP, R.RL_W, s0)
        assert _rel(out["L"][0], L.detach()) < 1e-13 and _rel(out["dpred"][0][:B, :n], dp) < 1e-13
        assert float(out["dpred"][0][B:].abs().sum()) == 0 and float(out["dpred"][0][:, n:].abs().sum()) == 0
        assert float(out["reg5"][0]) == float(coef) and _rel(out["loss"][0], loss.detach()) < 1e-13
        assert float(coef) == [-2 * w, -w, 0.0, -2 * w][i]
    assert float(R.ref_reg_loss(cases[3]["pred"], cases[3]["tgt"], 1, 4, R.RL_LDP, R.RL_W, s0)["L"][0]) == R.CLAMP_LO


def test_fc4_restatements_vs_linear_on_a_one_hot_and_torch_adam():
    """fc4 = nn.Linear(50, 128): the forward column (ref_reg_gather), and two Adam steps at different indices -- the second with
    non-zero moments, so the first step's column moves on without a gradient (ref_fc4_adam)."""
    torch.manual_seed(7)
    Bp, n = 16, 3
    fc4 = torch.nn.Linear(REG_T, REG_C).double()
    opt = torch.optim.Adam(fc4.parameters(), lr=R.FA_LR, betas=(_f32(R.FA_B1), _f32(R.FA_B2)), eps=_f32(R.FA_EPS))
    st = {k: torch.zeros(s) for k, s in (("m4", (REG_C, REG_T)), ("v4", (REG_C, REG_T)), ("bm4", (REG_C,)), ("bv4", (REG_C,)))}
    for step, idx in ((1, 49), (2, 0)):
        w4, b4 = fc4.weight.detach().float(), fc4.bias.detach().float()
        with torch.no_grad():                                      # the restatement starts from the fp32 state
            fc4.weight.copy_(w4.double())
            fc4.bias.copy_(b4.double())
        onehot = torch.zeros(Bp, REG_T, dtype=F64)
        onehot[:, idx] = 1.0
        y = fc4(onehot)
        h3, seq = torch.randn(Bp, 4), torch.randn(Bp, REG_T * n + 3)
        got = R.ref_reg_gather(w4, b4, h3, seq, idx, n, Bp)
        assert _rel(got["fc4"][0], torch.relu(y[0]).detach()) < 1e-13
        assert torch.equal(got["tgt"][0], seq[:, :REG_T * n].view(Bp, REG_T, n)[:, idx]) and torch.equal(got["h3"][0], h3)
        dzc = torch.randn(Bp, REG_C)
        opt.zero_grad()
        (y * dzc.double()).sum().backward()
        dense = fc4.weight.grad.clone()
        assert int((dense.abs().sum(0) > 0).sum()) == 1 and float(dense[:, idx].abs().min()) > 0
        opt.step()
        s1, k2 = R.FA_LR / (1 - _f32(R.FA_B1) ** step), 1 / math.sqrt(1 - _f32(R.FA_B2) ** step)
        out = R.ref_fc4_adam(dzc, w4, b4, st["m4"], st["v4"], st["bm4"], st["bv4"], idx, s1, k2, R.FA_B1, R.FA_B2, R.FA_EPS)
        sw, sb = opt.state[fc4.weight], opt.state[fc4.bias]
        for k, want in (("w4", fc4.weight), ("b4", fc4.bias), ("m4", sw["exp_avg"]), ("v4", sw["exp_avg_sq"]), ("bm4", sb["exp_avg"]),
                        ("bv4", sb["exp_avg_sq"])):
            assert _rel(out[k][0], want.detach()) < 1e-10, k
        if step == 2:
            assert float((out["w4"][0][:, 49] - w4[:, 49].double()).abs().min()) > 0      # untouched column, moved by its moments
        for k in st:                                               # carry the moments on (exact in float64 -> fp32 -> float64?  no:
            st[k] = out[k][0].float()                              # rounded, and torch's state is set to the rounded values)
        with torch.no_grad():
            sw["exp_avg"].copy_(st["m4"].double())
            sw["exp_avg_sq"].copy_(st["v4"].double())
            sb["exp_avg"].copy_(st["bm4"].double())
            sb["exp_avg_sq"].copy_(st["bv4"].double())
    # out-of-range indices read and update the clamped column
    for bad, col in ((-3, 0), (50, 49)):
        a = R.ref_fc4_adam(dzc, w4, b4, st["m4"], st["v4"], st["bm4"], st["bv4"], bad, s1, k2, R.FA_B1, R.FA_B2, R.FA_EPS)
        b = R.ref_fc4_adam(dzc, w4, b4, st["m4"], st["v4"], st["bm4"], st["bv4"], col, s1, k2, R.FA_B1, R.FA_B2, R.FA_EPS)
        assert all(torch.equal(a[k][0], b[k][0]) for k in a)


def test_adam_restatement_vs_torch_adam():
    d = R.make_adam(300, 8)
    for step in (1, 1000):
        tp = d["p"].double().clone().requires_grad_(True)
        opt = torch.optim.Adam([tp], lr=R.ADAM_LR, betas=(_f32(R.ADAM_B1), _f32(R.ADAM_B2)), eps=_f32(R.ADAM_EPS))
        opt.state[tp] = {"step": torch.tensor(float(step - 1)), "exp_avg": d["m"].double().clone(), "exp_avg_sq": d["v"].double().clone()}
        tp.grad = d["g"].double().clone()
        opt.step()
        s1, k2 = R.ADAM_LR / (1 - _f32(R.ADAM_B1) ** step), 1 / math.sqrt(1 - _f32(R.ADAM_B2) ** step)
        out = R.ref_adam(d["p"], d["m"], d["v"], d["g"], s1, k2, R.ADAM_B1, R.ADAM_B2, R.ADAM_EPS)
        assert _rel(out["p"][0], tp.detach()) < 1e-10 and _rel(out["m"][0], opt.state[tp]["exp_avg"]) < 1e-13
        assert _rel(out["v"][0], opt.state[tp]["exp_avg_sq"]) < 1e-13


def test_cat_bwd_restatement_vs_autograd_through_relu():
    d = R.make_cat_bwd(3, 16, 4, 9)
    pre = d["cat"].double().clone().requires_grad_(True)             # relu(pre) > 0 exactly where pre > 0
    (torch.relu(pre) * d["raw"].double().sum(0)).sum().backward()
    out = R.ref_cat_bwd(d["raw"], torch.relu(d["cat"]), 4)
    assert torch.equal(out["dz3"][0], pre.grad[:, :4]) and torch.equal(out["dzc"][0], pre.grad[:, 4:])
    a, b = R.cat_bwd_fp32(d["raw"], d["cat"], 4)
    assert ratio(a, *out["dz3"]) <= 1 and ratio(b, *out["dzc"]) <= 1


def test_adv_restatement_vs_autograd():
    """loss = reg5 L(mu) with d L / d mu = the slabs' sum: d loss / d mu = reg5 sum_s raw[s], added onto gmu."""
    d = R.make_adv(5, 96, 3, 10)
    mu = torch.zeros(5, 96, dtype=F64, requires_grad=True)
    mu.grad = d["gmu"][:5].double().clone()
    (float(d["reg"][5]) * (mu * d["raw"][:, :5].double().sum(0)).sum()).backward()
    out = R.ref_adv(d["raw"], d["reg"], d["gmu"], 5)
    assert _rel(out["gmu"][0], mu.grad) < 1e-13


# ================================================================================================ b. the fp32 stand-in inside the bounds
SEEDS = (0, 1, 2)                                   # the three nets of a GPU launch


def test_standin_cell_fwd_inside_the_bound():
    worst = {}
    for Rr in R.CELL_ROWS:
        for scale in R.CELL_SCALES:
            for s in SEEDS:
                d = R.make_cell_fwd(Rr, scale, 100 + s)
                for t in R.CELL_STEPS:
                    merge(worst, ratios(std_cell_fwd(d["gi"][t], d["gh"][t], d["h"][t]), R.ref_cell_fwd(d["gi"][t], d["gh"][t], d["h"][t])))
    inside("vunet_seq_cls_cell_fwd", worst)


def test_standin_cell_bwd_inside_the_bound():
    worst = {}
    for Rr in R.CELL_ROWS:
        for s in SEEDS:
            d = R.make_cell_bwd(Rr, 200 + s)
            for t in R.CELL_STEPS:
                a = (d["gates"][t], d["gh"][t][:, 2 * HID:], d["h"][t], d["dh"])
                merge(worst, ratios(std_cell_bwd(*a), R.ref_cell_bwd(*a)))
    inside("vunet_seq_cls_cell_bwd", worst)


def test_standin_head_inside_the_bound():
    worst = {}
    for bs in R.HEAD_BS:
        for scale in R.HEAD_SCALES:
            for with_real in (1, 0):
                for s in SEEDS:
                    d = R.make_head(bs, with_real, scale, 300 + s)
                    ref = R.ref_head(d["hT"], d["w"], d["fb"], bs, with_real)
                    got = std_head(d["hT"], d["w"], d["fb"], bs, with_real)
                    assert float(got["acc"]) == float(got["acc"]) and float((d["hT"][0] * d["w"]).sum() + d["fb"]) == 0.0
                    merge(worst, ratios(got, ref))
    inside("vunet_seq_cls_head", worst)


def test_standin_sgd_inside_the_bound():
    worst = {}
    for S in R.SGD_S:
        for it in R.SGD_ITS:
            d = R.make_sgd(S, it, 400)
            merge(worst, ratios(std_sgd(d["params"], d["grad"], d["buf"], it), R.ref_sgd(d["params"], d["grad"], d["buf"], it)))
    inside("vunet_seq_cls_sgd", worst)


def test_standin_cls_reg_loss_inside_the_bound():
    worst = {}
    for bs in R.CRL_BS:
        for ldp in R.CRL_LDP:
            for with_xc in (False, True):
                sets = R.make_cls_reg_sets(bs, with_xc, 500)
                for s in SEEDS:
                    d = R.make_cls_reg_loss(*sets, bs, ldp, R.CRL_STARTS[s], 500 + s)
                    a = (d["pred"], d["xo"], d["xc"], bs, R.CRL_NB, R.CRL_IT, R.CRL_STARTS[s])
                    merge(worst, ratios(std_cls_reg_loss(*a), R.ref_cls_reg_loss(*a)))
    inside("vunet_seq_cls_reg_loss", worst)


def test_standin_adam_inside_the_bound():
    worst = {}
    for n in R.ADAM_N:
        for step in R.ADAM_STEPS:
            for s in SEEDS:
                d = R.make_adam(n, 600 + s)
                c = R.adam_constants(R.ADAM_LR, step, R.ADAM_B1, R.ADAM_B2)
                a = (d["p"], d["m"], d["v"], d["g"], *c, R.ADAM_B1, R.ADAM_B2, R.ADAM_EPS)
                merge(worst, ratios(std_adam(*a), R.ref_adam(*a, own_constants=True)))
    inside("vunet_seq_cls_adam", worst)


def test_standin_reg_gather_inside_the_bound():
    worst = {}
    for n in R.RG_N:
        d = R.make_reg_gather(5, 4, n, 700)
        for idx in R.RG_IDX:
            ref = R.ref_reg_gather(d["w4"], d["b4"], d["h3"], d["seq"], idx, n, 5)
            merge(worst, {"fc4": ratio(std_reg_gather(d["w4"], d["b4"], d["h3"], d["seq"], idx, n, 5)["fc4"], *ref["fc4"])})
    inside("vunet_seq_reg_gather", worst)


def test_standin_reg_loss_inside_the_bound():
    worst = {}
    for B in R.RL_B:
        for n in R.RL_N:
            for tL in R.RL_TARGETS:
                d = R.make_reg_loss(B, n, tL, 800 + B + n)
                s0 = None if tL is None else R.RL_S0
                ref = R.ref_reg_loss(d["pred"], d["tgt"], B, n, R.RL_LDP, R.RL_W, s0)
                if tL is not None:                                  # L is further from both thresholds than its bound
                    L, dL = float(ref["L"][0]), float(ref["L"][1])
                    assert min(abs(L - R.CLAMP_LO), abs(L - R.CLAMP_HI)) > dL and abs(L - tL) < 1e-3
                merge(worst, ratios(std_reg_loss(d["pred"], d["tgt"], B, n, R.RL_LDP, R.RL_W, s0), ref))
    inside("vunet_seq_reg_loss", worst)


def test_standin_cat_bwd_inside_the_bound():
    worst = {}
    for S in R.CB_S:
        for Bp in R.CB_BP:
            for H4 in R.CB_H4:
                d = R.make_cat_bwd(S, Bp, H4, 900 + S)
                merge(worst, ratios(std_cat_bwd(d["raw"], d["cat"], H4), R.ref_cat_bwd(d["raw"], d["cat"], H4)))
    inside("vunet_seq_reg_cat_bwd", worst)


def _fa_args(d, idx, step):
    c = R.adam_constants(R.FA_LR, step, R.FA_B1, R.FA_B2)
    return (d["dzc"], d["w4"], d["b4"], d["m4"], d["v4"], d["bm4"], d["bv4"], idx, *c, R.FA_B1, R.FA_B2, R.FA_EPS)


def test_standin_fc4_adam_inside_the_bound():
    worst = {}
    for Bp in R.FA_BP:
        d = R.make_fc4_adam(Bp, 1000 + Bp)
        for step in R.FA_STEPS:
            for idx in R.FA_IDX:
                a = _fa_args(d, idx, step)
                merge(worst, ratios(std_fc4_adam(*a), R.ref_fc4_adam(*a)))
    inside("vunet_seq_reg_fc4_adam", worst)


def test_standin_adv_inside_the_bound():
    worst = {}
    for B, H in R.ADV_SHAPES:
        for S in R.ADV_S:
            d = R.make_adv(B, H, S, 1100 + S)
            merge(worst, ratios(std_adv(d["raw"], d["reg"], d["gmu"], B), R.ref_adv(d["raw"], d["reg"], d["gmu"], B)))
    inside("vunet_seq_reg_adv", worst)


# ================================================================================================ c. the bounds reject the mutations
@pytest.mark.parametrize("mut", ["zrn", "r_on_gi", "h_plus"])
def test_bound_rejects_gru_mutations(mut):
    """Gates read in the order z, r, n; r applied to gi_n instead of gh_n; h' = h + z (n - h)."""
    d = R.make_cell_fwd(37, 1.0, 101)
    a = (d["gi"][2], d["gh"][2], d["h"][2])
    rejected(mut, std_cell_fwd(*a, mut=mut), R.ref_cell_fwd(*a))


@pytest.mark.parametrize("mut", ["swap", "no_bs"])
def test_bound_rejects_head_mutations(mut):
    """BCE targets swapped; dlogit not divided by bs."""
    d = R.make_head(37, 1, 1.0, 301)
    rejected(mut, std_head(d["hT"], d["w"], d["fb"], 37, 1, mut=mut), R.ref_head(d["hT"], d["w"], d["fb"], 37, 1))


def test_bound_rejects_sgd_using_the_buffer_at_iteration_0():
    d = R.make_sgd(1, 1, 401)                                       # (iteration 1's inputs: a finite, non-zero buffer)
    rejected("mom_at_0", std_sgd(d["params"], d["grad"], d["buf"], 0, mut="mom_at_0"), R.ref_sgd(d["params"], d["grad"], d["buf"], 0))


def test_bound_rejects_adam_without_the_second_bias_correction():
    d = R.make_adam(300, 601)
    for step in R.ADAM_STEPS:
        c = R.adam_constants(R.ADAM_LR, step, R.ADAM_B1, R.ADAM_B2)
        a = (d["p"], d["m"], d["v"], d["g"], *c, R.ADAM_B1, R.ADAM_B2, R.ADAM_EPS)
        rejected(f"no_bc2 step {step}", std_adam(*a, mut="no_bc2"), R.ref_adam(*a, own_constants=True))


def test_bound_rejects_dpred_over_the_squared_norm():
    d = R.make_cls_reg_loss(*R.make_cls_reg_sets(37, False, 500), 37, 64, 1, 501)
    a = (d["pred"], d["xo"], d["xc"], 37, R.CRL_NB, R.CRL_IT, 1)
    rejected("sq", std_cls_reg_loss(*a, mut="sq"), R.ref_cls_reg_loss(*a))


def test_bound_rejects_the_halved_mse_scale():
    d = R.make_reg_loss(5, 51, 0.3, 801)
    rejected("half", std_reg_loss(d["pred"], d["tgt"], 5, 51, R.RL_LDP, R.RL_W, R.RL_S0, mut="half"),
             R.ref_reg_loss(d["pred"], d["tgt"], 5, 51, R.RL_LDP, R.RL_W, R.RL_S0))


def test_bound_rejects_a_strict_clamp_coefficient_at_the_threshold():
    """L constructed equal to 0.45f in the float64 reference and in fp32: ``<=`` gives -2 w, ``<`` gives -w."""
    d = _threshold_case()
    ref = R.ref_reg_loss(d["pred"], d["tgt"], 1, 4, R.RL_LDP, R.RL_W, R.RL_S0)
    assert float(ref["L"][0]) == R.CLAMP_LO and float(ref["reg5"][0]) == -2 * _f32(R.RL_W)
    good = std_reg_loss(d["pred"], d["tgt"], 1, 4, R.RL_LDP, R.RL_W, R.RL_S0)
    assert float(good["L"]) == R.CLAMP_LO and max(ratios(good, ref).values()) <= 1
    bad = std_reg_loss(d["pred"], d["tgt"], 1, 4, R.RL_LDP, R.RL_W, R.RL_S0, mut="lt")
    assert float(bad["reg5"]) == -_f32(R.RL_W)
    rejected("lt", bad, ref)


def test_bound_rejects_fc4_gradient_in_the_next_column():
    d = R.make_fc4_adam(16, 1016)
    a = _fa_args(d, 23, 7)
    rejected("next_col", std_fc4_adam(*a, mut="next_col"), R.ref_fc4_adam(*a))


def test_bound_rejects_the_relu_mask_taken_from_raw():
    d = R.make_cat_bwd(3, 16, 4, 903)
    rejected("mask_raw", std_cat_bwd(d["raw"], d["cat"], 4, mut="mask_raw"), R.ref_cat_bwd(d["raw"], d["cat"], 4))


def test_constants_are_the_documented_ones():
    assert (R.EXP_U, R.LOG_U, R.TANH_U, R.SQRT_U, R.DIV_U, R.SIG_U) == (6 * U, 6 * U, 10 * U, 6 * U, 5 * U, 12 * U) and U == 2.0 ** -24
    assert R.P == 247556 and (REG_T, REG_C) == (50, 128)
