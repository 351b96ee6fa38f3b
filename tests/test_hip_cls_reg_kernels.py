"""-m gpu: the training kernels of the classifier study (csrc/seq_cls.hip) and of the adversarial pose regressor (csrc/seq_reg.hip),
one entry point at a time through the C ABI, against the float64 restatements and bounds of tests/cls_reg_ref.py (which
tests/test_cls_reg_ref.py holds to torch itself, to an fp32 stand-in and to a list of mutations, on the host).

Conventions: those of tests/test_hip_seq_kernels.py (outputs NaN-filled with a guard band behind them; copies bit-exact;
reductions c U sum|terms|; the transcendental constants), and in addition:
  * inputs a kernel must not read are NaN;
  * an entry point that takes nets runs with nets = 3 on distinct data, every net stride it takes 40 elements larger than needed,
    NaN in the gaps of inputs and outputs (``_pack`` / ``_unpack``: a gap that is written shows);
  * net 1 of that launch is bit-equal to a nets = 1 launch on net 1's data (a net never reads its neighbour's block);
  * each test prints the worst error / bound of each output: ``ratio gpu <entry> <output> <value>``.
The shapes are the smallest that reach each code path; none is the study's or the trainer's own.

The census in tests/test_cabi_and_host.py requires every ``extern "C" int vunet_*`` of the two files to be named here or listed
in NOT_HELD with a reason.
"""
import ctypes

import pytest
import torch

import cls_reg_ref as R
from cls_reg_ref import G3, HID, NIN, OFF_FCB, OFF_FCW, P, REG_C, REG_T, _up16
from hip_parity_utils import ERR_ARG, NAN, Outs, _adam_hp, _d, _refused, assert_same, assert_ulps

pytestmark = pytest.mark.gpu

NOT_HELD = {
    "vunet_seq_cls_gemm_run": "held alone, against float64 matmul over 3 nets at their own strides, by tests/test_hip_pointwise.py",
}

GAP = 40
WORST = {}


def _m():
    from behavior_driven_video_synthesis_amd import ops, seq_cls, seq_train
    return ops, seq_cls, seq_train


def held(entry, name, got, ref, tag):
    """|got - ref| <= bound elementwise (assert_ulps), after noting the worst error / bound."""
    value, bound = ref
    g, v = got.detach().cpu().double().reshape(-1), torch.as_tensor(value).double().reshape(-1)
    b = bound.double().reshape(-1).expand_as(v) if torch.is_tensor(bound) else torch.full_like(v, float(bound))
    err = (g - v).abs()
    q = torch.where(err == 0, torch.zeros_like(err), err / b)
    q = q[~torch.isnan(q)]
    w = WORST.setdefault(entry, {})
    w[name] = max(w.get(name, 0.0), float(q.max()) if q.numel() else 0.0)
    assert_ulps(got, torch.as_tensor(value), bound if torch.is_tensor(bound) else float(bound), f"{entry} {name} {tag}")


def report(entry):
    for k, v in WORST.get(entry, {}).items():
        print(f"ratio gpu {entry} {k} {v:.3f}")


def _i32(*v):
    return _d(torch.tensor(v, dtype=torch.int32, device="cuda"))


def _pack(ts, need=None):
    """Per-net tensors -> one flat NaN-filled tensor at net stride need + GAP -> (flat, stride)."""
    need = need or ts[0].numel()
    stride = need + GAP
    flat = torch.full((len(ts) * stride,), NAN)
    for i, t in enumerate(ts):
        flat[i * stride:i * stride + t.numel()] = t.reshape(-1)
    return flat, stride


def _unpack(flat, nets, stride, shape, prefill=None, tag=""):
    """The nets' blocks of an output, after checking that the gaps still hold their pre-fill (NaN, or ``prefill``'s)."""
    flat = flat.detach().cpu().view(nets, stride)
    n = 1
    for s in shape:
        n *= s
    want = torch.full((nets, stride - n), NAN) if prefill is None else prefill.view(nets, stride)[:, n:]
    assert_same(flat[:, n:], want, f"{tag}: the gap between the nets was written")
    return [flat[i, :n].view(*shape).clone() for i in range(nets)]


def _both(run, data):
    """The nets = 3 launch, and the nets = 1 launch on net 1's data: net 1 bit-equal between them."""
    three, one = run(data), run(data[1:2])
    for k in three[1]:
        if three[1][k] is not None:
            assert_same(three[1][k], one[0][k], f"net 1 of three vs alone: {k}")
    return three


def test_header_constants():
    _, C, _ = _m()
    assert (C.NIN, C.KP, C.HID, C.G3, C.P, C.OFF_FCW, C.OFF_FCB) == (NIN, R.KP, HID, G3, P, OFF_FCW, OFF_FCB)


# ================================================================================================ vunet_seq_cls_gather
@pytest.mark.parametrize("T,n,ld", R.GATHER_SHAPES)
@pytest.mark.parametrize("bs", R.GATHER_BS)
def test_cls_gather_bit_exact(T, n, ld, bs):
    """dst[g][t][r][k] = set[b bs + r % bs][t][k], b = *it_dev % 3 for *it_dev = 0, 2, 3, 10 (the wrap), fake rows then real rows;
    columns n .. ld are 0; without a real set its table entry is NULL."""
    ops, _, _ = _m()
    nb = R.GATHER_NB
    for with_real in (0, 1):
        data = [R.make_gather(T, n, bs, with_real, 10 * bs + s) for s in range(3)]
        total = T * (2 if with_real else 1) * bs * ld
        assert total % 256
        for it in R.GATHER_ITS:
            def run(ds):
                dev = [(_d(d["fake"]), _d(d["real"])) for d in ds]
                tab = torch.tensor([0 if t is None else t.data_ptr() for pair in dev for t in pair], dtype=torch.int64, device="cuda")
                o = Outs()
                dst = o.new(len(ds) * (total + GAP))
                ops._call("vunet_seq_cls_gather", ops._p(tab), len(ds), T, n, ld, bs, nb, with_real, ops._p(_i32(it)), ops._p(dst),
                          total + GAP, ops._stream())
                o.check()
                return [dict(dst=t) for t in _unpack(dst, len(ds), total + GAP, (T, total // (T * ld), ld), tag="gather")]
            for d, got in zip(data, _both(run, data)):
                assert_same(got["dst"], R.ref_gather(d["fake"], d["real"], T, n, ld, bs, nb, it)["dst"][0], f"gather it {it} real {with_real}")


def test_cls_gather_refusals():
    ops, _, _ = _m()
    buf = torch.zeros(4096, device="cuda")
    tab = torch.tensor([buf.data_ptr(), 0], dtype=torch.int64, device="cuda")
    p, it, st = ops._p(buf), ops._p(_i32(0)), ops._stream()
    _refused(ops, ERR_ARG, "vunet_seq_cls_gather", ops._p(tab), 1, 1, 8, 7, 2, 1, 0, it, p, 4096, st)            # ld < n
    _refused(ops, ERR_ARG, "vunet_seq_cls_gather", ops._p(tab), 1, 2, 8, 8, 2, 1, 0, it, p, 2 * 2 * 8 - 1, st)   # dst_net < total


# ================================================================================================ vunet_seq_cls_cell_fwd
@pytest.mark.parametrize("Rr", R.CELL_ROWS)
@pytest.mark.parametrize("scale", R.CELL_SCALES)
def test_cls_cell_fwd_vs_float64(Rr, scale):
    """gates[t] and h[t + 1] of step t in {0, 2} of T = 3 within the bound, with gi / gh at scale 1 and at scale 8 (saturated
    gates) and a random h[t]; every other step of gates and h keeps its pre-fill bit for bit."""
    ops, _, _ = _m()
    T = R.CELL_T
    data = [R.make_cell_fwd(Rr, scale, 100 + s) for s in range(3)]
    ng, nh = T * Rr * G3, (T + 1) * Rr * HID
    for t in R.CELL_STEPS:
        def run(ds):
            gi, gi_net = _pack([d["gi"] for d in ds])
            gh, _ = _pack([d["gh"] for d in ds])
            h0, h_net = _pack([d["h"] for d in ds])
            o = Outs()
            gates, h = o.new(len(ds) * gi_net), o.load(_d(h0))
            ops._call("vunet_seq_cls_cell_fwd", ops._p(_d(gi)), ops._p(_d(gh)), ops._p(gates), ops._p(h), len(ds), T, Rr, t, gi_net, h_net,
                      ops._stream())
            o.check()
            return [dict(gates=a, h=b) for a, b in zip(_unpack(gates, len(ds), gi_net, (T, Rr, G3), tag="gates"),
                                                       _unpack(h, len(ds), h_net, (T + 1, Rr, HID), prefill=h0, tag="h"))]
        for d, got in zip(data, _both(run, data)):
            ref = R.ref_cell_fwd(d["gi"][t], d["gh"][t], d["h"][t])
            tag = f"R {Rr} scale {scale} t {t}"
            held("vunet_seq_cls_cell_fwd", "gates", got["gates"][t], ref["gates"], tag)
            held("vunet_seq_cls_cell_fwd", "h", got["h"][t + 1], ref["h"], tag)
            others = [q for q in range(T) if q != t]
            assert_same(got["gates"][others], torch.full((T - 1, Rr, G3), NAN), f"{tag}: gates of another step written")
            keep = [q for q in range(T + 1) if q != t + 1]
            assert_same(got["h"][keep], d["h"][keep], f"{tag}: h of another step written")
    report("vunet_seq_cls_cell_fwd")


def test_cls_cell_fwd_refusals():
    ops, _, _ = _m()
    buf = torch.zeros(1 << 14, device="cuda")
    p, st = ops._p(buf), ops._stream()
    _refused(ops, ERR_ARG, "vunet_seq_cls_cell_fwd", p, p, p, p, 1, 2, 1, 2, 2 * G3, 3 * HID, st)          # t == T
    _refused(ops, ERR_ARG, "vunet_seq_cls_cell_fwd", p, p, p, p, 1, 2, 1, 0, 2 * G3, 3 * HID - 1, st)      # h_net one short


# ================================================================================================ vunet_seq_cls_cell_bwd
@pytest.mark.parametrize("Rr", R.CELL_ROWS)
def test_cls_cell_bwd_vs_float64(Rr):
    """Step t in {0, 2} of T = 3 from gates constructed in (0, 1) and (-1, 1), some within 2 U of the ends: dgi[t] over gi[t] and
    dgh[t] over gh[t] within the bound (da_r needs the forward's gh_n, which the same launch overwrites: read first), dh_prev
    bit-equal to the fp32 product dh z, every other step of gi / gh bit-equal to what it held."""
    ops, _, _ = _m()
    T = R.CELL_T
    data = [R.make_cell_bwd(Rr, 200 + s) for s in range(3)]
    for t in R.CELL_STEPS:
        def run(ds):
            gi0, gi_net = _pack([d["gi"] for d in ds])
            gh0, _ = _pack([d["gh"] for d in ds])
            gates, _ = _pack([d["gates"] for d in ds])
            h, h_net = _pack([d["h"] for d in ds])
            dh, dh_net = _pack([d["dh"] for d in ds])
            o = Outs()
            gi, gh, dhp = o.load(_d(gi0)), o.load(_d(gh0)), o.new(len(ds) * dh_net)
            ops._call("vunet_seq_cls_cell_bwd", ops._p(gi), ops._p(gh), ops._p(_d(gates)), ops._p(_d(h)), ops._p(_d(dh)), ops._p(dhp),
                      len(ds), T, Rr, t, gi_net, h_net, dh_net, ops._stream())
            o.check()
            return [dict(gi=a, gh=b, dh_prev=c) for a, b, c in zip(_unpack(gi, len(ds), gi_net, (T, Rr, G3), prefill=gi0, tag="gi"),
                                                                   _unpack(gh, len(ds), gi_net, (T, Rr, G3), prefill=gh0, tag="gh"),
                                                                   _unpack(dhp, len(ds), dh_net, (Rr, HID), tag="dh_prev"))]
        for d, got in zip(data, _both(run, data)):
            ref = R.ref_cell_bwd(d["gates"][t], d["gh"][t][:, 2 * HID:], d["h"][t], d["dh"])
            tag = f"R {Rr} t {t}"
            held("vunet_seq_cls_cell_bwd", "gi", got["gi"][t], ref["gi"], tag)
            held("vunet_seq_cls_cell_bwd", "gh", got["gh"][t], ref["gh"], tag)
            assert_same(got["dh_prev"], d["dh"] * d["gates"][t][:, HID:2 * HID], f"{tag}: dh_prev")
            others = [q for q in range(T) if q != t]
            assert_same(got["gi"][others], d["gi"][others], f"{tag}: gi of another step written")
            assert_same(got["gh"][others], d["gh"][others], f"{tag}: gh of another step written")
    report("vunet_seq_cls_cell_bwd")


# ================================================================================================ vunet_seq_cls_head
@pytest.mark.parametrize("bs", R.HEAD_BS)
def test_cls_head_vs_float64(bs):
    """bs 1 .. 1024 (a thread owns several rows from 257 on) x {real rows and dh, real rows without dh, fake rows alone with
    loss_out NULL} x h_T at scale 1 and at the scale that spreads the logits over about +-30, row 0's logit exactly 0:
    loss, acc at slot *it_dev + slot_off = 7 of 11 (every other slot keeps its NaN), dh, grad[OFF_FCW .. OFF_FCB]; the rest of
    the grad block untouched.  The parameter block is NaN outside fc1."""
    ops, _, _ = _m()
    slot, ldc = R.HEAD_IT + R.HEAD_SLOT_OFF, R.HEAD_LD_CURVE
    for scale in R.HEAD_SCALES:
        for with_real, with_dh in ((1, True), (1, False), (0, False)):
            Rr = 2 * bs if with_real else bs
            data = [R.make_head(bs, with_real, scale, 300 + s) for s in range(3)]

            def run(ds):
                nets = len(ds)
                params = torch.full((nets, P), NAN)
                for i, d in enumerate(ds):
                    params[i, OFF_FCW:OFF_FCB], params[i, OFF_FCB] = d["w"], d["fb"]
                hT, h_net = _pack([d["hT"] for d in ds])
                o = Outs()
                loss, acc = (o.new(nets, ldc) if with_real else None), o.new(nets, ldc)
                dh, grad = (o.new(nets, Rr, HID), o.new(nets * (P + GAP))) if with_dh else (None, None)
                ops._call("vunet_seq_cls_head", ops._p(_d(hT)), h_net, ops._p(_d(params)), nets, bs, with_real, ops._p(_i32(R.HEAD_IT)),
                          R.HEAD_SLOT_OFF, ops._p(loss), ops._p(acc), ldc, ops._p(dh), ops._p(grad), P + GAP, ops._stream())
                o.check()
                gr = _unpack(grad, nets, P + GAP, (P,), tag="grad") if with_dh else [None] * nets
                return [dict(loss=None if loss is None else loss[i].cpu(), acc=acc[i].cpu(), dh=None if dh is None else dh[i].cpu(),
                             grad=gr[i]) for i in range(nets)]
            for d, got in zip(data, _both(run, data)):
                ref = R.ref_head(d["hT"], d["w"], d["fb"], bs, with_real)
                tag = f"bs {bs} scale {scale} real {with_real} dh {with_dh}"
                keep = [q for q in range(ldc) if q != slot]
                held("vunet_seq_cls_head", "acc", got["acc"][slot], ref["acc"], tag)
                assert torch.isnan(got["acc"][keep]).all(), f"{tag}: another slot of acc written"
                if with_real:
                    held("vunet_seq_cls_head", "loss", got["loss"][slot], ref["loss"], tag)
                    assert torch.isnan(got["loss"][keep]).all(), f"{tag}: another slot of loss written"
                if with_dh:
                    held("vunet_seq_cls_head", "dh", got["dh"], ref["dh"], tag)
                    held("vunet_seq_cls_head", "gw", got["grad"][OFF_FCW:OFF_FCB], ref["gw"], tag)
                    held("vunet_seq_cls_head", "gb", got["grad"][OFF_FCB], ref["gb"], tag)
                    assert torch.isnan(got["grad"][:OFF_FCW]).all() and torch.isnan(got["grad"][OFF_FCB + 1:]).all(), \
                        f"{tag}: grad written outside fc1"
    report("vunet_seq_cls_head")


def test_cls_head_refusals():
    ops, _, _ = _m()
    buf = torch.zeros(P + 1026 * HID, device="cuda")
    p, it, st = ops._p(buf), ops._p(_i32(0)), ops._stream()
    _refused(ops, ERR_ARG, "vunet_seq_cls_head", p, 1025 * HID, p, 1, 1025, 0, it, 0, None, p, 4, None, None, 0, st)   # bs = 1025
    _refused(ops, ERR_ARG, "vunet_seq_cls_head", p, 4 * HID, p, 1, 4, 0, it, 0, p, p, 4, p, p, P, st)                 # dh without real rows


# ================================================================================================ vunet_seq_cls_sgd
@pytest.mark.parametrize("S", R.SGD_S)
@pytest.mark.parametrize("it", R.SGD_ITS)
def test_cls_sgd_bit_exact_and_vs_float64(S, it):
    """Bit-equal to the fp32 restatement in the kernel's order (it pins its roundings; slices added in slice order) and within the
    float64 bound of torch.optim.SGD.  At iteration 0 the buffer is NaN and must be ignored; the fc range of slices >= 1 is NaN
    (read from slice 0 only)."""
    ops, _, _ = _m()
    data = [R.make_sgd(S, it, 400 + s) for s in range(3)]

    def run(ds):
        o = Outs()
        params, buf = o.load(_d(torch.stack([d["params"] for d in ds]))), o.load(_d(torch.stack([d["buf"] for d in ds])))
        ops._call("vunet_seq_cls_sgd", ops._p(params), ops._p(_d(torch.stack([d["grad"] for d in ds]))), ops._p(buf), len(ds), S,
                  R.SGD_LR, R.SGD_MOM, ops._p(_i32(it)), ops._stream())
        o.check()
        return [dict(params=params[i].cpu(), buf=buf[i].cpu()) for i in range(len(ds))]
    for d, got in zip(data, _both(run, data)):
        p32, b32 = R.sgd_fp32(d["params"], d["grad"], d["buf"], it)
        assert_same(got["params"], p32, f"sgd S {S} it {it}: params")
        assert_same(got["buf"], b32, f"sgd S {S} it {it}: buf")
        ref = R.ref_sgd(d["params"], d["grad"], d["buf"], it)
        held("vunet_seq_cls_sgd", "params", got["params"], ref["params"], f"S {S} it {it}")
        held("vunet_seq_cls_sgd", "buf", got["buf"], ref["buf"], f"S {S} it {it}")
    report("vunet_seq_cls_sgd")


# ================================================================================================ vunet_seq_cls_reg_loss
@pytest.mark.parametrize("bs", R.CRL_BS)
@pytest.mark.parametrize("ldp", R.CRL_LDP)
def test_cls_reg_loss_vs_float64(bs, ldp):
    """bs 1 / 37 / 257 (a thread owns two rows), ldp 51 / 64, batch *it_dev % nb = 4 % 3, a start per net (0, T - 1, 1), xc NULL and
    given: loss (and de) at slot 6 of 11, dpred within the bound; the row with pred == target gives a dpred row of 0 and no NaN;
    columns 51 .. ldp of dpred keep their pre-fill."""
    ops, _, _ = _m()
    slot, ldc = R.CRL_IT + 2, 11
    for with_xc in (False, True):
        xo, xc = R.make_cls_reg_sets(bs, with_xc, 500)
        data = [R.make_cls_reg_loss(xo, xc, bs, ldp, R.CRL_STARTS[s], 500 + s) for s in range(3)]
        starts = {id(d): R.CRL_STARTS[s] for s, d in enumerate(data)}

        def run(ds):
            nets = len(ds)
            pred, pred_net = _pack([d["pred"] for d in ds])
            o = Outs()
            loss, de, dpred = o.new(nets, ldc), o.new(nets, ldc), o.new(nets * pred_net)
            ops._call("vunet_seq_cls_reg_loss", ops._p(_d(pred)), ldp, pred_net, ops._p(_d(xo)), ops._p(_d(xc)), R.CRL_T, bs, R.CRL_NB,
                      ops._p(_i32(*[starts[id(d)] for d in ds])), ops._p(_i32(R.CRL_IT)), 2, ops._p(loss), ops._p(de), ldc, ops._p(dpred),
                      nets, ops._stream())
            o.check()
            return [dict(loss=loss[i].cpu(), de=de[i].cpu(), dpred=t) for i, t in enumerate(_unpack(dpred, nets, pred_net, (bs, ldp), tag="dpred"))]
        for d, got in zip(data, _both(run, data)):
            ref = R.ref_cls_reg_loss(d["pred"], xo, xc, bs, R.CRL_NB, R.CRL_IT, starts[id(d)])
            tag = f"bs {bs} ldp {ldp} xc {with_xc} start {starts[id(d)]}"
            keep = [q for q in range(ldc) if q != slot]
            held("vunet_seq_cls_reg_loss", "loss", got["loss"][slot], ref["loss"], tag)
            held("vunet_seq_cls_reg_loss", "dpred", got["dpred"][:, :NIN], ref["dpred"], tag)
            assert_same(got["dpred"][bs // 2, :NIN], torch.zeros(NIN), f"{tag}: the row at its target")
            assert torch.isnan(got["dpred"][:, NIN:]).all(), f"{tag}: dpred written beyond column 51"
            assert torch.isnan(got["loss"][keep]).all(), f"{tag}: another slot of loss written"
            if with_xc:
                held("vunet_seq_cls_reg_loss", "de", got["de"][slot], ref["de"], tag)
                assert torch.isnan(got["de"][keep]).all(), f"{tag}: another slot of de written"
            else:
                assert torch.isnan(got["de"]).all(), f"{tag}: de written without xc"
    report("vunet_seq_cls_reg_loss")


def test_cls_reg_loss_refusals():
    ops, _, _ = _m()
    buf = torch.zeros(4096, device="cuda")
    p, z, st = ops._p(buf), ops._p(_i32(0)), ops._stream()
    _refused(ops, ERR_ARG, "vunet_seq_cls_reg_loss", p, 50, 2 * 50, p, None, 2, 2, 1, z, z, 0, p, None, 4, p, 1, st)   # ldp = 50


# ================================================================================================ vunet_seq_cls_adam / _tick
@pytest.mark.parametrize("n", R.ADAM_N)
@pytest.mark.parametrize("step", R.ADAM_STEPS)
def test_cls_adam_vs_float64(n, step):
    """torch.optim.Adam (defaults but lr) on n = 1 / 300 floats per net at step 1 / 1000, some elements with g = 0 and v = 0,
    resolved_dev NULL (the kernel forms the bias corrections itself); then once more with the constants vunet_seq_adam_tick
    resolves, which is printed as bit-equal to the first or not."""
    ops, _, T = _m()
    data = [R.make_adam(n, 600 + s) for s in range(3)]
    lr, b1, b2, eps = R.ADAM_LR, R.ADAM_B1, R.ADAM_B2, R.ADAM_EPS
    res = {}
    for ticked in (False, True):
        def run(ds):
            o = Outs()
            p, m, v = (o.load(_d(torch.stack([d[k] for d in ds]))) for k in ("p", "m", "v"))
            hp, keep = _adam_hp(T, lr, step - 1 if ticked else step, b1, b2, eps, 0.0, resolved=ticked)
            if ticked:
                ops._call("vunet_seq_adam_tick", ops._p(keep[1]), ops._p(keep[0]), b1, b2, ops._p(keep[2]), ops._stream())
            ops._call("vunet_seq_cls_adam", ops._p(p), ops._p(m), ops._p(v), ops._p(_d(torch.stack([d["g"] for d in ds]))), len(ds), n,
                      ctypes.byref(hp), ops._stream())
            o.check()
            c = tuple(float(x) for x in keep[2].cpu().double()) if ticked else None
            return [dict(p=p[i].cpu(), m=m[i].cpu(), v=v[i].cpu(), c=c) for i in range(len(ds))]
        three, one = run(data), run(data[1:2])
        for k in ("p", "m", "v"):
            assert_same(three[1][k], one[0][k], f"net 1 of three vs alone: {k}")
        res[ticked] = three
        for d, got in zip(data, three):
            c = got["c"] or R.adam_constants(lr, step, b1, b2)
            ref = R.ref_adam(d["p"], d["m"], d["v"], d["g"], *c, b1, b2, eps, own_constants=not ticked)
            for k in ("p", "m", "v"):
                held("vunet_seq_cls_adam", k, got[k], ref[k], f"n {n} step {step} ticked {ticked}")
    same = all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for a, b in zip(res[False], res[True]) for k in ("p", "m", "v"))
    print(f"note gpu vunet_seq_cls_adam n {n} step {step}: own constants vs vunet_seq_adam_tick's: {'bit-equal' if same else 'differ'}")
    report("vunet_seq_cls_adam")


def test_cls_adam_refusals():
    ops, _, T = _m()
    buf = torch.zeros(64, device="cuda")
    p, st = ops._p(buf), ops._stream()
    _, keep = _adam_hp(T, 1e-3, 1, 0.9, 0.999, 1e-8, 0.0, resolved=False)
    nolr = T.SeqAdamHp(None, keep[1].data_ptr(), 0.9, 0.999, 1e-8, 0.0, None)
    _refused(ops, ERR_ARG, "vunet_seq_cls_adam", p, p, p, p, 1, 8, ctypes.byref(nolr), st)
    for b1, b2, eps in ((1.0, 0.999, 1e-8), (0.9, 1.0, 1e-8), (0.9, 0.999, -1e-8)):
        bad, keep2 = _adam_hp(T, 1e-3, 1, b1, b2, eps, 0.0, resolved=False)
        _refused(ops, ERR_ARG, "vunet_seq_cls_adam", p, p, p, p, 1, 8, ctypes.byref(bad), st)


def test_cls_tick_exact():
    """Each counter alone, then both."""
    ops, _, _ = _m()
    o = Outs()
    it = o.load(torch.tensor([41], dtype=torch.int32, device="cuda"))
    step = o.load(torch.tensor([(1 << 40) + 5], dtype=torch.int64, device="cuda"))
    ops._call("vunet_seq_cls_tick", ops._p(it), None, ops._stream())
    o.check()
    assert (int(it.item()), int(step.item())) == (42, (1 << 40) + 5)
    ops._call("vunet_seq_cls_tick", None, ops._p(step), ops._stream())
    o.check()
    assert (int(it.item()), int(step.item())) == (42, (1 << 40) + 6)
    ops._call("vunet_seq_cls_tick", ops._p(it), ops._p(step), ops._stream())
    o.check()
    assert (int(it.item()), int(step.item())) == (43, (1 << 40) + 7)


# ================================================================================================ vunet_seq_reg_gather
@pytest.mark.parametrize("B", R.RG_B)
def test_reg_gather_bit_exact(B):
    """B 1 .. 64 x H4 4 / 300 x n 3 / 51, seq rows 50 n + 3 apart, idx_dev = {0, 49, -1, 50, 17} read at each k (the two out of
    range are clamped): the copies bit-exact, the fc4 column bit-equal to fp32 max(w + b, 0) and within U of float64, tgt rows
    B .. Bp exactly 0, cat rows B .. Bp carrying h3's padding rows (their NaN too)."""
    ops, _, _ = _m()
    Bp = _up16(B)
    for H4 in R.RG_H4:
        for n in R.RG_N:
            d = R.make_reg_gather(B, H4, n, 700 + B)
            dev = {k: _d(d[k]) for k in ("w4", "b4", "h3", "seq")}
            idx = _i32(*R.RG_IDX)
            for k in range(5):
                o = Outs()
                cat, tgt = o.new(Bp, H4 + REG_C), o.new(Bp, n)
                ops._call("vunet_seq_reg_gather", ops._p(dev["w4"]), ops._p(dev["b4"]), ops._p(idx), k, ops._p(dev["h3"]), ops._p(dev["seq"]),
                          REG_T * n + 3, n, B, H4, ops._p(cat), ops._p(tgt), ops._stream())
                o.check()
                ref = R.ref_reg_gather(d["w4"], d["b4"], d["h3"], d["seq"], R.RG_IDX[k], n, B)
                tag = f"B {B} H4 {H4} n {n} k {k}"
                cat = cat.cpu()
                assert_same(cat[:, :H4], d["h3"], f"{tag}: h3 part of cat")
                col = torch.clamp_min(d["w4"][:, min(max(R.RG_IDX[k], 0), REG_T - 1)] + d["b4"], 0.0)
                assert_same(cat[:, H4:], col[None, :].expand(Bp, REG_C), f"{tag}: fc4 part of cat")
                held("vunet_seq_reg_gather", "fc4", cat[0, H4:], ref["fc4"], tag)
                assert_same(tgt, ref["tgt"][0], f"{tag}: tgt")
    report("vunet_seq_reg_gather")


def test_reg_gather_refusals():
    ops, _, _ = _m()
    buf = torch.zeros(1 << 15, device="cuda")
    p, i, st = ops._p(buf), ops._p(_i32(0, 0, 0, 0, 0, 0)), ops._stream()
    _refused(ops, ERR_ARG, "vunet_seq_reg_gather", p, p, i, 5, p, p, 150, 3, 4, 4, p, p, st)      # k = 5
    _refused(ops, ERR_ARG, "vunet_seq_reg_gather", p, p, i, 0, p, p, 150, 3, 65, 4, p, p, st)     # B = 65
    _refused(ops, ERR_ARG, "vunet_seq_reg_gather", p, p, i, 0, p, p, 149, 3, 4, 4, p, p, st)      # seq_stride < 50 n


# ================================================================================================ vunet_seq_reg_loss
@pytest.mark.parametrize("B", R.RL_B)
@pytest.mark.parametrize("n", R.RL_N)
def test_reg_loss_vs_float64(B, n):
    """ldp = 64 with pred's padding rows and columns NaN (dpred there exactly 0): reg[k] = L within the bound, the other slots of
    reg NaN.  With scalars (k = 4), pred scaled so that L is about 0.3, 0.55 and 0.9 -- further from 0.45 and 0.7 than its bound --
    reg[5] is exactly -2 w, -w, 0 and scalars[0] within the bound."""
    ops, _, _ = _m()
    Bp, ldp, w = _up16(B), R.RL_LDP, R.RL_W
    for tL in R.RL_TARGETS:
        d = R.make_reg_loss(B, n, tL, 800 + B + n)
        k = 1 if tL is None else 4
        o = Outs()
        reg, dpred = o.new(6), o.new(Bp, ldp)
        scal = None if tL is None else o.load(torch.tensor([R.RL_S0, NAN, NAN, NAN], device="cuda"))
        ops._call("vunet_seq_reg_loss", ops._p(_d(d["pred"])), ldp, ops._p(_d(d["tgt"])), B, n, k, w, ops._p(reg), ops._p(dpred), ops._p(scal),
                  ops._stream())
        o.check()
        ref = R.ref_reg_loss(d["pred"], d["tgt"], B, n, ldp, w, None if tL is None else R.RL_S0)
        tag = f"B {B} n {n} L {tL}"
        reg, dpred = reg.cpu(), dpred.cpu()
        held("vunet_seq_reg_loss", "L", reg[k], ref["L"], tag)
        held("vunet_seq_reg_loss", "dpred", dpred, ref["dpred"], tag)
        assert_same(dpred[B:], torch.zeros(Bp - B, ldp), f"{tag}: dpred on padding rows")
        assert_same(dpred[:, n:], torch.zeros(Bp, ldp - n), f"{tag}: dpred on padding columns")
        written = {k} if tL is None else {k, 5}
        assert torch.isnan(reg[[q for q in range(6) if q not in written]]).all(), f"{tag}: another slot of reg written"
        if tL is not None:
            L, dL = float(ref["L"][0]), float(ref["L"][1])
            assert min(abs(L - R.CLAMP_LO), abs(L - R.CLAMP_HI)) > dL
            assert float(reg[5]) == float(ref["reg5"][0]) == -float(torch.tensor(w)) * {0.3: 2, 0.55: 1, 0.9: 0}[tL], tag
            held("vunet_seq_reg_loss", "loss", scal[0], ref["loss"], tag)
            assert torch.isnan(scal[1:]).all(), f"{tag}: scalars beyond [0] written"
    report("vunet_seq_reg_loss")


def test_reg_loss_refusals():
    ops, _, _ = _m()
    buf = torch.zeros(4096, device="cuda")
    p, st = ops._p(buf), ops._stream()
    _refused(ops, ERR_ARG, "vunet_seq_reg_loss", p, 50, p, 4, 51, 0, 0.5, p, p, None, st)         # ldp < n


# ================================================================================================ vunet_seq_reg_cat_bwd
@pytest.mark.parametrize("S", R.CB_S)
@pytest.mark.parametrize("Bp", R.CB_BP)
def test_reg_cat_bwd_bit_exact(S, Bp):
    """The slabs added in slab order, times the mask [cat > 0] (cat holds +0, -0, positive and negative values), split at H4 = 4 /
    256, with dzc given and NULL: bit-equal to the fp32 restatement, and within (S - 1) U sum|raw| of float64."""
    ops, _, _ = _m()
    for H4 in R.CB_H4:
        d = R.make_cat_bwd(S, Bp, H4, 900 + S)
        want3, wantc = R.cat_bwd_fp32(d["raw"], d["cat"], H4)
        ref = R.ref_cat_bwd(d["raw"], d["cat"], H4)
        for with_c in (True, False):
            o = Outs()
            dz3, dzc = o.new(Bp, H4), (o.new(Bp, REG_C) if with_c else None)
            ops._call("vunet_seq_reg_cat_bwd", ops._p(_d(d["raw"])), S, Bp, H4, ops._p(_d(d["cat"])), ops._p(dz3), ops._p(dzc), ops._stream())
            o.check()
            assert_same(dz3, want3, f"S {S} Bp {Bp} H4 {H4}: dz3")
            held("vunet_seq_reg_cat_bwd", "dz3", dz3, ref["dz3"], f"S {S} Bp {Bp} H4 {H4}")
            if with_c:
                assert_same(dzc, wantc, f"S {S} Bp {Bp} H4 {H4}: dzc")
                held("vunet_seq_reg_cat_bwd", "dzc", dzc, ref["dzc"], f"S {S} Bp {Bp} H4 {H4}")
    report("vunet_seq_reg_cat_bwd")


def test_reg_cat_bwd_refusals():
    ops, _, _ = _m()
    buf = torch.zeros(1 << 15, device="cuda")
    p, st = ops._p(buf), ops._stream()
    for Bp in (8, 24, 80):
        _refused(ops, ERR_ARG, "vunet_seq_reg_cat_bwd", p, 1, Bp, 4, p, p, p, st)


# ================================================================================================ vunet_seq_reg_fc4_adam
def _fc4_adam_case(ops, T, Bp, step, ks):
    d = R.make_fc4_adam(Bp, 1000 + Bp)
    names = ("w4", "b4", "m4", "v4", "bm4", "bv4")
    for k in ks:
        hp, keep = _adam_hp(T, R.FA_LR, step - 1, R.FA_B1, R.FA_B2, R.FA_EPS, 0.0)
        ops._call("vunet_seq_adam_tick", ops._p(keep[1]), ops._p(keep[0]), R.FA_B1, R.FA_B2, ops._p(keep[2]), ops._stream())
        o = Outs()
        st = {q: o.load(_d(d[q])) for q in names}
        ops._call("vunet_seq_reg_fc4_adam", ops._p(_d(d["dzc"])), Bp, ops._p(_i32(*R.FA_IDX)), k, *(ops._p(st[q]) for q in names),
                  ctypes.byref(hp), ops._stream())
        o.check()
        c = tuple(float(x) for x in keep[2].cpu().double())
        ref = R.ref_fc4_adam(d["dzc"], *(d[q] for q in names), R.FA_IDX[k], *c, R.FA_B1, R.FA_B2, R.FA_EPS)
        col = min(max(R.FA_IDX[k], 0), REG_T - 1)
        others = [j for j in range(REG_T) if j != col]
        for q in names:
            held("vunet_seq_reg_fc4_adam", q, st[q], ref[q], f"Bp {Bp} step {step} idx {R.FA_IDX[k]}")
        # the untouched columns move as Adam moves them, by their moments alone (an update below half an ulp of the weight
        # leaves it: a few of the 6272 do not move)
        assert float((st["w4"].cpu()[:, others] != d["w4"][:, others]).float().mean()) > 0.9
        assert_same(st["m4"].cpu()[:, others], (torch.tensor(R.FA_B1) * d["m4"])[:, others], "m4 of the untouched columns: b1 m")


@pytest.mark.parametrize("Bp", R.FA_BP)
@pytest.mark.parametrize("step", R.FA_STEPS)
def test_reg_fc4_adam_vs_float64(Bp, step):
    """Moments pre-loaded non-zero, step 1 / 7 (constants from vunet_seq_adam_tick), idx 0, 49 and 23: w4, b4 and the four moments
    against float64 Adam on the dense gradient (one non-zero column, g = the batch sum, 6 U sum|dzc| for the butterfly; the bias
    takes g itself); the other 49 columns move by their moments alone."""
    ops, _, T = _m()
    _fc4_adam_case(ops, T, Bp, step, (0, 1, 4))
    report("vunet_seq_reg_fc4_adam")


@pytest.mark.parametrize("k", [2, 3])
def test_reg_fc4_adam_clamps_an_index_out_of_range(k):
    """idx -3 and 50 update column 0 and 49: the column vunet_seq_reg_gather read for them."""
    ops, _, T = _m()
    _fc4_adam_case(ops, T, 16, 7, (k,))
    report("vunet_seq_reg_fc4_adam")


# ================================================================================================ vunet_seq_reg_adv
@pytest.mark.parametrize("B,H", R.ADV_SHAPES)
@pytest.mark.parametrize("S", R.ADV_S)
def test_reg_adv_vs_float64(B, H, S):
    """gmu[b][j] += reg[5] sum_s raw[s][b][j] onto a pre-loaded gmu, adv given and NULL, within a bound that admits the contracted
    form; raw's padding rows and reg[0 .. 4] are NaN (not read); gmu's rows >= B keep what they held."""
    ops, _, _ = _m()
    Bp = _up16(B)
    d = R.make_adv(B, H, S, 1100 + S)
    ref = R.ref_adv(d["raw"], d["reg"], d["gmu"], B)
    for with_adv in (True, False):
        o = Outs()
        gmu, adv = o.load(_d(d["gmu"])), (o.new(B, H) if with_adv else None)
        ops._call("vunet_seq_reg_adv", ops._p(_d(d["raw"])), S, B, H, ops._p(_d(d["reg"])), ops._p(gmu), ops._p(adv), ops._stream())
        o.check()
        tag = f"B {B} H {H} S {S} adv {with_adv}"
        held("vunet_seq_reg_adv", "gmu", gmu[:B], ref["gmu"], tag)
        assert_same(gmu[B:], d["gmu"][B:], f"{tag}: gmu rows >= B")
        if with_adv:
            held("vunet_seq_reg_adv", "adv", adv, ref["adv"], tag)
    assert Bp >= B
    report("vunet_seq_reg_adv")
