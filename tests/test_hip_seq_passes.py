"""Several training passes of the behaviour net / the flow alive at once under autograd (``seq_train``'s pass slots): what the
reference's unchanged ``train_fn`` (experiments/behavior_net.py:611-686) does per iteration -- three calls of one shape, the
backward of the first after the second's forward, the third's backward after the optimiser's step -- against the reference's own
run (tests/golden/g18_cvae_iteration.npz), and the properties behind it: any backward order, repeated backward, the encoder-only
backward, stale weights refused, the cap on live passes.  Expected gradients of the interleaved cases: the same pass run alone on
a fresh copy of the module -- the kernels sum in a fixed order, so "the same" means bit for bit."""
import gc

import pytest
import torch

import test_hip_seq_train as S          # its helpers: the measures of g11's tests are the measures here
from conftest import load_golden
from synth import seeded_randn, synth_behavior_state

pytestmark = pytest.mark.gpu

N_KPS = 51
NET_SHAPES = [(1, 64, 3), (17, 128, 5), (64, 64, 4)]          # rows, hidden, T; 64 rows: h goes from step to step as tiles (``ht``)
FLOW = dict(chan=32, mid=64, depth=2, n_flows=3)
FLOW_ROWS = [1, 17, 64]


# ------------------------------------------------------------------------------------------------ the behaviour net
def _net(hid, seed=9):
    from behavior_driven_video_synthesis_amd.models.pose_behavior_rnn import ResidualBehaviorNet
    net = ResidualBehaviorNet(N_KPS, information_bottleneck=True, decoder_arch="lstm", dim_hidden_b=hid)
    net.load_state_dict(synth_behavior_state({k: list(v.shape) for k, v in net.state_dict().items()}, seed, {}))
    return net.cuda().train()


def _inputs(tag, rows, hid, t):
    """One pass's sequences, noise and the weights of a loss that reaches every output."""
    d = dict(x1=0.5 * seeded_randn(f"ps.{tag}.x1", (rows, t, N_KPS), 9), x2=0.5 * seeded_randn(f"ps.{tag}.x2", (rows, t, N_KPS), 9),
             eps=seeded_randn(f"ps.{tag}.eps", (rows, hid), 9))
    for k, shp in dict(xs=(rows, t, N_KPS), cs=(rows, t, N_KPS), b=(rows, hid), mu=(rows, hid), logstd=(rows, hid), pre=(rows, hid)).items():
        d["w." + k] = seeded_randn(f"ps.{tag}.w.{k}", shp, 9)
    return {k: v.cuda() for k, v in d.items()}


def _forward(net, inp):
    xs, cs, _, b, mu, logstd, pre = net(inp["x1"], inp["x2"], inp["x1"].shape[1], eps=inp["eps"])
    return dict(xs=xs, cs=cs, b=b, mu=mu, logstd=logstd, pre=pre)


def _loss(out, inp, keys=("xs", "cs", "b", "mu", "logstd", "pre")):
    return sum((out[k] * inp["w." + k]).sum() for k in keys)


def _grads(net, loss, **kw):
    names = [n for n, _ in net.named_parameters()]
    return dict(zip(names, torch.autograd.grad(loss, list(net.parameters()), **kw)))


_ALONE = {}


def _alone(tag, rows, hid, t, keys=("xs", "cs", "b", "mu", "logstd", "pre")):
    """The gradients of pass ``tag`` run alone on a fresh copy of the net: computed once, shared, never written to."""
    key = (tag, rows, hid, t, keys)
    if key not in _ALONE:
        net, inp = _net(hid), _inputs(tag, rows, hid, t)
        _ALONE[key] = _grads(net, _loss(_forward(net, inp), inp, keys))
    return _ALONE[key]


def _same(got, want, what):
    assert set(got) == set(want)
    for n, g in got.items():
        assert torch.equal(g, want[n]), (what, n, float((g - want[n]).abs().max()))


def _train_plans(eng):
    return [k for k in eng._plans if isinstance(k, tuple) and k and k[0] == "train"]


def test_reference_iteration_follows_the_reference_trajectory():
    """The g18 sequence on the HIP net with ``torch.optim.Adam``: per iteration pass 1 and its losses, the dead pass 2,
    ``zero_grad`` / ``backward`` / ``step``, gamma, pass 3 on the stepped weights, the classifier's loss, its ``backward`` (back
    through the net's encoder) and its own Adam step.  Tolerances are g11's (the same arithmetic at the same sizes): each loss
    2e-5 relative, the final parameters 3e-5 of max (``_check_cvae_final``), the two recorded ``.grad`` tensors 3e-5 of max.
    Before the pass slots this raised at the first ``backward`` (pass 2 had replaced pass 1's activations)."""
    from behavior_driven_video_synthesis_amd.models.pose_behavior_rnn import ResidualBehaviorNet
    meta, arr = load_golden("g18_cvae_iteration")
    seed = meta["seed"]
    net = ResidualBehaviorNet(**meta["kw"])
    net.load_state_dict(synth_behavior_state(meta["shapes"], seed, {}))
    net = net.cuda().train()
    bsz, t_len, n_kps, hid = meta["batch"], meta["seq_len"], meta["kw"]["n_kps"], meta["kw"]["dim_hidden_b"]
    classifier_beta = torch.nn.Linear(hid, meta["n_classes"])           # Classifier_action_beta.forward is its fc1 (stays torch)
    with torch.no_grad():
        classifier_beta.weight.copy_(0.1 * seeded_randn("cvit.cls.weight", (meta["n_classes"], hid), seed))
        classifier_beta.bias.copy_(0.1 * seeded_randn("cvit.cls.bias", (meta["n_classes"],), seed))
    classifier_beta = classifier_beta.cuda()
    optimizer = torch.optim.Adam([{"params": net.b_enc.parameters(), "name": "z_enc"}, {"params": net.decoder.parameters(), "name": "dec"}],
                                 lr=meta["lr"])
    optimizer_classifier_beta = torch.optim.Adam(classifier_beta.parameters(), lr=meta["lr_classifier"])
    labels = torch.tensor(meta["labels"]).cuda()
    named = dict(net.named_parameters())
    state = {"gamma": meta["gamma_init"]}

    def noise(it, k):
        return seeded_randn(f"cvit.s{it}.p{k}.eps0", (bsz, hid), seed).cuda()

    def train_fn(it):      # (a function, as the reference's is: its locals -- the three passes' outputs -- die when it returns)
        kps = (0.5 * seeded_randn(f"cvit.kps{it}", (bsz, t_len + 1, n_kps), seed)).cuda()
        kps_cross = (0.5 * seeded_randn(f"cvit.kpsx{it}", (bsz, t_len + 1, n_kps), seed)).cuda()
        seq_b, target_self, seq_2 = kps[:, :-1], kps[:, 1:], kps_cross[:, :-1]
        xs, cs, _, bs, mu_s, logstd_s, pre_s = net(seq_b, seq_b, t_len, eps=noise(it, 1))
        recon_loss = torch.mean(torch.nn.functional.mse_loss(xs, target_self, reduction="none"))
        std = torch.exp(logstd_s)
        kl_loss_avg = (torch.sum(-logstd_s + 0.5 * (std ** 2 + mu_s ** 2), dim=-1) - 0.5 * hid).mean()      # lib/losses.py:283-291
        xt, ct, _, bt, mu_t, logstd_t, pre_t = net(seq_2, seq_b, t_len, eps=noise(it, 2))
        loss = meta["recon_loss_weight"] * recon_loss + state["gamma"] * kl_loss_avg
        optimizer.zero_grad()
        loss.backward()
        optimizer.step()
        state["gamma"] = max(state["gamma"] - meta["gamma_step"] * (meta["imax"] - float(kl_loss_avg.detach())), 0)
        _, _, _, _, mu_s, *_ = net(seq_b, seq_b, t_len, eps=noise(it, 3))
        mu3 = mu_s.detach().clone()
        predict = classifier_beta(mu_s)
        loss_classifier_action_beta = torch.nn.CrossEntropyLoss()(predict, labels)
        optimizer_classifier_beta.zero_grad()
        loss_classifier_action_beta.backward()
        optimizer_classifier_beta.step()
        return float(loss.detach()), float(loss_classifier_action_beta.detach()), mu3

    figures = []
    for it in range(meta["steps"]):
        loss, loss_cls, mu3 = train_fn(it)
        want = meta["logs"][it]
        figures.append((abs(loss - want["loss"]) / abs(want["loss"]),
                        abs(loss_cls - want["loss_classifier_action_beta"]) / abs(want["loss_classifier_action_beta"])))
        if it == 0:
            g_enc = S._rel(named["b_enc.rnn.weight_hh_l0"].grad, arr["grad0.b_enc.rnn.weight_hh_l0"])     # pass 1's + pass 3's
            g_dec = S._rel(named["decoder.rnn.weight_hh"].grad, arr["grad0.decoder.rnn.weight_hh"])       # pass 1's alone
            mu_err = S._rel(mu3, arr["mu3_0"])
        assert abs(state["gamma"] - want["gamma"]) <= 2e-5 * abs(want["gamma"]) + 2e-6, (it, state["gamma"], want["gamma"])
    cls_err = max(S._rel(classifier_beta.weight, arr["classifier_beta.fc1.weight"]), S._rel(classifier_beta.bias, arr["classifier_beta.fc1.bias"]))
    print(f"\n[g18] per iteration (loss, classifier loss) relative: {[(f'{a:.1e}', f'{b:.1e}') for a, b in figures]}; grads after "
          f"iteration 0: encoder {g_enc:.1e}, decoder {g_dec:.1e} of max; pass 3's mu {mu_err:.1e}; classifier_beta {cls_err:.1e}")
    for it, (a, b) in enumerate(figures):
        assert a <= 2e-5 and b <= 2e-5, (it, a, b)
    assert g_enc <= 3e-5 and g_dec <= 3e-5 and mu_err <= 2e-5, (g_enc, g_dec, mu_err)
    worst = S._check_cvae_final(net, meta, arr, 3e-5)
    assert cls_err <= 3e-5, cls_err
    print(f"[g18] parameters after 3 iterations: {worst:.2e} of max|.|")
    # the iteration holds three passes of one shape at its peak, and lets go of all of them
    eng = net.train_engine()
    assert len(_train_plans(eng)) == 3 and eng._passes.alive((bsz, t_len, t_len, t_len)) == 0


@pytest.mark.parametrize("order", ["AB", "BA"])
@pytest.mark.parametrize("rows,hid,t", NET_SHAPES)
def test_two_passes_in_flight_either_backward_order(rows, hid, t, order):
    net = _net(hid)
    inp = {tag: _inputs(tag, rows, hid, t) for tag in "AB"}
    loss = {}
    for tag in "AB":                       # forward A, forward B ...
        loss[tag] = _loss(_forward(net, inp[tag]), inp[tag])
    for tag in order:                      # ... then the two backward passes in either order
        _same(_grads(net, loss[tag]), _alone(tag, rows, hid, t), (order, tag))
    assert len(_train_plans(net.train_engine())) == 2


def test_a_third_pass_of_another_length_interleaved():
    rows, hid, t = 17, 128, 5
    net = _net(hid)
    shapes = {"A": t, "C": t + 2, "B": t}
    inp = {tag: _inputs(tag, rows, hid, tt) for tag, tt in shapes.items()}
    loss = {tag: _loss(_forward(net, inp[tag]), inp[tag]) for tag in ("A", "C", "B")}
    for tag in ("B", "C", "A"):
        _same(_grads(net, loss[tag]), _alone(tag, rows, hid, shapes[tag]), tag)
    eng = net.train_engine()
    assert sorted(len(k) for k in _train_plans(eng)) == [5, 5, 6]      # slot 0 of each length, slot 1 of the length used twice


@pytest.mark.parametrize("rows,hid,t", NET_SHAPES)
def test_backward_may_run_more_than_once(rows, hid, t):
    net, inp = _net(hid), _inputs("A", rows, hid, t)
    loss = _loss(_forward(net, inp), inp)
    want = _alone("A", rows, hid, t)
    loss.backward(retain_graph=True)
    loss.backward(retain_graph=True)
    for n, q in net.named_parameters():
        assert torch.equal(q.grad, 2 * want[n]), n          # g + g is exact in float32
    _same(_grads(net, loss), want, "third")


@pytest.mark.parametrize("rows,hid,t", NET_SHAPES)
def test_encoder_only_backward(rows, hid, t, monkeypatch):
    """A loss on mu and logstd alone (pass 3 of the reference's iteration) skips the decoder's back-propagation through time: no
    cell kernel of the roll-out is launched, the decoder's gradients are exactly zero, the encoder's and the heads' are those of
    the full path with zero upstream gradients (the same loss ``+ 0 * xs.sum()``)."""
    from behavior_driven_video_synthesis_amd import seq_train as T
    cells = []
    real = T._call
    monkeypatch.setattr(T, "_call", lambda name, *a: (cells.append(name) if name == "vunet_seq_cell_bwd" else None, real(name, *a))[1])
    inp = _inputs("A", rows, hid, t)
    res = {}
    for full in (False, True):
        net = _net(hid)
        out = _forward(net, inp)
        loss = _loss(out, inp, ("mu", "logstd"))
        if full:
            loss = loss + 0 * out["xs"].sum()
        del cells[:]
        res[full] = _grads(net, loss)
        assert len(cells) == (2 * t if full else t), (full, len(cells))
    for n, g in res[False].items():
        if n.startswith("decoder."):
            assert not g.any() and not res[True][n].any(), n
        else:
            assert g.any(), n
        assert torch.equal(g, res[True][n]), n
    _same(res[False], _alone("A", rows, hid, t, ("mu", "logstd")), "alone")


def test_stale_weights_are_refused():
    rows, hid, t = 17, 128, 5
    net, inp = _net(hid), _inputs("A", rows, hid, t)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    _loss(_forward(net, inp), inp).backward()                  # forward and backward without a step between them: fine
    loss = _loss(_forward(net, inp), inp)
    opt.step()
    with pytest.raises(RuntimeError, match="parameters were modified between this pass's forward and its backward"):
        loss.backward()
    loss = _loss(_forward(net, inp), inp)                      # a new forward sees the stepped weights and is fine again
    loss.backward()


def test_the_pool_of_live_passes():
    rows, hid, t = 5, 64, 3
    net, inp = _net(hid), _inputs("A", rows, hid, t)
    eng = net.train_engine()
    assert eng.max_passes == 4
    eng.max_passes = 2
    a, b = _forward(net, inp), _forward(net, inp)
    with pytest.raises(RuntimeError, match=r"2 passes .* alive .* max_passes = 2"):
        _forward(net, inp)
    _same(_grads(net, _loss(b, inp)), _alone("A", rows, hid, t), "b")      # the refused pass disturbed nothing
    del a
    gc.collect()
    c = _forward(net, inp)                                     # takes the slot a left
    _same(_grads(net, _loss(c, inp)), _alone("A", rows, hid, t), "c")
    assert len(_train_plans(eng)) == 2
    del b, c
    gc.collect()

    net2 = _net(hid)
    for _ in range(10):                                        # one pass at a time allocates what it always did: one plan
        out = _forward(net2, inp)
        _loss(out, inp).backward()
        del out
    assert len(_train_plans(net2.train_engine())) == 1


# ------------------------------------------------------------------------------------------------ the flow
def _flow():
    flow, _ = S._random_flow(FLOW["chan"], FLOW["mid"], FLOW["depth"], FLOW["n_flows"], 5)
    return flow.train()


def _flow_inputs(tag, rows):
    c = FLOW["chan"]
    return dict(x=seeded_randn(f"pf.{tag}.x", (rows, c), 5).cuda(), wz=seeded_randn(f"pf.{tag}.wz", (rows, c), 5).cuda(),
                wl=seeded_randn(f"pf.{tag}.wl", (rows,), 5).cuda())


def _flow_loss(flow, inp):
    x = inp["x"].clone().requires_grad_(True)
    z, logdet = flow(x)
    return (z.reshape(x.shape) * inp["wz"]).sum() + (logdet * inp["wl"]).sum(), x


def _flow_grads(flow, loss, x, **kw):
    names = ["x"] + [n for n, _ in flow.named_parameters()]
    return dict(zip(names, torch.autograd.grad(loss, [x] + list(flow.parameters()), **kw)))


def _flow_alone(tag, rows):
    key = ("flow", tag, rows)
    if key not in _ALONE:
        flow, inp = _flow(), _flow_inputs(tag, rows)
        loss, x = _flow_loss(flow, inp)
        _ALONE[key] = _flow_grads(flow, loss, x)
    return _ALONE[key]


@pytest.mark.parametrize("order", ["AB", "BA"])
@pytest.mark.parametrize("rows", FLOW_ROWS)
def test_flow_two_passes_in_flight_either_backward_order(rows, order):
    flow = _flow()
    flow.flow.train_engine().max_passes = 2
    passes = {tag: _flow_loss(flow, _flow_inputs(tag, rows)) for tag in "AB"}
    for tag in order:
        _same(_flow_grads(flow, *passes[tag]), _flow_alone(tag, rows), (order, tag))
    assert len(_train_plans(flow.flow.train_engine())) == 2


def test_flow_keeps_one_pass_until_max_passes_is_raised():
    """The flow stage runs one pass per iteration (experiments/behavior_net.py:707-710): by default the flow engine keeps one, a
    second forward replaces the first pass's activations and that pass's backward raises.  With the cap raised the passes own
    their plans, and one pass more than the cap raises at its forward."""
    rows = 17
    flow = _flow()
    eng = flow.flow.train_engine()
    assert eng.max_passes == 1
    passes = {tag: _flow_loss(flow, _flow_inputs(tag, rows)) for tag in "AB"}
    with pytest.raises(RuntimeError, match="run again before this pass's backward.*max_passes"):
        _flow_grads(flow, *passes["A"])
    _same(_flow_grads(flow, *passes["B"]), _flow_alone("B", rows), "B")
    assert len(_train_plans(eng)) == 1
    del passes
    gc.collect()
    eng.max_passes = 2
    passes = {tag: _flow_loss(flow, _flow_inputs(tag, rows)) for tag in "AB"}
    with pytest.raises(RuntimeError, match=r"2 passes .* alive .* max_passes = 2"):
        _flow_loss(flow, _flow_inputs("A", rows))
    for tag in "AB":
        _same(_flow_grads(flow, *passes[tag]), _flow_alone(tag, rows), tag)
    del passes
    gc.collect()
    for _ in range(5):                                         # one pass at a time stays in slot 0
        loss, x = _flow_loss(flow, _flow_inputs("A", rows))
        loss.backward()
        del loss, x
    assert len(_train_plans(eng)) == 2


@pytest.mark.parametrize("rows", FLOW_ROWS)
def test_flow_backward_may_run_more_than_once(rows):
    flow = _flow()
    loss, x = _flow_loss(flow, _flow_inputs("A", rows))
    want = _flow_alone("A", rows)
    loss.backward(retain_graph=True)
    loss.backward(retain_graph=True)
    assert torch.equal(x.grad, 2 * want["x"])
    for n, q in flow.named_parameters():
        assert torch.equal(q.grad, 2 * want[n]), n
    _same(_flow_grads(flow, loss, x), want, "third")


@pytest.mark.parametrize("rows", FLOW_ROWS)
def test_flow_stale_weights_are_refused(rows):
    flow = _flow()
    opt = torch.optim.Adam(flow.parameters(), lr=1e-4)
    inp = _flow_inputs("A", rows)
    _flow_loss(flow, inp)[0].backward()
    loss, _ = _flow_loss(flow, inp)
    opt.step()
    with pytest.raises(RuntimeError, match="parameters were modified between this pass's forward and its backward"):
        loss.backward()
    _flow_loss(flow, inp)[0].backward()
