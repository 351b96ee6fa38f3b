"""Float64 CPU restatement of the real-vs-fake classifier study (experiments/behavior_net.py:1302-1521) with torch modules,
and the seeded inputs of fixture g14 (tests/golden/make_golden_classifier_study.py).  Used by
tests/test_classifier_study_golden.py (CPU) and tests/test_hip_classifier_study.py (GPU)."""
import numpy as np
import torch

from synth import seeded_randn

NIN = 51
# tag: (with a flow, rows, T, H, bs, iterations, times)
CASES = {"flow": (True, 96, 12, 32, 32, 30, (0, 5, 11)), "noflow": (False, 96, 12, 32, 32, 30, (0, 5, 11))}
SEED = 141
KINDS = ("prior", "cross", "flow")


def inputs(tag):
    """-> (sets {orig, prior, cross, self, (flow), embed}, init [per start time {prior, cross, (flow), self, regressor}]),
    float32 CPU tensors drawn from ``seeded_randn``.  Classifier weights ~ N(0, 1) / 16 (torch's default is U(-1/16, 1/16)),
    regressor weights ~ N(0, 1) / sqrt(fan_in)."""
    flow, n, t, h, _, _, times = CASES[tag]
    sets = {k: seeded_randn(f"g14.{tag}.{k}", (n, t, NIN), SEED) for k in ("orig", "prior", "cross", "self") + (("flow",) if flow else ())}
    sets["cross"] = sets["orig"] + 0.5 * sets["cross"]            # fakes at different distances from the real set
    sets["self"] = sets["orig"] + 0.1 * sets["self"]
    sets["embed"] = seeded_randn(f"g14.{tag}.embed", (n, h), SEED)
    init = []
    for si in range(len(times)):
        d = {}
        for k in KINDS[:3 if flow else 2] + ("self",):
            p = f"g14.{tag}.{si}.{k}."
            d[k] = {"GRU.weight_ih_l0": seeded_randn(p + "wih", (768, NIN), SEED) / 16, "GRU.weight_hh_l0": seeded_randn(p + "whh", (768, 256), SEED) / 16,
                    "GRU.bias_ih_l0": seeded_randn(p + "bih", (768,), SEED) / 16, "GRU.bias_hh_l0": seeded_randn(p + "bhh", (768,), SEED) / 16,
                    "fc1.weight": seeded_randn(p + "fcw", (1, 256), SEED) / 16, "fc1.bias": seeded_randn(p + "fcb", (1,), SEED) / 16}
        p = f"g14.{tag}.{si}.reg."
        r = {}
        for name, (o, i) in (("fc1", (h // 2, h)), ("fc2", (h // 4, h // 2)), ("fc3", (NIN, h // 4))):
            r[name + ".weight"] = seeded_randn(p + name + "w", (o, i), SEED) / float(np.sqrt(i))
            r[name + ".bias"] = seeded_randn(p + name + "b", (o,), SEED) / float(np.sqrt(i))
        d["regressor"] = r
        init.append(d)
    return sets, init


class GRUClassifier(torch.nn.Module):
    def __init__(self, sd, dtype):
        super().__init__()
        self.GRU = torch.nn.GRU(NIN, 256, 1, batch_first=True)
        self.fc1 = torch.nn.Linear(256, 1)
        self.load_state_dict(sd)
        self.to(dtype)

    def forward(self, x):
        _, h = self.GRU(x)
        return self.fc1(h.reshape(x.shape[0], -1))


class Regressor(torch.nn.Module):
    def __init__(self, sd, h, dtype):
        super().__init__()
        self.fc1 = torch.nn.Linear(h, h // 2)
        self.fc2 = torch.nn.Linear(h // 2, h // 4)
        self.fc3 = torch.nn.Linear(h // 4, NIN)
        self.load_state_dict(sd)
        self.to(dtype)

    def forward(self, x):
        return self.fc3(torch.relu(self.fc2(torch.relu(self.fc1(x)))))


def run(sets, init, times, bs, iterations, dtype=torch.float64):
    """The study with torch modules in ``dtype``: -> (finals, curves) in behavior_eval.classifier_study's layout.
    ``class_real_self`` never trains (its optimiser covers class_real2's parameters after their zero_grad): only its mean
    sigmoid on the fake half is computed."""
    flow = "flow" in sets
    kinds = KINDS[:3 if flow else 2]
    x = {k: v.to(dtype) for k, v in sets.items()}
    n = x["orig"].shape[0]
    nb = n // bs
    epochs = iterations // nb
    bce = torch.nn.BCEWithLogitsLoss(reduction="mean")
    names = {"prior": ("acc1", "loss1", "Acc Prior"), "cross": ("acc2", "loss2", "Acc Cross"), "flow": ("acc_flow", "loss_flow", "Acc Flow")}
    finals, curves = [], []
    for si, start in enumerate(times):
        cls = {k: GRUClassifier(init[si][k], dtype) for k in kinds}
        opt = {k: torch.optim.SGD(cls[k].parameters(), lr=1e-3, momentum=0.9) for k in kinds}
        selfc = GRUClassifier(init[si]["self"], dtype)
        reg = Regressor(init[si]["regressor"], x["embed"].shape[1], dtype)
        ropt = torch.optim.Adam(reg.parameters(), lr=1e-3)
        cur = {v: [] for k in kinds for v in names[k][:2]}
        cur["acc_self"], cur["loss_regressor"] = [], []

        def reg_step(i):
            pred = reg(x["embed"][i * bs:(i + 1) * bs])
            loss = torch.mean(torch.norm(pred - x["orig"][i * bs:(i + 1) * bs, start], dim=1))
            ropt.zero_grad()
            loss.backward()
            ropt.step()
            return loss.item()

        for _ in range(epochs):
            for i in range(nb):
                sl = slice(i * bs, (i + 1) * bs)
                for k in kinds:
                    p = cls[k](x[k][sl])
                    cur[names[k][0]].append(torch.mean(torch.sigmoid(p)).item())
                    loss = bce(p, torch.zeros_like(p)) + bce(cls[k](x["orig"][sl]), torch.ones_like(p))
                    cur[names[k][1]].append(loss.item())
                    opt[k].zero_grad()
                    loss.backward()
                    opt[k].step()
                with torch.no_grad():
                    cur["acc_self"].append(torch.mean(torch.sigmoid(selfc(x["self"][sl]))).item())
                cur["loss_regressor"].append(reg_step(i))
        fin = {names[k][2]: [] for k in kinds}
        fin.update({"Acc Self": [], "Loss_regressor": [], "DE": []})
        for i in range(nb):
            sl = slice(i * bs, (i + 1) * bs)
            fin["DE"].append(torch.mean(torch.norm(x["cross"][sl, start] - x["orig"][sl, start], dim=1)).item())
            with torch.no_grad():
                for k in kinds:
                    fin[names[k][2]].append(torch.mean(torch.sigmoid(cls[k](x[k][sl]))).item())
                fin["Acc Self"].append(torch.mean(torch.sigmoid(selfc(x["self"][sl]))).item())
            fin["Loss_regressor"].append(reg_step(i))
        finals.append({k: float(np.mean(v)) for k, v in fin.items()})
        curves.append({k: np.asarray(v) for k, v in cur.items()})
    return finals, curves
