"""The image experiments' post-hoc pose-regressor probe as one recorded training step (csrc/reg_probe.hip,
include/vunet_reg_probe.h).

Both image experiments end ``run_inference`` by training a fresh ``models.vunets.Regressor`` on the frozen VUnet's appearance
``means`` (experiments/shape_and_pose_net.py:921-995, experiments/vunet.py:745-805):

    preds = regressor(means);  loss = torch.mean(torch.norm(preds - reg_targets, dim=1))
    optimizer_regressor.zero_grad();  loss.backward();  optimizer_regressor.step()          # Adam(lr=0.001)

``RegProbeEngine`` runs that step over the module's own parameters: the embedders as split-K products of the flattened latents
(``weight`` [out, in, k, k] is already the row-major [out, in k k] matrix: read in place), the linears, the input gradients
and the weight gradients fused into Adam on the seq family's kernels, the loss on a kernel that appends to a device-side loss
course.  The step is recorded once per batch size into a hipGraph and replayed (``VUNET_SEQ_GRAPH=0``: issued eagerly).

The kernels' tiles want every matrix in multiples of 64 rows and columns.  A parameter whose shape fits -- both embedders and
the first linear of the shipped configuration -- is the kernels' operand and is updated in place; any other trains as a
zero-padded image (padded rows produce zeros and receive no update) that ``write_back`` copies into the module.

There is no CPU path.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Sequence

import torch

from . import _lib
from .ops import _call, _p, _stream, mark_written
from .seq import ACT_NONE, SeqLinearDesc, _GraphCache, _need_device, _need_module_on, _up, linear
from .seq_train import (ACT_RELU_SEQ, AdamState, SeqDxDesc, TrainLayer, _table, adam_state_dict, dx_chain, dx_split,
                        load_adam_state)

MAX_SCALES = 2
TOO_MANY_SCALES = "the fused regressor engine covers at most two latent scales; the module route still serves more"


def split_k(m: int, k: int) -> int:
    """Slabs of an embedder's K: as many as put about one workgroup on each of the chip's 256 CUs (a workgroup owns 16 rows of W
    over one slab), each a multiple of 64 columns, in equal parts."""
    chunks = k // 64
    want = max(1, min(chunks, 256 // max(1, m // 16)))
    return max(s for s in range(1, want + 1) if chunks % s == 0)


class RegProbeEngine:
    """One training step of ``models.vunets.Regressor`` -- forward, ``mean_b ||pred_b - tgt_b||_2``, backward, torch's Adam
    (betas 0.9 / 0.999, eps 1e-8, no weight decay; bias correction in double on the device) -- for one batch of <= 64 rows.
    The module's parameters are updated in place (after ``write_back`` for those that train as padded images); the engine owns
    Adam's moments (``optimizer_state_dict`` / ``load_optimizer_state_dict``: torch.optim.Adam's layout)."""

    def __init__(self, reg, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, n_steps: int = 0):
        if reg.n_stages > MAX_SCALES:
            raise NotImplementedError(TOO_MANY_SCALES)
        dev = reg.linears[0].weight.device
        if dev.type != "cuda":
            raise RuntimeError("the regressor probe runs on hand-written gfx950 kernels: move the module to the GPU first "
                               "(no CPU fallback)")
        _lib.lib()
        _need_module_on(dev, reg.named_parameters())
        self.reg, self.dev = reg, dev
        self.adam = AdamState(dev, lr, betas, eps, 0.0)
        self.graph = _GraphCache()
        self._plans: Dict[int, dict] = {}
        self.last = torch.zeros(1, device=dev)                           # the latest step's loss
        self.cursor = torch.zeros(1, dtype=torch.int32, device=dev)      # steps appended to the loss course
        self.losses_dev = torch.zeros(max(int(n_steps), 1), device=dev)
        self.cap = int(n_steps)
        self.load_module()

    # ---- weights
    def load_module(self):
        """(Re)build the training state from the module's parameters; Adam's moments and step count are reset."""
        r = self.reg
        self.emb: List[TrainLayer] = []
        pieces, off = [], 0
        for i, e in enumerate(r.embedders):
            m, k = e.weight.shape[0], e.weight[0].numel()
            if k % 64:
                raise ValueError(f"embedder {i} reads {k} values per sample: the split-K kernel takes multiples of 64")
            self.emb.append(TrainLayer(f"embedders.{i}", e.weight, e.bias))
            pieces.append((i * m, m, off))
            off += _up(m, 64)
        self.ldc = off                                                   # the concat operand: one 64-padded block per embedder
        self.lin: List[TrainLayer] = []
        kp = self.ldc
        for i, lin_ in enumerate(r.linears):
            pc = pieces if i == 0 else None
            if i == 0 and sum(n for _, n, _ in pc) != lin_.weight.shape[1]:
                raise ValueError("the first linear layer does not read the concatenated embeddings")
            self.lin.append(TrainLayer(f"linears.{i}", lin_.weight, lin_.bias, pc, kp))
            kp = self.lin[-1].mp
        self.n_out = r.linears[-1].weight.shape[0]
        self._inplace = [t for lay in self.layers() for t in lay.inplace_params()]
        self.adam.step_dev.zero_()
        self._reset_recordings()

    def layers(self) -> List[TrainLayer]:
        return self.emb + self.lin

    def write_back(self):
        for layer in self.layers():
            layer.write_back()

    def _reset_recordings(self):
        self._plans.clear()
        self.graph.clear()

    def reserve(self, n_steps: int):
        """A fresh loss course of ``n_steps`` entries (the recorded steps hold the old buffer's address: they are dropped)."""
        self.cap = int(n_steps)
        self.losses_dev = torch.zeros(max(self.cap, 1), device=self.dev)
        self.cursor.zero_()
        self._reset_recordings()

    # ---- buffers
    def plan(self, rows: int) -> dict:
        p = self._plans.get(rows)
        if p is not None:
            return p
        if not 1 <= rows <= 64:
            raise ValueError(f"the regressor probe's step takes one batch of 1..64 rows, got {rows}")
        bp = _up(rows, 16)
        z = lambda *s: torch.zeros(*s, device=self.dev)   # noqa: E731
        p = dict(b_pad=bp, x=[z(bp, e.k) for e in self.emb], cat=z(bp, self.ldc), dcat=z(bp, self.ldc),
                 y=[z(bp, lay.mp) for lay in self.lin], dz=[z(bp, lay.mp) for lay in self.lin], tgt=z(rows, self.n_out),
                 S_emb=[split_k(_up(e.rows, 16), e.k) for e in self.emb],
                 S_dx=[dx_split(lay.mp, lay.kp, 1) for lay in self.lin])
        p["part"] = z(max(s * bp * _up(e.rows, 16) for s, e in zip(p["S_emb"], self.emb)))
        p["raw"] = z(max(s * bp * lay.kp for s, lay in zip(p["S_dx"], self.lin)))
        # the update sweep: every layer in one launch.  An embedder's dZ is its column block of the concat operand's gradient.
        entries, tile, off = [], 0, 0
        for e, x in zip(self.emb, p["x"]):
            entries.append(e.dw_entry(p["dcat"].data_ptr() + 4 * off, self.ldc, x.data_ptr(), e.k, tile))
            tile += e.tiles()
            off += e.mp
        for i, lay in enumerate(self.lin):
            x = p["cat"] if i == 0 else p["y"][i - 1]
            entries.append(lay.dw_entry(p["dz"][i].data_ptr(), lay.mp, x.data_ptr(), lay.kp, tile))
            tile += lay.tiles()
        p["dw"] = dict(table=_table(entries, self.dev), n=len(entries), tiles=tile)
        self._plans[rows] = p
        return p

    # ---- the launch sequence
    def _issue_forward(self, rows: int, p: dict):
        off = 0
        for e, x, s in zip(self.emb, p["x"], p["S_emb"]):
            m16 = _up(e.rows, 16)
            _call("vunet_reg_probe_embed", _p(x), _p(e.w), rows, m16, e.k, s, _p(p["part"]), _stream())
            _call("vunet_reg_probe_embed_finish", _p(p["part"]), s, _p(e.b), rows, m16, _p(p["cat"]), self.ldc, off, _stream())
            off += e.mp
        last = len(self.lin) - 1
        for i, lay in enumerate(self.lin):
            x = p["cat"] if i == 0 else p["y"][i - 1]
            linear(SeqLinearDesc(rows, lay.mp, lay.kp, lay.kp, ACT_NONE if i == last else ACT_RELU_SEQ, ACT_NONE, 1, 1, 1), [lay.w], x,
                   [lay.b], p["y"][i])

    def _issue_step(self, rows: int, p: dict):
        last = len(self.lin) - 1
        self._issue_forward(rows, p)
        _call("vunet_reg_probe_loss", _p(p["y"][last]), self.lin[last].mp, _p(p["tgt"]), self.n_out, rows, self.n_out, _p(p["dz"][last]),
              _p(self.last), _p(self.losses_dev) if self.cap else None, self.cap, _p(self.cursor), _stream())
        for i in range(last, -1, -1):          # input gradients on the weights before this step's update
            lay = self.lin[i]
            dx_chain(SeqDxDesc(rows, lay.mp, lay.kp, 1, p["S_dx"][i], 0), [lay.w], p["dz"][i], p["raw"],
                     (p["cat"], p["dcat"]) if i == 0 else (p["y"][i - 1], p["dz"][i - 1]))
        self.adam.tick()
        _call("vunet_seq_dw", _p(p["dw"]["table"]), p["dw"]["n"], 0, p["dw"]["tiles"], rows, ctypes.byref(self.adam.hp), _stream())

    def _load_inputs(self, p: dict, means: Sequence[torch.Tensor], rows: int):
        means = list(means)
        if len(means) != len(self.emb):
            raise ValueError(f"the regressor has {len(self.emb)} embedders, got {len(means)} latents")
        _need_device(*means)
        for latent, e, x in zip(reversed(means), self.emb, p["x"]):      # models/vunets.py:813: reversed(embeddings)
            if latent.shape[0] != rows or latent[0].numel() != e.k:
                raise ValueError(f"{e.name} reads {e.k} values per sample, got a latent of shape {tuple(latent.shape)}")
            x[:rows].copy_(latent.detach().reshape(rows, e.k))

    def forward(self, means: Sequence[torch.Tensor]) -> torch.Tensor:
        """``Regressor.forward`` on the engine's kernels and operand images -> pred [B, n_out] (a copy)."""
        rows = means[0].shape[0]
        p = self.plan(rows)
        self._load_inputs(p, means, rows)
        self._issue_forward(rows, p)
        return p["y"][-1][:rows, :self.n_out].clone()

    def step(self, means: Sequence[torch.Tensor], targets: torch.Tensor) -> torch.Tensor:
        """One optimisation step on ``means`` (the VUnet's list, coarsest first) and ``targets`` [B, n_out].  -> the device
        scalar [1] holding this step's loss (overwritten by the next step).  No host synchronisation."""
        rows = means[0].shape[0]
        p = self.plan(rows)
        self._load_inputs(p, means, rows)
        _need_device(targets)
        p["tgt"].copy_(targets.detach().reshape(rows, self.n_out))
        self.graph.run_step(rows, lambda: self._issue_step(rows, p))
        mark_written(self._inplace)      # (the padded images' parameters: ``write_back``)
        return self.last

    def losses(self) -> torch.Tensor:
        """The loss course so far, as a host tensor (ONE device-to-host copy)."""
        both = torch.cat([self.cursor.to(torch.float32), self.losses_dev]).cpu()
        return both[1:1 + min(int(both[0]), self.cap)].clone()

    # ---- torch.optim.Adam's state layout over ``reg.parameters()`` (embedders, then linears: weight, bias each)
    def optimizer_state_dict(self) -> dict:
        return adam_state_dict(self.adam, self.adam.step, [mv for lay in self.layers() for mv in lay.moments()])

    def load_optimizer_state_dict(self, sd: dict):
        states, step = load_adam_state(self.adam, sd)
        for i, lay in enumerate(self.layers()):
            lay.set_moments(states[2 * i], states[2 * i + 1])
        self.adam.step_dev.fill_(step)
        self.graph.clear()      # the hyper-parameters are launch arguments of the recorded step


# ================================================================================================
# the probe loop of run_inference (experiments/shape_and_pose_net.py:936-986, experiments/vunet.py:757-797)
# ================================================================================================
def run_probe(regressor, encode, batches, n_epochs: int = 20, lr: float = 1e-3, eps=None) -> dict:
    """Train ``regressor`` for ``n_epochs`` passes over ``batches`` (a re-iterable of dict batches with ``keypoints``) on the
    latents ``encode(batch, eps)`` returns, one recorded step per batch, without a host synchronisation inside the loop.
    ``eps``: None, one list of noise tensors (one per latent scale, used for every batch) or one such list per batch of an epoch.
    -> {"loss": float tensor [n_steps] on the host, "regressor": the trained module, "running_mean_100": the mean of the last
    100 losses, the figure the reference's progress bar shows (:980-982)}."""
    try:
        per_epoch = len(batches)
    except TypeError:
        per_epoch = sum(1 for _ in batches)
    engine = regressor.probe_engine(lr=lr, n_steps=per_epoch * n_epochs)
    per_batch = eps is not None and len(eps) > 0 and isinstance(eps[0], (list, tuple))
    for _ in range(n_epochs):
        for i, batch in enumerate(batches):
            reg_targets = batch["keypoints"]
            reg_targets = reg_targets.reshape(reg_targets.shape[0], -1).to(engine.dev, torch.float32)      # :957-958
            with torch.no_grad():
                means = encode(batch, eps[i] if per_batch else eps)
            engine.step(means, reg_targets)
    engine.write_back()
    loss = engine.losses()
    return {"loss": loss, "regressor": regressor, "running_mean_100": float(loss[-100:].mean()) if loss.numel() else float("nan")}
