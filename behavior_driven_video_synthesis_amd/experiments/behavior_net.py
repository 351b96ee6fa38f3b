"""The two training stages of ``experiments/behavior_net.py`` (BASELINE config 4) on the MI355X path.

``BehaviorNet.train_fn(batch)`` is the reference's ``train_fn`` (:446-760) for a batch ``{"keypoints": [B, T + 1, n_kps]}``:

* first stage (``only_flow`` False, :591-660): ``net(seq_b, seq_b, seq_len)`` -> ``recon_loss_weight * mean(MSE) + tuning *
  kl_loss`` (``tuning`` = gamma, or 1 with ``cvae``) -> with ``use_regressor`` (:627-648) five inner steps of the adversarial
  pose regressor and ``loss -= w clamp(L_5, max=0.45) + w clamp(L_5, max=0.7)`` -> backward -> ``Adam(lr_init)`` -> the gamma
  controller (:111-116).  Forward, loss, the regressor's steps, back-propagation through time and the fused optimiser step
  are one recorded hipGraph (csrc/seq.hip, csrc/seq_bptt.hip, csrc/seq_train.hip, csrc/seq_reg.hip).  ``train_fn(...,
  update=epoch < n_epochs - 10)`` is the reference's freeze of the last ten epochs (:656-660): the regressor still trains,
  the net and gamma do not.  The regressor term follows the reference's pinned torch 1.3.1, whose Adam writes through
  ``p.data``: its gradient reaches mu through the regressor's weights AFTER the fifth inner update, with the fifth forward's
  ReLU masks (seq_train.RegressorTrainEngine).
* flow stage (``only_flow`` True, :703-714): the net encodes under ``no_grad``, then ``latent_flow(bs.detach())`` ->
  ``FlowLoss`` -> backward -> ``Adam(flow_lr * batch_size, betas (0.5, 0.9), weight_decay)`` with the weight gradient fused
  into the update (``seq_train.FlowTrainEngine``).

``BehaviorNet.evaluate(batches, stats)`` scores a model as ``run_inference`` does (:1112-1301, APD from lib/logging.py:2079-2093):
ASD, FSD, APD, ADE and FDE of ``n_samples`` sampled behaviours per scored sequence, and the transfer metrics
(behavior_eval.py, csrc/seq_eval.hip).  With ``latent_diagnostics`` it also runs the latent part of ``eval_nets``
(lib/logging.py:2228-2262, :2549-2562): the flow's held-out ``FlowLoss`` entries, the self-reconstruction error, the KS test of the
Gaussianised codes and the collected sample sets (latent_diag.py, csrc/seq_latent.hip).

Not on this path, and said here rather than silently dropped:
* the second pass ``net(seq_2, seq_start_t, seq_len)`` (:600-603): none of its outputs reaches the loss or the log;
* the action classifiers (:662-690): models/pose_discriminator.py is outside the path and they feed no
  gradient that the net's optimiser uses.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import torch

from ..models.flow.simple_flow import UnsupervisedTransformer2
from ..models.pose_behavior_rnn import Regressor_fly, ResidualBehaviorNet
from ..ops import _call, _p, _stream
from ..optim import FusedAdam
from ..seq_train import REG_C, REG_T, RegressorTrainEngine

DEFAULT_CONFIG = {   # config/behavior_net.yaml
    "architecture": {"decoder_arch": "lstm", "linear_in_decoder": False, "dim_hidden_b": 1024, "flow_mid_channels_factor": 2,
                     "n_flows": 15, "flow_hidden_depth": 2, "cvae": False},
    "training": {"batch_size": 64, "n_epochs": 50, "lr_init": 1e-4, "tau": [0.2, 0.45, 0.7], "gamma": 0.3, "weight_decay": 0.0,
                 "recon_loss_weight": 2.5, "information_max": 100, "gamma_init": 0, "gamma_step": 1e-5, "flow_lr": 4.5e-7,
                 "use_regressor": False, "weight_regressor": 0.01, "imax_scaling": "none", "only_flow": False},
}


class BehaviorNet:
    def __init__(self, config: Optional[dict] = None, n_kps: int = 51, device="cuda", hip_graph: bool = True):
        import copy
        self.config = copy.deepcopy(DEFAULT_CONFIG if config is None else config)
        arch, tr = self.config["architecture"], self.config["training"]
        self.device = torch.device(device)
        self.only_flow = bool(tr.get("only_flow", False))
        self.net = ResidualBehaviorNet(n_kps=n_kps, information_bottleneck=True, **arch).to(self.device)     # :310-313
        self.optimizer = FusedAdam([{"params": list(self.net.b_enc.parameters()), "name": "z_enc"},
                                    {"params": list(self.net.decoder.parameters()), "name": "dec"}], lr=tr["lr_init"])   # :324-331
        self.optimizer.use_device_schedule()
        self.latent_flow = UnsupervisedTransformer2(flow_in_channels=arch["dim_hidden_b"], n_flows=arch["n_flows"],
                                                    flow_hidden_depth=arch["flow_hidden_depth"],
                                                    flow_mid_channels=arch["dim_hidden_b"] * arch["flow_mid_channels_factor"]).to(self.device)
        self.flow_lr = tr["flow_lr"] * tr["batch_size"]                                                          # :382
        self.flow_engine = self.latent_flow.flow.train_engine(lr=self.flow_lr, betas=(0.5, 0.9), weight_decay=tr["weight_decay"])
        self.gamma_dev = torch.full((1,), float(tr["gamma_init"]), device=self.device)
        self.imax = float(tr["information_max"])
        self.imax_dev = torch.full((1,), self.imax, device=self.device)
        self.hip_graph = hip_graph
        self.use_regressor = bool(tr.get("use_regressor", False))
        self.cvae = bool(arch.get("cvae", False))
        self.kl_weight_dev = torch.ones(1, device=self.device) if self.cvae else None   # tuning = 1. (:606)
        self.regressor = self.regressor_engine = None
        self._reg_generation = 0
        if self.use_regressor:   # :305-306
            self.regressor = Regressor_fly(arch["dim_hidden_b"], n_kps).to(self.device)
            self.regressor_engine = RegressorTrainEngine(self.regressor, lr=1e-4)

    # ---- the reference's knobs
    @property
    def gamma(self) -> float:
        return float(self.gamma_dev.item())

    def set_imax(self, imax: float):
        if float(imax) != self.imax:
            self.imax = float(imax)
            self.imax_dev.fill_(self.imax)

    def set_lr(self, lr: float):
        """``MultiStepLR`` (:337-339) steps the net's learning rate per epoch."""
        for g in self.optimizer.param_groups:
            g["lr"] = float(lr)
        self.optimizer.lr_dev.fill_(float(lr))
        self.optimizer._lr_mirrored = float(lr)

    # ---- one step
    def _cvae_step(self, seq_b, target, eps, reg_index, update: bool) -> Dict:
        tr = self.config["training"]
        eng = self.net.train_engine()
        eng._check()
        rows, t_in = seq_b.shape[0], seq_b.shape[1]
        p = eng._tplan(rows, t_in, t_in, t_in)
        p["x1"].copy_(seq_b)
        p["x2"].copy_(seq_b)
        p["target"].copy_(target)
        if eps is None:
            torch.randn(p["eps"].shape, out=p["eps"])
        else:
            p["eps"].copy_(eps)
        rp = None
        if self.use_regressor:
            rp = self.regressor_engine.plan(rows)
            if reg_index is None:   # torch.randint(0, seq_len, (1,)) per inner step (:629), drawn outside the recording
                rp["idx"].random_(0, t_in)
            else:
                idx = torch.as_tensor(reg_index).reshape(-1)
                if idx.numel() != 5 or int(idx.min()) < 0 or int(idx.max()) >= t_in:
                    raise ValueError(f"reg_index: five indices in [0, {t_in}), got {idx.tolist()}")
                rp["idx"].copy_(idx)
        grads = {n: q.grad for n, q in self.net.named_parameters()}
        gamma_step = float(tr["gamma_step"]) if update else 0.0   # the frozen epochs do not move gamma (:656-660)

        def issue():
            eng._fill_images()
            eng._issue_train_forward(rows, p, t_in, t_in, t_in, 0, False)
            dxs, dmu, dlogstd = (_p(p["gxs"]), _p(p["gmu"]), _p(p["glogstd"])) if update else (None, None, None)
            if self.cvae:
                _call("vunet_seq_vae_loss_w", _p(p["xs"]), _p(p["target"]), _p(p["mu"]), _p(p["logstd"]), rows, t_in, eng.n, eng.H,
                      float(tr["recon_loss_weight"]), _p(self.kl_weight_dev), _p(self.gamma_dev), _p(self.imax_dev), gamma_step,
                      _p(p["part"]), _p(p["scalars"]), _p(p["per_seq"]), dxs, dmu, dlogstd, _stream())
            else:
                _call("vunet_seq_vae_loss", _p(p["xs"]), _p(p["target"]), _p(p["mu"]), _p(p["logstd"]), rows, t_in, eng.n, eng.H,
                      float(tr["recon_loss_weight"]), _p(self.gamma_dev), _p(self.imax_dev), gamma_step, _p(p["part"]),
                      _p(p["scalars"]), _p(p["per_seq"]), dxs, dmu, dlogstd, _stream())
            if rp is not None:
                self.regressor_engine.issue_step(rows, rp, p["mu"], p["x1"], t_in, float(tr["weight_regressor"]), p["scalars"],
                                                 p["gmu"] if update else None)
            if update:
                eng._issue_train_backward(rows, p, t_in, t_in, False)
                eng._unpack_grads(p, grads)
                self.optimizer.step()
        eng.graph.enabled = self.hip_graph
        mode = eng.graph.run_step(("cvae", rows, t_in, self.use_regressor, self.cvae, bool(update), self._reg_generation), issue)
        if mode == "replayed" and update:
            self.optimizer.note_replayed_steps(1)
        if rp is not None:
            self.regressor_engine.mark_written()
        p["reg"] = rp
        return p

    def train_fn(self, batch: Dict[str, torch.Tensor], eps: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
                 sync: bool = True, update: bool = True, reg_index=None) -> Dict:
        """``eps``: the reparametrisation noise (None: drawn); ``noise``: the draw behind the flow stage's logged
        ``reference_nll_loss``.  ``sync`` False returns device tensors instead of floats (no host round trip per step).
        ``update``: the caller passes ``epoch < n_epochs - 10`` (:656); False runs the step without the net's backward, its
        optimiser step and the gamma update -- the regressor still trains and the logs are produced.  ``reg_index``: the five
        inner steps' sequence indices (None: drawn on the device)."""
        kps = batch["keypoints"].to(self.device, torch.float32)
        seq_b, target = kps[:, :-1].contiguous(), kps[:, 1:].contiguous()       # prepare_input (lib/utils.py:914-917)
        seq_len = seq_b.shape[1]
        out: Dict = {}
        if not self.only_flow:
            if self.use_regressor and seq_len != REG_T:
                raise ValueError(f"use_regressor needs seq_len == {REG_T}: the regressor's fc4 is Linear({REG_T}, {REG_C}) on a one-hot over the "
                                 f"sequence (models/pose_behavior_rnn.py:55), got seq_len {seq_len}")
            p = self._cvae_step(seq_b, target, eps, reg_index, update)
            sc = p["scalars"]
            out.update(loss=sc[0], loss_recon=sc[1], kl_loss=sc[2], gamma=self.gamma_dev[0], mu_s=sc[4], logstd_s=sc[5],
                       loss_per_seq_recon=p["per_seq"])
            if p["reg"] is not None:
                out["loss_regressor"] = p["reg"]["reg"][4]
        else:
            with torch.no_grad():
                xs, cs, _, bs, mu_s, logstd_s, pre_s = self.net(seq_b, seq_b, seq_len, eps=eps)
                eng = self.net.train_engine()
                eng._check()
                p = eng._tplan(seq_b.shape[0], seq_len, seq_len, seq_len)
                _call("vunet_seq_vae_loss", _p(xs), _p(target), _p(mu_s), _p(logstd_s), seq_b.shape[0], seq_len, eng.n, eng.H,
                      float(self.config["training"]["recon_loss_weight"]), _p(self.gamma_dev), _p(self.imax_dev), 0.0, _p(p["part"]),
                      _p(p["scalars"]), _p(p["per_seq"]), None, None, None, _stream())
                sc = p["scalars"].clone()
            self.flow_engine.graph.enabled = self.hip_graph
            fl = self.flow_engine.train_step(bs.detach(), noise)
            out.update(flow_loss=fl[0], reference_nll_loss=fl[1], nlogdet_loss=fl[2], nll_loss=fl[3], loss_recon=sc[1], kl_loss=sc[2],
                       gamma=self.gamma_dev[0], mu_s=sc[4], logstd_s=sc[5], loss_per_seq_recon=p["per_seq"])
        out["imax"], out["seq_len"] = self.imax, seq_len
        if sync:
            out = {k: (v.detach().cpu().numpy() if k == "loss_per_seq_recon" else float(v)) if isinstance(v, torch.Tensor) else v
                   for k, v in out.items()}
        return out

    # ---- scoring (experiments/behavior_net.py:1112-1301, lib/logging.py:2079-2093)
    @torch.no_grad()
    def evaluate(self, batches, stats, n_samples: int = 50, skip: int = 4, use_flow: bool = True, z=None, eps=None,
                 classifier_study: bool = False, study_kwargs=None, study_noise=None, euler=None, flow_weights: str = "f32",
                 latent_diagnostics=False, latent_noise=None):
        """The reference's per-batch metric recipe of ``run_inference`` over an iterable of dict batches -> a
        ``behavior_eval.BehaviorEvaluator`` (``.summary()``: the means the reference prints; ``.lists()``: the lists).

        Batch keys:
        * ``keypoints`` [B, T + 1, n]: ``prepare_input`` (lib/utils.py:914-917) gives x_s = kps[:, :-1], target_s = kps[:, 1:].
        * ``future_keypoints`` [B, T + 1, n], one per row: what the dataset's ``_sample_valid_seq_ids`` / ``_get_keypoints`` look
          up for rows [::skip] (:1162-1179); rows [::skip] are scored against its frames 1 .. T (:1235).
        * optional ``paired_keypoints`` and ``matched_keypoints`` [B, T + 1, n] (kps2, kps3 of :1137-1143): with both present the
          transfer metrics of :1262-1278 run too.
        Sampling (:1182-1217): ``n_samples`` behaviours per scored row, from ``target_s[::skip]`` at start_frame T - 1, through
        the flow (``use_flow``) or straight from the prior.  ``stats``: ``behavior_eval.PoseStats`` of the dataset.
        ``z``: the sampling noise, [n_samples, B / skip, H] or a list with one per batch (None: drawn); ``eps``: the transfer
        metrics' reparametrisation noise [B, H], or a list (None: drawn).

        ``classifier_study`` (needs ``paired_keypoints`` and ``matched_keypoints``): the second half of ``run_inference``.  While
        fewer than ``max_rows`` (``study_kwargs``, default 25 000) rows are held, every batch's transfer metrics run and its
        sequences are collected (:1262-1295): X_orig = x_s, X_prior = net(x_s, target_s, sample=True) from frame T - 1,
        X_cross / X_self = generate_seq(mu, x_t / x_s) from frame 0, X_flow = generate_seq(flow.reverse(noise), target_s) from
        frame T - 1 (with the flow), X_embed = mu; the batch after the cap is still scored, then the loop ends.  After the loop
        ``behavior_eval.classifier_study`` runs on what was collected (the other ``study_kwargs``) and its result is
        ``ev.study``.  ``study_noise``: per batch (or one for all) {"prior": [B, H], "flow": [B, H]} (None: drawn).

        ``euler`` (a model trained on ``keypoint_type: angle_world_expmap``): ``(stats, horizons)`` or ``(stats, horizons, actions,
        max_len)`` with ``stats`` a ``pose_angles.AngleStats``.  Every batch's reconstruction ``net(x_s, x_s, T)`` (``eps``, when
        given, is its noise too) is scored against ``target_s`` with ``pose_angles.euler_error`` (``mse_euler``, lib/metrics.py:321-357)
        into ``ev.euler``, a ``pose_angles.EulerErrorTable``: per action -- the batch's optional ``actions``, one name per row;
        without it every row counts as ``"all"`` -- and horizon.  None: nothing of this runs.

        ``flow_weights``: "f32" or "bf16", the flow's weight precision while this call samples through it
        (``seq.flow_weight_mode``; the previous mode is restored afterwards).  bf16 weight images halve the bytes of a pass and
        measured 12-15 % faster at 1 and 16 rows but SLOWER than f32 in 64-row chunks, which is how the
        ``n_samples`` rows per sequence run here: the default stays "f32".

        ``latent_diagnostics``: False (nothing of this runs, no key is added), True, or {"n_max": 20000, "ks_method":
        "reference"}: the latent part of ``eval_nets`` (lib/logging.py:1988-1997, :2228-2262, :2549-2562, :2623, :2656-2660) per
        batch, on the device and without a host sync.  The reconstruction pass ``net(x_s, x_s, T)`` (``eps`` is its noise; shared
        with ``euler``) gives b, mu, pre and ``self_recon = mean((seq_pred_s - target_s)^2)``; with the flow, ``gauss, logdet =
        flow(b)`` gives the batch's ``FlowLoss`` entries (``latent_diag.flow_nll``) and ``flow.reverse(randn_like(b))`` the flow
        samples.  While ``(batch_nr + 1) B < n_max`` -- strict, as in the reference -- b, mu, pre, the prior sample (the noise
        ``net(x_s, x_s, T, sample=True)[3]`` returns; the pass around it computes nothing else that is kept and is not run),
        gauss, the flow samples and the batch's optional ``action_labels`` ([B] or [B, T] int64, the last frame's is kept) go
        into a ``latent_diag.LatentCollector``.  After the loop ``ev.latent`` (``latent_diag.LatentDiagnostics``) holds the
        collector, ``ks`` = the KS test of every dimension of the collected gauss against N(0, 1), and ``summary()`` gains
        ``self_recon_eval``, the four ``FlowLoss`` means and ``ks_p_mean`` (without a flow: ``self_recon_eval`` only).
        ``latent_noise``: per batch (or one for all) {"prior": [B, H], "flow": [B, H], "reference": [B, H]} (None: drawn)."""
        from ..seq import flow_weight_mode
        with flow_weight_mode(self.latent_flow if use_flow else None, flow_weights):
            return self._evaluate(batches, stats, n_samples, skip, use_flow, z, eps, classifier_study, study_kwargs, study_noise, euler,
                                  latent_diagnostics, latent_noise)

    def _evaluate(self, batches, stats, n_samples, skip, use_flow, z, eps, classifier_study, study_kwargs, study_noise, euler,
                  latent_diagnostics=False, latent_noise=None):
        from .. import behavior_eval as E
        ev = E.BehaviorEvaluator()
        latent_kw = None
        if latent_diagnostics:
            latent_kw = {"n_max": 20000, "ks_method": "reference"}
            if isinstance(latent_diagnostics, dict):
                unknown = set(latent_diagnostics) - set(latent_kw)
                if unknown:
                    raise ValueError(f"latent_diagnostics: unknown keys {sorted(unknown)}")
                latent_kw.update(latent_diagnostics)
        if euler is not None:
            import sys
            from .. import pose_angles as A
            angle_stats, horizons = euler[0], euler[1]
            ev.euler = A.EulerErrorTable(euler[2] if len(euler) > 2 else None, horizons, euler[3] if len(euler) > 3 else sys.maxsize)
        flow = self.latent_flow if use_flow else None
        kw = dict(study_kwargs or {})
        study = E.StudySet(kw.pop("max_rows", 25000)) if classifier_study else None
        for bi, batch in enumerate(batches):
            if study is not None and not ("paired_keypoints" in batch and "matched_keypoints" in batch):
                raise ValueError("classifier_study needs paired_keypoints and matched_keypoints in every batch")
            kps = batch["keypoints"].to(self.device, torch.float32)
            x_s, target_s = kps[:, :-1].contiguous(), kps[:, 1:].contiguous()
            t = x_s.shape[1]
            fut = batch["future_keypoints"].to(self.device, torch.float32)[::skip].contiguous()
            zb = z[bi] if isinstance(z, (list, tuple)) else z
            samples = E.sample_behaviors(self.net, flow, target_s[::skip].contiguous(), n_samples, t, start_frame=t - 1, z=zb)
            ev.add(E.sample_metrics(samples, fut, stats))
            if euler is not None or latent_kw is not None:       # one reconstruction pass serves both
                self_pass = self.net(x_s, x_s, t, eps=eps[bi] if isinstance(eps, (list, tuple)) else eps)
            if euler is not None:
                ev.euler.add(A.euler_error(self_pass[0], target_s, angle_stats, horizons), batch.get("actions") or ["all"] * x_s.shape[0])
            if latent_kw is not None:
                self._latent_batch(ev, latent_kw, bi, batch, self_pass, target_s, flow,
                                   latent_noise[bi] if isinstance(latent_noise, (list, tuple)) else latent_noise)
            if study is not None:
                if study.full:
                    break
                self._collect_study(batch, x_s, target_s, flow, study, eps[bi] if isinstance(eps, (list, tuple)) else eps,
                                    study_noise[bi] if isinstance(study_noise, (list, tuple)) else study_noise, ev)
            elif "paired_keypoints" in batch and "matched_keypoints" in batch:
                x_t = batch["paired_keypoints"].to(self.device, torch.float32)[:, :-1].contiguous()
                x_rel = batch["matched_keypoints"].to(self.device, torch.float32)[:, :-1].contiguous()
                eb = eps[bi] if isinstance(eps, (list, tuple)) else eps
                ev.add(E.transfer_metrics(self.net, x_s, x_t, x_rel, eps=eb))
        if study is not None:
            ev.study_set = study
            ev.study = E.classifier_study(study, **kw)
        if ev.latent is not None:
            ev.latent.finish()
        return ev

    @torch.no_grad()
    def _latent_batch(self, ev, kw, batch_nr, batch, self_pass, target_s, flow, noise):
        """One batch of eval_nets' latent part (lib/logging.py:1988-1997, :2228-2262): device work only."""
        from .. import latent_diag as L
        seq_pred, _, _, b, mu, _, pre = self_pass
        rows, h = b.shape[0], b.shape[1]
        noise = noise or {}

        def draw(key, like):
            v = noise.get(key)
            return torch.randn_like(like) if v is None else v.to(like.device, torch.float32).reshape(like.shape).contiguous()
        if ev.latent is None:
            dims = {"b": h, "mu": mu.shape[1], "pre": pre.reshape(rows, -1).shape[1], "prior_samples": h}
            if flow is not None:
                dims.update(flow_samples=h, gaussian_samples=h)
            ev.latent = L.LatentDiagnostics(L.LatentCollector(dims, kw["n_max"], b.device), kw["n_max"], kw["ks_method"], flow is not None)
        lat = ev.latent
        admit = lat.admits(batch_nr, rows)
        if flow is not None:
            gauss, logdet = flow(b)
            gauss = gauss.reshape(rows, h)
            lat.flow_scalars.append(L.flow_nll(gauss, logdet, draw("reference", gauss)).scalars)
            flow_samples = flow.reverse(draw("flow", b)).reshape(rows, h)
            if admit:
                lat.collector.add("flow_samples", flow_samples)
                lat.collector.add("gaussian_samples", gauss)
        lat.recon.append(torch.mean((seq_pred - target_s) ** 2))
        if admit:
            lat.collector.add("b", b)
            lat.collector.add("mu", mu)
            lat.collector.add("pre", pre)
            lat.collector.add("prior_samples", draw("prior", b))
            if "action_labels" in batch:
                a = torch.as_tensor(batch["action_labels"]).to(b.device, torch.int64)
                lat.collector.add("actions", a[:, -1] if a.dim() == 2 else a)

    @torch.no_grad()
    def _collect_study(self, batch, x_s, target_s, flow, study, eps, noise, ev):
        """One batch of :1262-1295: the transfer metrics (their mu reused) and the five sequence sets."""
        from .. import behavior_eval as E
        t = x_s.shape[1]
        x_t = batch["paired_keypoints"].to(self.device, torch.float32)[:, :-1].contiguous()
        x_rel = batch["matched_keypoints"].to(self.device, torch.float32)[:, :-1].contiguous()
        m, mu = E.transfer_metrics(self.net, x_s, x_t, x_rel, eps=eps, return_mu=True)
        ev.add(m)
        noise = noise or {}
        h = self.net.dim_hidden_b
        zp = noise.get("prior")
        if zp is None:
            zp = torch.randn(x_s.shape[0], h, device=x_s.device)
        prior = self.net(x_s, target_s, t, sample=True, start_frame=t - 1, eps=zp.to(x_s.device, torch.float32))[0]
        cross = self.net.generate_seq(mu, x_t, t, start_frame=0)[0]
        self_ = self.net.generate_seq(mu, x_s, t, start_frame=0)[0]
        xf = None
        if flow is not None:
            zf = noise.get("flow")
            if zf is None:
                zf = torch.randn(x_s.shape[0], h, device=x_s.device)
            bf = flow.reverse(zf.to(x_s.device, torch.float32).contiguous()).reshape(x_s.shape[0], h)
            xf = self.net.generate_seq(bf, target_s, t, start_frame=t - 1)[0]
        study.add(x_s, prior, cross, self_, mu, flow=xf)

    # ---- checkpoints in the reference's layout (:1003-1011: model / optimizer / flow / flow optimizer)
    def state_dict(self) -> dict:
        sd = {"model": self.net.state_dict(), "optimizer": self.optimizer.state_dict(), "flow": self.latent_flow.state_dict(),
              "flow_optimizer": self.flow_engine.optimizer_state_dict(), "gamma": self.gamma}
        if self.use_regressor:
            sd["regressor"] = self.regressor_engine.state_dict()
            sd["regressor_optimizer"] = self.regressor_engine.optimizer_state_dict()
        return sd

    def load_state_dict(self, sd: dict):
        self.net.load_state_dict(sd["model"])
        if sd.get("optimizer") is not None:
            self.optimizer.load_state_dict(sd["optimizer"])
        if sd.get("flow") is not None:
            self.latent_flow.load_state_dict(sd["flow"])
        if sd.get("flow_optimizer") is not None:
            self.flow_engine.load_optimizer_state_dict(sd["flow_optimizer"])
        if "gamma" in sd:
            self.gamma_dev.fill_(float(sd["gamma"]))
        if self.use_regressor and sd.get("regressor") is not None:   # (its optimiser state starts afresh)
            self.regressor.load_state_dict(sd["regressor"])
            self.regressor_engine.load_module()
            self._reg_generation += 1      # a recorded step holds the old fc5 image and moments
