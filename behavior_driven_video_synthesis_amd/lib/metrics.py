"""Evaluation hooks of the hot path's output on the device (reference ``lib/metrics.py:22-116``).

``compute_ssim`` there runs the model over a reconstruction loader, moves every batch to the host and calls
``skimage.metrics.structural_similarity(..., multichannel=True, data_range=1.0, gaussian_weights=True,
use_sample_covariance=False)`` image by image (:94-107).  Here the SSIM map, its Gaussian windows and the mean are
one HIP kernel over the whole batch (``vunet_ssim_partial``); the dataset / sampler plumbing is out of scope, so the
hook takes an iterable of batches.

The Inception-based scores (``compute_fid`` :119-282, ``_calculate_fid`` :285-322, ``inception_score`` :362-415) are
DRIVERS around a feature extractor / classifier: any callable mapping an image batch to features / logits.  The network the
reference plugs in -- torchvision's Inception-v3 -- is shipped as ``models.imagenet_pretrained.FIDInceptionModel`` (pool
features, the reference's class) and ``InceptionV3`` (logits), inference only, on their own HIP kernels (models/inception.py):
``compute_fid(model, batches, feature_extractor=FIDInceptionModel(state_dict=sd).cuda())``,
``inception_score(imgs, classifier=InceptionV3(state_dict=sd).cuda(), splits=10, resize=True)``.  Only the pretrained WEIGHTS are
third-party data this build cannot fetch (like VGG19's): ``sd`` is a torchvision ``inception_v3`` state dict the user supplies.
The statistics -- feature mean and covariance, the matrix square root, traces, softmax and the KL divergences -- are float64
on the host exactly as the reference computes them (numpy / scipy), pinned against the reference's own functions on synthetic
features (tests/golden/g7_metrics.npz).  The Inception score's statistic also exists on the device (``inception_score_device``,
``inception_score(..., on_device=True)``: csrc/inception_score.hip), and ``evaluate_image_model`` is the one-pass scoring of an
image model -- SSIM and both Inception scores, optionally on person-box crops (person_crop.py) -- behind ``ShapePoseNet.evaluate``.
The FID statistic exists on the device too (``fid_from_features_device``, ``compute_fid(..., on_device=True)``,
``evaluate_image_model(..., fid_extractor=...)``: fid_device.py, csrc/fid.hip -- float64 matrix-core products and a polar iteration
in place of ``sqrtm``); the default route stays the host's.
"""
from __future__ import annotations

import math
from typing import Callable, Dict, Iterable, Optional, Tuple

import numpy as np
import torch

from . import utils
from .. import ops

_SIGMA, _TRUNCATE = 1.5, 3.5


def _window(device) -> torch.Tensor:
    r = int(_TRUNCATE * _SIGMA + 0.5)
    w = [math.exp(-0.5 * (i * i) / (_SIGMA * _SIGMA)) for i in range(-r, r + 1)]
    s = sum(w)
    return torch.tensor([v / s for v in w], dtype=torch.float32, device=device)


def ssim(rec: torch.Tensor, target: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    """Per-image SSIM of two [N, C, H, W] batches with values in [0, data_range] -> [N] (fp32)."""
    if rec.shape != target.shape or rec.dim() != 4:
        raise ValueError("ssim expects two [N, C, H, W] tensors of the same shape")
    ops._dev(rec)
    ops._dev(target)
    rec, target = rec.contiguous().float(), target.contiguous().float()
    n, c, h, w = rec.shape
    tiles = ((h + 7) // 8) * ((w + 31) // 32)
    partial = torch.empty(n * c * tiles, device=rec.device, dtype=torch.float32)
    ops._call("vunet_ssim_partial", ops._p(rec), ops._p(target), n * c, h, w, float(data_range), ops._p(_window(rec.device)),
              ops._p(partial), ops._stream())
    return partial.view(n, c * tiles).sum(dim=1) / float(c * (h - 10) * (w - 10))


def psnr(rec: torch.Tensor, target: torch.Tensor, data_range: float = 1.0) -> torch.Tensor:
    """Per-image PSNR in dB -> [N]."""
    mse = (rec.float() - target.float()).pow(2).flatten(1).mean(dim=1)
    return 10.0 * torch.log10(data_range * data_range / mse)


def _with_images(model, batch, jpeg_entropy: str = "host"):
    """``batch`` with ``pose_img`` / ``app_img`` made on the GPU from raw uint8 frames where it brings ``pose_img_u8`` /
    ``app_img_u8`` (+ ``*_geom``) or encoded ``pose_img_jpeg`` / ``app_img_jpeg`` instead (image_input.batch_images); the batch
    itself otherwise."""
    if not any(k in batch for k in ("pose_img_u8", "app_img_u8", "pose_img_jpeg", "app_img_jpeg")):
        return batch
    from .. import image_input
    made = image_input.batch_images(batch, model.spatial_size, jpeg_entropy)
    return {**batch, **made} if made else batch


def _inplane_app(model, batch, inplane_parts):
    """The appearance input of an ``inplane_normalize`` model: ``batch["pose_img_inplane"]`` where the batch carries it, else the
    part crops cut on the GPU from ``batch["pose_img"]`` and ``batch["inplane_keypoints"]`` with ``inplane_parts`` (a
    ``inplane.PartModel``, a dataset name or a part list), at the size the model's appearance encoder takes."""
    if "pose_img_inplane" in batch or "inplane_keypoints" not in batch:
        return batch["pose_img_inplane"]
    from .. import inplane
    if inplane_parts is None:
        raise ValueError("inplane_keypoints without pose_img_inplane: pass inplane_parts (inplane.MARKET_PARTS, ...) to cut the crops")
    s_out = model.spatial_size // 2 ** (model.n_scales - model.n_scales_x)
    return inplane.part_crops(batch["pose_img"], batch["inplane_keypoints"], inplane_parts, s_out, model.spatial_size)


@torch.no_grad()
def compute_ssim(model: torch.nn.Module, batches: Iterable[Dict[str, torch.Tensor]], max_n_samples: int = 8000,
                 inplane_normalize: bool = False, inplane_parts=None, jpeg_entropy: str = "host") -> float:
    """lib/metrics.py:22-116 on an iterable of batches: reconstruct (``model(app, stickman)[0]``), scale both images
    to [0, 1] (:86-92) and average the per-image SSIM over at most ``max_n_samples`` samples."""
    was_training = model.training
    model.eval()
    total, count = None, 0
    for batch in batches:
        batch = _with_images(model, batch, jpeg_entropy)
        target = batch["pose_img"]
        if "app_img" in batch and type(model).__name__ == "VunetOrg":   # :71-74
            app = batch["app_img"]
        else:
            app = _inplane_app(model, batch, inplane_parts) if inplane_normalize else target
        rec = model(app, batch["stickman"])[0]
        vals = ssim(utils.scale_img(rec), utils.scale_img(target))
        take = min(vals.numel(), max_n_samples - count)
        s = vals[:take].sum()
        total = s if total is None else total + s
        count += take
        if count >= max_n_samples:
            break
    model.train(was_training)
    return float(total / count) if count else float("nan")


# ------------------------------------------------------------------------------------------------
# FID / Inception score (lib/metrics.py:119-415): drivers around a user-supplied Inception network
# ------------------------------------------------------------------------------------------------
def _calculate_fid(mu1, cov1, mu2, cov2, eps: float = 1e-6) -> float:
    """lib/metrics.py:285-322 (Frechet distance of two Gaussians):
    ``|mu1 - mu2|^2 + tr(S1) + tr(S2) - 2 tr(sqrtm(S1 S2))`` with the reference's handling of a singular product (eps on the
    diagonals) and of the small imaginary part ``scipy.linalg.sqrtm`` may return."""
    from scipy import linalg
    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    sigma1, sigma2 = np.atleast_2d(cov1), np.atleast_2d(cov2)
    assert mu1.shape == mu2.shape, "Training and test mean vectors have different lengths"
    assert sigma1.shape == sigma2.shape, "Training and test covariances have different dimensions"
    diff = mu1 - mu2
    covmean, _ = linalg.sqrtm(sigma1.dot(sigma2), disp=False)
    if not np.isfinite(covmean).all():
        print(f"fid calculation produces singular product; adding {eps} to diagonal of cov estimates")
        offset = np.eye(sigma1.shape[0]) * eps
        covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError(f"Imaginary component {np.max(np.abs(covmean.imag))}")
        covmean = covmean.real
    return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean))


def fid_from_features(gt_features: np.ndarray, gen_features: np.ndarray) -> float:
    """:211-212, :272-275: mean and ``np.cov(rowvar=False)`` of each [N, D] feature set, then ``_calculate_fid``."""
    gt, gen = np.asarray(gt_features, dtype=np.float64), np.asarray(gen_features, dtype=np.float64)
    return _calculate_fid(np.mean(gt, axis=0), np.cov(gt, rowvar=False), np.mean(gen, axis=0), np.cov(gen, rowvar=False))


def fid_from_features_device(gt_features, gen_features, tol: float = 1e-14, max_iter: int = 100) -> float:
    """``fid_from_features`` on the device (fid_device.py): feature sets [N >= 2, D], fp32 or float64 device tensors (host arrays are
    uploaded); mean, covariance, traces and ``tr sqrtm(S1 S2)`` by float64 matrix products and a polar iteration, no ``sqrtm``."""
    from ..fid_device import fid_device
    return float(fid_device(gt_features, gen_features, tol, max_iter).fid)


def _compute_fid_device(model, batches, feature_extractor, gt_features, max_n_samples, inplane_normalize, inplane_parts,
                        jpeg_entropy="host") -> float:
    """``compute_fid`` with the features gathered on the device: one clone per batch (an ``InceptionV3`` returns views into its
    arena), no host copy, ``gt_features`` uploaded once."""
    def _keep(f):
        f = f.detach()
        return (f if f.dtype == torch.float64 else f.float()).clone()
    was_training = model.training
    model.eval()
    gts, gens, n = [], [], 0
    try:
        for batch in batches:
            batch = _with_images(model, batch, jpeg_entropy)
            target = batch["pose_img"]
            if "app_img" in batch and type(model).__name__ == "VunetOrg":
                app = batch["app_img"]
            else:
                app = _inplane_app(model, batch, inplane_parts) if inplane_normalize else target
            if gt_features is None:
                gts.append(_keep(feature_extractor(target)))
            gens.append(_keep(feature_extractor(model(app, batch["stickman"])[0])))
            n += target.shape[0]
            if n >= max_n_samples:
                break
    finally:
        model.train(was_training)
    gen = torch.cat(gens, dim=0)
    return fid_from_features_device(gt_features if gt_features is not None else torch.cat(gts, dim=0), gen)


@torch.no_grad()
def compute_fid(model: torch.nn.Module, batches: Iterable[Dict[str, torch.Tensor]], feature_extractor: Callable,
                gt_features: Optional[np.ndarray] = None, max_n_samples: int = 8000,
                inplane_normalize: bool = False, inplane_parts=None, on_device: bool = False, jpeg_entropy: str = "host") -> float:
    """lib/metrics.py:119-282 on an iterable of batches.  ``feature_extractor(images) -> [N, D]`` stands for the
    reference's ``FIDInceptionModel`` (``models.imagenet_pretrained.FIDInceptionModel`` with the user's torchvision weights, or any
    other callable); ground-truth features are
    computed from ``batch["pose_img"]`` unless ``gt_features`` (the reference's cached ``<dataset>-fid-features.npy``) is
    given; generated features come from the reconstructions ``model(app, stickman)[0]`` (:243-258).  ``on_device``: the features
    of all batches stay in device buffers and the statistic is ``fid_from_features_device`` -- no per-batch host copy, no
    ``np.cov``, no ``scipy.linalg.sqrtm``.  ``jpeg_entropy``: ``jpeg_decode.decode_batch``'s ``entropy`` for batches of encoded frames."""
    if on_device:
        return _compute_fid_device(model, batches, feature_extractor, gt_features, max_n_samples, inplane_normalize, inplane_parts,
                                   jpeg_entropy)
    was_training = model.training
    model.eval()
    gts, gens, n = [], [], 0
    for batch in batches:
        batch = _with_images(model, batch, jpeg_entropy)
        target = batch["pose_img"]
        if "app_img" in batch and type(model).__name__ == "VunetOrg":
            app = batch["app_img"]
        else:
            app = _inplane_app(model, batch, inplane_parts) if inplane_normalize else target
        if gt_features is None:
            gts.append(feature_extractor(target).detach().double().cpu().numpy())
        gens.append(feature_extractor(model(app, batch["stickman"])[0]).detach().double().cpu().numpy())
        n += target.shape[0]
        if n >= max_n_samples:
            break
    model.train(was_training)
    gt = np.asarray(gt_features) if gt_features is not None else np.concatenate(gts, axis=0)
    return fid_from_features(gt, np.concatenate(gens, axis=0))


def inception_score_from_probs(preds: np.ndarray, splits: int = 1) -> Tuple[float, float]:
    """:403-415: per split, ``exp(mean_i KL(p(y|x_i) || p(y)))`` with ``p(y)`` the split's mean prediction
    (``scipy.stats.entropy(pyx, py)``); returns (mean, std) over the splits."""
    from scipy.stats import entropy
    preds = np.asarray(preds, dtype=np.float64)
    n = preds.shape[0]
    split_scores = []
    for k in range(splits):
        part = preds[k * (n // splits): (k + 1) * (n // splits), :]
        py = np.mean(part, axis=0)
        split_scores.append(np.exp(np.mean([entropy(part[i, :], py) for i in range(part.shape[0])])))
    return float(np.mean(split_scores)), float(np.std(split_scores))


def inception_score_device(logits: torch.Tensor, splits: int = 1) -> Tuple[float, float]:
    """``inception_score_from_probs(softmax(logits), splits)`` on the device: logits [N, K] fp32 -> (mean, std) over the splits.
    The float64 softmax, the split means, the KL divergences and the exponentials are ``vunet_inception_score``
    (csrc/inception_score.hip); only the ``splits`` doubles are copied to the host."""
    if not (torch.is_tensor(logits) and logits.is_cuda):
        raise RuntimeError("inception_score_device needs device logits (hand-written gfx950 kernels; no CPU fallback)")
    if logits.dim() != 2 or logits.shape[0] < 1 or logits.shape[1] < 1 or int(splits) < 1:
        raise ValueError(f"logits [N >= 1, K >= 1] and splits >= 1 expected, got {tuple(logits.shape)}, splits = {splits}")
    x = logits.detach().to(torch.float32).contiguous()
    n, k, splits = int(x.shape[0]), int(x.shape[1]), int(splits)
    work = torch.empty(4 * n + splits * k, device=x.device, dtype=torch.float64)
    scores = torch.empty(splits, device=x.device, dtype=torch.float64)
    with torch.cuda.device(x.device):
        ops._call("vunet_inception_score", ops._p(x), n, k, splits, ops._p(work), ops._p(scores), ops._stream())
    s = scores.cpu().numpy()
    return float(np.mean(s)), float(np.std(s))


@torch.no_grad()
def inception_score(imgs, classifier: Callable, batch_size: int = 32, resize: bool = False, splits: int = 1,
                    device=None, boxes=None, valid=None, crop_size=None, sampling="reference",
                    on_device: bool = False) -> Tuple[float, float]:
    """lib/metrics.py:362-415.  ``imgs``: tensor [N, 3, H, W] in [-1, 1] (or a dataset of 1-tuples of such images, as the
    reference takes); ``classifier(images) -> logits [n, K]`` stands for torchvision's pretrained ``inception_v3``
    (``models.imagenet_pretrained.InceptionV3`` with the user's weights, or any other callable).  ``resize``: bilinear up-sampling to 299 x 299 first (:385, ``nn.Upsample(size=(299, 299),
    mode='bilinear')`` -- align_corners False).

    ``boxes`` [N, 4] int32 (+ ``valid`` [N], ``crop_size``, ``sampling``: person_crop.py): the score of the person-box crops of
    ``imgs`` (run_inference's "IS on masks") without the crops being stored -- needs ``resize=True`` and a classifier that takes the
    boxes (``InceptionV3``): crop and resize are then the classifier's first launch.  ``on_device``: the logits of all batches are
    gathered in one device buffer and the statistic is one call at the end (``inception_score_device``) instead of one host copy
    of the probabilities per batch."""
    if not torch.is_tensor(imgs):
        imgs = torch.stack([imgs[i][0] if isinstance(imgs[i], (tuple, list)) else imgs[i] for i in range(len(imgs))])
    n = imgs.shape[0]
    assert batch_size > 0 and n > batch_size
    if boxes is not None or on_device:
        return _inception_score_boxed(imgs, classifier, batch_size, resize, splits, device, boxes, valid, crop_size, sampling, on_device)
    preds = []
    for i in range(0, n, batch_size):
        x = imgs[i:i + batch_size]
        if device is not None:
            x = x.to(device)
        if resize:
            x = torch.nn.functional.interpolate(x.float(), size=(299, 299), mode="bilinear", align_corners=False)
        preds.append(torch.softmax(classifier(x).double(), dim=1).cpu().numpy())
    return inception_score_from_probs(np.concatenate(preds, axis=0), splits)


def _inception_score_boxed(imgs, classifier, batch_size, resize, splits, device, boxes, valid, crop_size, sampling, on_device):
    """``inception_score`` with boxes and / or the statistic on the device; batches as there."""
    if boxes is not None and not resize:
        raise ValueError("boxes are cropped inside the resize-to-299 launch: pass resize=True")
    n = imgs.shape[0]
    logits = None
    preds = []
    for i in range(0, n, batch_size):
        x = imgs[i:i + batch_size]
        if device is not None:
            x = x.to(device)
        if boxes is not None:
            out = classifier(x.float(), boxes=boxes[i:i + batch_size].to(x.device),
                             valid=None if valid is None else valid[i:i + batch_size].to(x.device), crop_size=crop_size,
                             sampling=sampling, resize=True)
        else:
            if resize:
                x = torch.nn.functional.interpolate(x.float(), size=(299, 299), mode="bilinear", align_corners=False)
            out = classifier(x)
        if on_device:
            if logits is None:
                logits = torch.empty(n, out.shape[1], device=out.device, dtype=torch.float32)
            logits[i:i + out.shape[0]] = out
        else:
            preds.append(torch.softmax(out.double(), dim=1).cpu().numpy())
    if on_device:
        return inception_score_device(logits, splits)
    return inception_score_from_probs(np.concatenate(preds, axis=0), splits)


@torch.no_grad()
def evaluate_image_model(model: torch.nn.Module, batches: Iterable[Dict[str, torch.Tensor]], classifier: Callable,
                         crop: Optional[str] = None, max_n_samples: int = 8000, splits: int = 1, sampling: str = "reference",
                         inplane_normalize: bool = False, inplane_parts=None, *, fid_extractor: Optional[Callable] = None,
                         gt_features=None) -> Dict[str, float]:
    """The scores of an image model in one pass over ``batches`` -- ``compute_eval_metrics``
    (experiments/shape_and_pose_net.py:666-755) with ``crop=None``, ``run_inference`` (:856-918) with ``crop="person"``.

    Per batch, in eval mode under ``no_grad``: ``rec = model(timg, stickman)[0]`` and ``tr = model.transfer(app_img, stickman)``
    (:693-703; ``app_img`` is ``batch["app_img"]`` where the batch brings one, else ``timg``; ``VunetOrg`` reconstructs from its
    appearance input, as ``compute_ssim`` decides).  The SSIM is taken of the SAME ``rec`` -- the reference runs a second loader and a
    second reconstruction for it (``compute_ssim``, :737-745); sums and the one division as in ``compute_ssim``.  Both image sets go
    through ``classifier`` with the resize to 299 x 299 as its first launch; with ``crop="person"`` that launch also cuts every
    image to the box of ``batch["keypoints"] * spatial_size`` (:880, :888-891; ``classifier`` an ``InceptionV3``: one fused launch,
    any other callable: ``person_crop.crop_and_resize`` then ``inception_input``).  The logits stay on the device and the two
    statistics are ``inception_score_device``: no image and no probability leaves the device.  An image without a valid keypoint
    (``valid == 0``) is left out of both scores and counted in ``n_without_box``.  The loop ends as the reference's does:
    before batch ``i`` where ``i * batch_size >= max_n_samples``.

    ``fid_extractor`` (keyword only; a ``FIDInceptionModel`` or any callable images -> [n, D]): the same ``rec``, uncropped, also
    goes through it, as ``compute_fid`` feeds it, and the result gains ``"fid"`` -- ``fid_from_features_device`` of the gathered
    features against those of ``target`` (or against ``gt_features``, the reference's cached feature file, uploaded once): the
    FID that experiments/vunet.py:604-636 logs beside the SSIM.  Without an extractor nothing changes.

    -> {"ssim", "is_recon", "std_is_recon", "is_transfer", "std_is_transfer", "n", "n_without_box"} (+ "fid")."""
    from .. import person_crop
    from ..models.inception import InceptionV3, inception_input
    if crop not in (None, "person"):
        raise ValueError(f"crop: None or 'person' expected, got {crop!r}")
    person_crop._sampling(sampling)
    fused = isinstance(classifier, InceptionV3)
    was_training = model.training
    model.eval()
    total, count, n_seen, batch_size = None, 0, 0, None
    rec_logits, tr_logits, valids = [], [], []
    fid_gt, fid_gen = [], []

    def _keep(f):   # (an InceptionV3 returns a view into its arena)
        f = f.detach()
        return (f if f.dtype == torch.float64 else f.float()).clone()
    try:
        for i, batch in enumerate(batches):
            batch = _with_images(model, batch)
            target = batch["pose_img"]
            if batch_size is None:
                batch_size = int(target.shape[0])
            if i * batch_size >= max_n_samples:
                break
            size = int(target.shape[-1])
            if "app_img" in batch and type(model).__name__ == "VunetOrg":   # as compute_ssim
                timg = batch["app_img"]
            else:
                timg = _inplane_app(model, batch, inplane_parts) if inplane_normalize else target
            app_img = batch.get("app_img", timg)
            stickman = batch["stickman"]
            rec = model(timg, stickman)[0]
            tr = model.transfer(app_img, stickman)
            vals = ssim(utils.scale_img(rec), utils.scale_img(target))
            take = min(vals.numel(), max_n_samples - count)
            if take > 0:
                s = vals[:take].sum()
                total = s if total is None else total + s
                count += take
            boxes = valid = None
            if crop == "person":
                if "keypoints" not in batch:
                    raise KeyError('crop="person" cuts every image to the box of batch["keypoints"] * spatial_size: the batch has none')
                kps = batch["keypoints"].to(rec.device).float() * float(model.spatial_size)   # :880
                boxes, valid = person_crop.keypoint_boxes(kps)
                valids.append(valid)
            for img, sink in ((rec, rec_logits), (tr, tr_logits)):
                img = img.detach().float()
                if boxes is None:
                    out = classifier(img, resize=True) if fused else classifier(inception_input(img))
                elif fused:
                    out = classifier(img, boxes=boxes, valid=valid, crop_size=size, sampling=sampling, resize=True)
                else:
                    out = classifier(inception_input(person_crop.crop_and_resize(img, boxes, size, valid, sampling)))
                sink.append(out.float().clone())   # (an InceptionV3 returns a view into its arena)
            if fid_extractor is not None:
                if gt_features is None:
                    fid_gt.append(_keep(fid_extractor(target)))
                fid_gen.append(_keep(fid_extractor(rec)))
            n_seen += int(target.shape[0])
    finally:
        model.train(was_training)
    if not rec_logits:
        raise ValueError("evaluate: no batch")
    rec_all, tr_all = torch.cat(rec_logits, dim=0), torch.cat(tr_logits, dim=0)
    n_without_box = 0
    if valids:
        keep = torch.cat(valids, dim=0) != 0
        n_without_box = int(keep.numel() - int(keep.sum()))
        rec_all, tr_all = rec_all[keep], tr_all[keep]
    if rec_all.shape[0] == 0:
        raise ValueError("evaluate: no image with a valid keypoint")
    is_rec, std_rec = inception_score_device(rec_all, splits)
    is_tr, std_tr = inception_score_device(tr_all, splits)
    res = {"ssim": float(total / count) if count else float("nan"), "is_recon": is_rec, "std_is_recon": std_rec,
           "is_transfer": is_tr, "std_is_transfer": std_tr, "n": n_seen, "n_without_box": n_without_box}
    if fid_extractor is not None:
        res["fid"] = fid_from_features_device(gt_features if gt_features is not None else torch.cat(fid_gt, dim=0),
                                              torch.cat(fid_gen, dim=0))
    return res
