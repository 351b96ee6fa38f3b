"""CPU reference of the skeleton frames (TEST INFRASTRUCTURE ONLY): the canvas through tests/skeleton_ref.c -- the drawing
primitives of oracle/stickman_oracle.c, included unchanged -- and the resize, crop, span and overlay as the reference's own
numpy expressions (data/data_conversions_3d.py:1176-1214), written out literally, one frame at a time."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "skeleton_ref.c")
ORACLE_SRC = os.path.join(os.path.dirname(HERE), "oracle", "stickman_oracle.c")
LIB = os.path.join(os.path.dirname(HERE), "oracle", "_build", "libskeleton_ref.so")


def build(force: bool = False) -> str:
    if force or not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(ORACLE_SRC)):
        os.makedirs(os.path.dirname(LIB), exist_ok=True)
        # the flags of oracle/stickman.py
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-std=c99", "-o", LIB, SRC, "-lm"], check=True)
    return LIB


_lib = None


def canvas(kps, limbs, colors, hs, ws, thickness=3, background=255):
    """kps [F, J, 2] float32 -> uint8 [F, Hs, Ws, 3]: every limb a cv2.line on the background-filled canvas."""
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build())
    kps = np.ascontiguousarray(kps, dtype=np.float32)
    limbs = np.ascontiguousarray(limbs, dtype=np.int32).reshape(-1, 2)
    colors = np.ascontiguousarray(colors, dtype=np.uint8).reshape(-1, 3)
    assert len(limbs) == len(colors)
    f, j = kps.shape[:2]
    out = np.zeros((f, 3, hs, ws), dtype=np.uint8)
    _lib.skeleton_ref_draw(kps.ctypes.data_as(ctypes.c_void_p), f, j, limbs.ctypes.data_as(ctypes.c_void_p),
                           colors.ctypes.data_as(ctypes.c_void_p), len(limbs), out.ctypes.data_as(ctypes.c_void_p), int(hs),
                           int(ws), int(thickness), int(background))
    return np.ascontiguousarray(out.transpose(0, 2, 3, 1))


def table(n_src, n_dst):
    """OpenCV 4.1.2 resizeNN's index table in float64: ifx = 1 / (dst / src); x -> min(floor(x * ifx), src - 1)."""
    ifx = 1.0 / (float(n_dst) / n_src)
    return np.asarray([min(int(np.floor(x * ifx)), n_src - 1) for x in range(n_dst)], dtype=np.int64)


def resize_nearest(img, ht, wt):
    """cv2.resize(img, (wt, ht), interpolation=cv2.INTER_NEAREST) by that table."""
    return img[table(img.shape[0], ht)][:, table(img.shape[1], wt)]


def frames(kps, limbs, colors, image_size, target_size=None, thickness=3, background=255, crop=False, target_width=128,
           crop_joints=None, rgb=None, overlay=False):
    """project_onto_image_plane after the projection, per frame.  ``target_size`` = (Ht, Wt); ``rgb`` uint8 [F, S, S, 3].
    -> dict(skel=[F, Ht, W', 3], rgb=..., overlay=..., span=int [F, 2, 2])."""
    hs, ws = image_size
    full = canvas(kps, limbs, colors, hs, ws, thickness, background)
    imgs, imgs_rgb, spans = [], [], []
    for f in range(len(full)):
        img = full[f]
        pose_i = np.asarray(kps[f], dtype=np.float32).astype(np.float64)
        s = np.asarray([hs, ws])
        span = [[0, 0], [0, 0]]
        if rgb is not None:
            rgb_img = rgb[f][None]
            size_arr = np.full((1, 2), rgb_img.shape[1], dtype=float)
            joint_scaling = size_arr / np.expand_dims(s, axis=0)
            if crop:
                k = pose_i[crop_joints] if crop_joints is not None else pose_i
                kps_rescaled = k * joint_scaling
                center_kps = np.mean(kps_rescaled, axis=0)
                min_x = int(min(max(0, center_kps[0] - target_width // 2), rgb_img.shape[1] - target_width))
                max_x = min_x + target_width
                rgb_img = rgb_img[:, :, min_x:max_x]
                span[1] = [min_x, max_x]
            imgs_rgb.append(rgb_img.squeeze(0))
        if target_size is not None:
            # cv2's dsize is (width, height); ``scaling`` below divides the image's (h, w) by it in that order, as upstream
            dsize = (target_size[1], target_size[0])
            scaling = np.asarray(img.shape[:2], dtype=float) / np.asarray(dsize, dtype=float)
            img = resize_nearest(img, target_size[0], target_size[1])
        else:
            scaling = np.ones(2, dtype=float)
        if crop:
            k = pose_i[crop_joints] if crop_joints is not None else pose_i
            kps_rescaled = k / np.expand_dims(scaling, axis=0)
            center_kps = np.mean(kps_rescaled, axis=0)
            min_x = int(min(max(0, center_kps[0] - target_width // 2), img.shape[1] - target_width))
            max_x = min_x + target_width
            img = img[:, min_x:max_x]
            span[0] = [min_x, max_x]
        imgs.append(img)
        spans.append(span)
    out = {"skel": np.stack(imgs, axis=0), "span": np.asarray(spans, dtype=np.int64).reshape(len(imgs), 2, 2)}
    if rgb is not None:
        out["rgb"] = np.stack(imgs_rgb, axis=0)
        if overlay:
            out["overlay"] = np.stack([np.where(np.expand_dims(np.all(stick == 255, axis=2), axis=-1), r, stick)
                                       for stick, r in zip(imgs, imgs_rgb)], axis=0)
    return out
