#!/usr/bin/env python3
"""Golden-vector generator for the angle-space pose path (g12_pose_angles).  Runs ONLY in the build container (needs the
reference checkout, as make_golden.py does, whose helpers it imports).

The reference's own ``convert_to_3d`` / ``fkl`` (data/data_conversions_3d.py:1047-1066, :608-668), ``revert_coordinate_space``
(:671-703), ``unNormalizeData`` (:178-211) and ``mse_euler`` (lib/metrics.py:321-357), imported behind the stubs g9b_projection
uses, on seeded inputs.  The kinematic tree stored here is what the reference's ``_some_variables(use_posInd=True)`` returned:
data it produced, which reaches this repository's code only as arrays of this file.

Precision.  The reference runs these functions on what ``revert_output_format`` returns with the dataset's float64 statistics:
float64 arrays.  The inputs are therefore stored as the float32 values a network or a device tensor holds and handed to the
reference as float64 (handed float32 arrays, ``expmap2rotmat`` would take its norm, sine and cosine in float32).

    python tests/golden/make_golden_pose_angles.py      # regenerate tests/golden/g12_pose_angles.npz
"""
import contextlib
import io
import sys
import types

import numpy as np

import make_golden as G
from make_golden import save

SEED = 1207
DIMS, N_IGNORE = 99, 45                  # 54 used dimensions, the usual H3.6M exp-map width
N_SEQ, T_SEQ = 6, 20                     # kinematics / root path
HORIZONS = [2, 4, 8, 10]
EULER = {"long": (10, 12), "short": (4, 9)}   # tag: (sequences, frames); "short": horizon 10 is longer than the sequence
ACTIONS, MAX_LEN = ["walking", "eating"], 3


def _stubs():
    for name in ["h5py", "imagesize", "skimage", "skimage.metrics", "natsort", "kornia.geometry", "umap"]:
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                sys.modules[name] = types.ModuleType(name)
                sys.modules[name].__getattr__ = lambda k: type(k, (), {"__init__": lambda self, *a, **kw: None})


def stats(rng):
    """H3.6M-like exp-map statistics, float64: the root translation in millimetres, the angles in radians."""
    ignore = sorted((3 + rng.choice(DIMS - 3, size=N_IGNORE, replace=False)).tolist())      # the translation stays in use
    mean = np.concatenate([rng.randn(3) * 300.0, rng.randn(DIMS - 3) * 0.3])
    std = np.concatenate([50.0 + 200.0 * rng.rand(3), 0.05 + 0.3 * rng.rand(DIMS - 3)])
    return mean, std, ignore


def angle_sequences(rng):
    """[N_SEQ, T_SEQ, 99] float32 un-normalised: per joint a random axis times a magnitude in [0, 3] rad; a root translation of
    some centimetres per frame (revert_coordinate_space accumulates it); one pose all zero."""
    axis = rng.randn(N_SEQ, T_SEQ, 32, 3)
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    mag = 3.0 * rng.rand(N_SEQ, T_SEQ, 32, 1)
    x = np.concatenate([rng.randn(N_SEQ, T_SEQ, 3) * 40.0, (axis * mag).reshape(N_SEQ, T_SEQ, 96)], axis=-1)
    x[0, 3] = 0.0
    x[1, 0, 3:6] = 0.0                    # a zero root rotation in front of a scan
    return x.astype(np.float32)


def g12_pose_angles():
    _stubs()
    from data import data_conversions_3d as dc
    from lib import metrics as rmet
    rng = np.random.RandomState(SEED)
    arrays, meta = {}, {"seed": SEED, "dims": DIMS, "horizons": HORIZONS, "actions": ACTIONS, "max_len": MAX_LEN}

    parent, offset, rot_ind, expmap_ind, pos_ind = dc._some_variables(use_posInd=True)
    tree = {"parent": parent, "offset": offset, "rotInd": rot_ind, "expmapInd": expmap_ind, "posInd": {"ids": pos_ind}}
    arrays["tree.parent"] = np.asarray(parent).astype(np.int64)
    arrays["tree.offset"] = np.asarray(offset, dtype=np.float64)
    arrays["tree.expmapInd"] = np.stack([np.asarray(e) for e in expmap_ind]).astype(np.int64)
    arrays["tree.posInd"] = np.asarray(pos_ind).astype(np.int64)
    assert all(-1 <= p < i for i, p in enumerate(arrays["tree.parent"]))

    mean, std, ignore = stats(rng)
    meta["ignore"] = ignore
    arrays["stats.mean"], arrays["stats.std"] = mean, std

    # ---- kinematics: given angle vectors, and normalised network output through unNormalizeData
    ang = angle_sequences(rng)
    arrays["fk.angles"] = ang
    for swap in (False, True):
        arrays[f"fk.xyz.swap{int(swap)}"] = np.stack([dc.convert_to_3d(s.astype(np.float64), tree, swap) for s in ang])
    norm = rng.randn(N_SEQ, T_SEQ, DIMS - N_IGNORE).astype(np.float32)
    arrays["fk.normalised"] = norm
    reverted = [dc.revert_output_format(s, mean, std, ignore) for s in norm]
    assert reverted[0].dtype == np.float64
    arrays["fk.xyz.normalised"] = np.stack([dc.convert_to_3d(s, tree, False) for s in reverted])
    tree_no_pos = dict(tree, posInd={"ids": None})
    arrays["fk.xyz.no_pos"] = np.stack([dc.convert_to_3d(s.astype(np.float64), tree_no_pos, False) for s in ang[:2]])

    # ---- the root path: identity, and a start rotated about a skew axis and moved away from the origin
    r0 = dc.expmap2rotmat(np.array([0.4, -1.1, 0.7]))
    t0 = np.array([150.0, -80.0, 920.0])
    arrays["revert.R0"], arrays["revert.T0"] = r0, t0
    with contextlib.redirect_stdout(io.StringIO()) as said:
        arrays["revert.identity"] = np.stack([dc.revert_coordinate_space(s.astype(np.float64), np.eye(3), np.zeros(3)) for s in ang])
        arrays["revert.moved"] = np.stack([dc.revert_coordinate_space(s.astype(np.float64), r0, t0) for s in ang])
    meta["revert_non_unit_quaternions"] = said.getvalue().count("corrupt")
    assert meta["revert_non_unit_quaternions"] == 0

    # ---- mse_euler
    meta["euler"] = {}
    for tag, (n, t) in EULER.items():
        gt = rng.randn(n, t, DIMS - N_IGNORE).astype(np.float32)
        gt[:, :, 9:15] = gt[:, :1, 9:15]                       # some used dimensions that do not move: the deviation filter
        gt[n // 2, :, :] = gt[n // 2, :1, :]                   # a sequence standing still: nothing is kept, the error is 0
        rec = (gt + 0.25 * rng.randn(n, t, DIMS - N_IGNORE)).astype(np.float32)
        actions = [ACTIONS[i % 3 == 1] for i in range(n)]
        arrays[f"euler.{tag}.rec"], arrays[f"euler.{tag}.gt"] = rec, gt
        # the two places where one ulp changes a decision: the reference alone must stay clear of both
        near_singular = near_threshold = 0
        for seq in (rec, gt):
            for s in seq:
                full = dc.revert_output_format(s, mean, std, ignore)
                for frame in full:
                    for idx in range(3, 97, 3):
                        near_singular += int(abs(dc.expmap2rotmat(frame[idx:idx + 3])[0, 2]) > 0.999)
        values = []
        for r, g, a in zip(rec, gt, actions):                  # one sequence at a time: every row, whatever the cap would skip
            d = {x: {e: [] for e in HORIZONS} for x in ACTIONS}
            rmet.mse_euler(d, r[None], g[None], [a], mean, std, ignore, 10 ** 9)
            values.append([d[a][e][0] for e in HORIZONS])
            ge = dc.revert_output_format(g, mean, std, ignore)
            for frame in ge:
                for idx in range(3, 97, 3):
                    frame[idx:idx + 3] = dc.rotmat2euler(dc.expmap2rotmat(frame[idx:idx + 3]))
            ge[:, :6] = 0
            near_threshold += int(np.sum(np.abs(np.std(ge, 0) - 1e-4) < 1e-6))
        assert near_singular == 0 and near_threshold == 0, (tag, near_singular, near_threshold)
        arrays[f"euler.{tag}.values"] = np.asarray(values, dtype=np.float64)
        table = {x: {e: [] for e in HORIZONS} for x in ACTIONS}
        rmet.mse_euler(table, rec, gt, actions, mean, std, ignore, MAX_LEN)                   # the batch, with the cap
        arrays[f"euler.{tag}.table"] = np.asarray([[np.mean(table[x][e]) for e in HORIZONS] for x in ACTIONS])
        meta["euler"][tag] = {"actions": actions, "near_singular": near_singular, "near_threshold": near_threshold,
                              "list_lengths": {x: len(table[x][HORIZONS[0]]) for x in ACTIONS}}
        print(tag, meta["euler"][tag]["list_lengths"], arrays[f"euler.{tag}.table"].round(3).tolist())
    save("g12_pose_angles", meta, arrays)


if __name__ == "__main__":
    assert G.REF
    g12_pose_angles()
