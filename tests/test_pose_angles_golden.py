"""CPU checks of the angle-space pose path: the float64 restatement (tests/pose_angles_ref.py) against every array the
reference's own functions wrote (tests/golden/g12_pose_angles.npz), and the host-only parts of the public surface -- the cap
rule of ``EulerErrorTable``, the tree checks of ``KinematicTree``, and the argument checks that run before any device work."""
import ctypes
import os

import numpy as np
import pytest
import torch

import pose_angles_ref as R
from conftest import load_golden

TOL = dict(rtol=1e-12, atol=0)     # float64 rounding: both sides are float64 numpy, only the order of a few sums differs


def _tree(arr, pos=True):
    return {"parent": arr["tree.parent"], "offset": arr["tree.offset"], "expmapInd": list(arr["tree.expmapInd"]),
            "posInd": {"ids": arr["tree.posInd"] if pos else None}}


def _close(got, want, name):
    np.testing.assert_allclose(got, want, err_msg=name, **TOL)


def test_the_fixture_is_what_the_issue_describes():
    meta, arr = load_golden("g12_pose_angles")
    assert arr["tree.parent"].shape == (32,) and arr["tree.offset"].shape == (32, 3) and arr["tree.expmapInd"].shape == (32, 3)
    assert arr["fk.angles"].dtype == np.float32 and arr["fk.angles"].shape == (6, 20, 99)
    assert not arr["fk.angles"][0, 3].any()                                        # the all-zero pose
    mag = np.linalg.norm(arr["fk.angles"][..., 3:].reshape(6, 20, 32, 3), axis=-1)
    assert mag.max() > 2.9 and mag.min() == 0.0
    assert arr["stats.mean"].dtype == np.float64 and len(meta["ignore"]) == 45
    for tag, info in meta["euler"].items():
        assert info["near_singular"] == 0 and info["near_threshold"] == 0          # the two 1-ulp decisions: clear of both
    assert meta["euler"]["long"]["list_lengths"]["walking"] == meta["max_len"] + 1   # the cap triggered
    assert meta["revert_non_unit_quaternions"] == 0


@pytest.mark.parametrize("swap", [False, True])
def test_restatement_reproduces_convert_to_3d(swap):
    meta, arr = load_golden("g12_pose_angles")
    got = R.forward_kinematics(arr["fk.angles"], _tree(arr), swap)
    assert got.dtype == np.float64 and got.shape == (6, 20, 32, 3)
    _close(got, arr[f"fk.xyz.swap{int(swap)}"], "xyz")
    np.testing.assert_array_equal(got[0, 3], R.forward_kinematics(np.zeros(99), _tree(arr), swap))


def test_restatement_reproduces_the_normalised_and_rootless_variants():
    meta, arr = load_golden("g12_pose_angles")
    full = R.unnormalise(arr["fk.normalised"], arr["stats.mean"], arr["stats.std"], meta["ignore"])
    assert full.shape == (6, 20, 99)
    np.testing.assert_array_equal(full[..., meta["ignore"]], np.broadcast_to(arr["stats.mean"][meta["ignore"]], (6, 20, 45)))
    _close(R.forward_kinematics(full, _tree(arr)), arr["fk.xyz.normalised"], "normalised")
    _close(R.forward_kinematics(arr["fk.angles"][:2], _tree(arr, pos=False)), arr["fk.xyz.no_pos"], "no_pos")


@pytest.mark.parametrize("tag", ["identity", "moved"])
def test_restatement_reproduces_revert_coordinate_space(tag):
    meta, arr = load_golden("g12_pose_angles")
    r0, t0 = (np.eye(3), np.zeros(3)) if tag == "identity" else (arr["revert.R0"], arr["revert.T0"])
    got = R.revert_root(arr["fk.angles"], r0, t0)
    _close(got[..., :3], arr[f"revert.{tag}"][..., :3], "translation")
    _close(got[..., 3:6], arr[f"revert.{tag}"][..., 3:6], "rotation")
    np.testing.assert_array_equal(got[..., 6:], arr["fk.angles"][..., 6:].astype(np.float64))
    # one sequence at a time gives the same: the batch axis is independent
    np.testing.assert_array_equal(R.revert_root(arr["fk.angles"][2], r0, t0), got[2])


@pytest.mark.parametrize("tag", ["long", "short"])
def test_restatement_reproduces_mse_euler(tag):
    meta, arr = load_golden("g12_pose_angles")
    hz = meta["horizons"]
    got = R.euler_error(arr[f"euler.{tag}.rec"], arr[f"euler.{tag}.gt"], arr["stats.mean"], arr["stats.std"], meta["ignore"], hz)
    np.testing.assert_allclose(got, arr[f"euler.{tag}.values"], **TOL)
    n = got.shape[0]
    assert (got[n // 2] == 0).all() and (np.delete(got, n // 2, axis=0) > 0).all()    # the sequence standing still keeps nothing
    if tag == "short":                                                               # 9 frames: [:10] is [:9]
        want9 = R.euler_error(arr["euler.short.rec"], arr["euler.short.gt"], arr["stats.mean"], arr["stats.std"], meta["ignore"], [9])
        np.testing.assert_array_equal(got[:, hz.index(10)], want9[:, 0])
    table = R.table_summary(got, meta["euler"][tag]["actions"], meta["actions"], hz, meta["max_len"])
    want = arr[f"euler.{tag}.table"]
    for ai, a in enumerate(meta["actions"]):
        np.testing.assert_allclose([table[a][e] for e in hz], want[ai], err_msg=a, **TOL)


def test_euler_conversion_keeps_the_gimbal_branch():
    """R[0, 2] exactly +-1: the third angle is 0 and the second is -+pi / 2, as the reference's special case."""
    for s in (1.0, -1.0):
        m = np.array([[0.0, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, 0.0]])
        e = R.euler_of_rotmat(m)
        assert e[2] == 0.0 and e[1] == -s * np.pi / 2 and e[0] == np.arctan2(0.0, s)
    np.testing.assert_array_equal(R.euler_of_rotmat(np.eye(3)), np.zeros(3))


def test_error_table_cap_is_the_references():
    """A sequence is skipped once its action's list ALREADY holds more than max_len entries: lists end at max_len + 1."""
    from behavior_driven_video_synthesis_amd.pose_angles import EulerErrorTable
    meta, arr = load_golden("g12_pose_angles")
    hz, acts = meta["horizons"], meta["euler"]["long"]["actions"]
    values = torch.as_tensor(arr["euler.long.values"])
    tab = EulerErrorTable(meta["actions"], hz, meta["max_len"])
    tab.add(values[:4], acts[:4])                       # two calls: the cap counts across them
    tab.add(values[4:], acts[4:])
    assert {a: v.shape[0] for a, v in tab.lists().items()} == meta["euler"]["long"]["list_lengths"]
    assert tab.counts["walking"] == meta["max_len"] + 1
    got = tab.summary()
    for ai, a in enumerate(meta["actions"]):
        np.testing.assert_allclose([got[a][e] for e in hz], arr["euler.long.table"][ai], err_msg=a, **TOL)
    with pytest.raises(KeyError):
        tab.add(values[:1], ["dancing"])
    with pytest.raises(ValueError):
        tab.add(values[:2], acts[:1])
    empty = EulerErrorTable(["sitting"], hz, 3).summary()
    assert all(np.isnan(v) for v in empty["sitting"].values())
    free = EulerErrorTable(None, hz, 0)                 # names taken as they come; max_len 0 keeps one entry per action
    free.add(values, acts)
    assert {a: v.shape[0] for a, v in free.lists().items()} == {"walking": 1, "eating": 1}


def test_kinematic_tree_rejects_a_child_before_its_parent():
    from behavior_driven_video_synthesis_amd.pose_angles import AngleStats, KinematicTree
    meta, arr = load_golden("g12_pose_angles")
    tree = KinematicTree(_tree(arr), device="cpu")
    assert tree.n_joints == 32 and tree.min_dim == 99 and tree.parent.dtype == torch.int32 and tree.offset.dtype == torch.float64
    assert KinematicTree(_tree(arr, pos=False), device="cpu").pos_ind is None
    # the same skeleton with two joints renumbered, every table permuted alike: joint 2's parent now comes after it
    perm = np.arange(32)
    perm[[1, 2]] = [2, 1]
    inv = np.argsort(perm)
    parent = arr["tree.parent"][perm]
    shuffled = {"parent": np.where(parent >= 0, inv[np.maximum(parent, 0)], -1), "offset": arr["tree.offset"][perm],
                "expmapInd": list(arr["tree.expmapInd"][perm]), "posInd": {"ids": arr["tree.posInd"]}}
    with pytest.raises(ValueError, match="parents must precede"):
        KinematicTree(shuffled, device="cpu")
    with pytest.raises(AssertionError):
        R.forward_kinematics(arr["fk.angles"][0], shuffled)
    with pytest.raises(ValueError, match="bone vectors"):
        KinematicTree(dict(_tree(arr), offset=arr["tree.offset"][:31]), device="cpu")
    stats = AngleStats(arr["stats.mean"], arr["stats.std"], meta["ignore"], device="cpu")
    assert (stats.dim, stats.n_use, stats.f32_math) == (99, 54, 0)
    pos = stats.pos_of_dim.numpy()
    assert (pos[meta["ignore"]] == -1).all() and sorted(pos[pos >= 0].tolist()) == list(range(54))
    same = AngleStats.from_dim_to_use(arr["stats.mean"].astype(np.float32), arr["stats.std"].astype(np.float32),
                                      np.nonzero(pos >= 0)[0], device="cpu")
    assert same.f32_math == 1 and torch.equal(same.pos_of_dim, stats.pos_of_dim)


def test_the_public_surface_refuses_the_cpu_and_bad_arguments():
    from behavior_driven_video_synthesis_amd import _lib
    from behavior_driven_video_synthesis_amd import pose_angles as A
    meta, arr = load_golden("g12_pose_angles")
    stats = A.AngleStats(arr["stats.mean"], arr["stats.std"], meta["ignore"], device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.convert_to_3d(torch.zeros(2, 99), _tree(arr))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.revert_coordinate_space(torch.zeros(2, 99), np.eye(3), np.zeros(3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        A.euler_error(torch.zeros(2, 3, 54), torch.zeros(2, 3, 54), stats, [2])
    with pytest.raises(ValueError, match="horizons"):
        A.euler_error(torch.zeros(2, 3, 54), torch.zeros(2, 3, 54), stats, [0, 2])
    with pytest.raises(ValueError):
        A.euler_error(torch.zeros(2, 3, 51), torch.zeros(2, 3, 51), stats, [2])
    with pytest.raises(ValueError):
        A.revert_coordinate_space(torch.zeros(2, 5), np.eye(3), np.zeros(3))
    # the C ABI checks its arguments before any launch (the pointers are never dereferenced)
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib, f = _lib.lib(), ctypes.c_void_p(256)
    assert lib.vunet_pose_fk(f, 99, None, None, None, 0, 99, f, f, f, f, 33, 0, f, 4, None) == -1        # J > 32
    assert lib.vunet_pose_fk(f, 54, f, None, f, 0, 99, f, f, f, f, 32, 0, f, 4, None) == -1             # statistics missing
    assert lib.vunet_pose_fk(f, 54, None, None, None, 0, 99, f, f, f, f, 32, 0, f, 4, None) == -1        # rows shorter than D
    assert lib.vunet_pose_revert_root(f, f, f, f, 2, 3, 5, None) == -1                                  # D < 6
    assert lib.vunet_pose_revert_root(f, None, f, f, 2, 3, 99, None) == -1
    assert lib.vunet_pose_euler_error(f, f, 54, f, f, f, 0, 98, f, 4, f, 2, 3, None) == -1              # D % 3
    assert lib.vunet_pose_euler_error(f, f, 54, f, f, f, 0, 99, f, 0, f, 2, 3, None) == -1              # no horizon
    assert lib.vunet_pose_euler_error(f, f, 54, f, f, f, 0, 99, f, 4, f, 2, 77, None) == -3             # one sequence exceeds LDS
