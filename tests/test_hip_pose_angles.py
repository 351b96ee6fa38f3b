"""The angle-space pose path on the GPU (csrc/pose_angles.hip, pose_angles.py, render.AnglePoseCamera, BehaviorNet.evaluate's
``euler``): the kernels against the fixture the reference's own functions wrote (tests/golden/g12_pose_angles.npz) and against
the float64 restatement (tests/pose_angles_ref.py) at the evaluation sizes; the camera against the composition; one synthesised
video at the angle width; the evaluation keyword.

The bound.  The kernels compute in float64 and round once on the fp32 store, so with U = 2^-24 every element lies within
2 U max(1, |ref|) of the float64 reference: one fp32 rounding (<= U |ref|) plus float64 libm and summation-order differences,
orders of magnitude below it."""
import copy

import numpy as np
import pytest
import torch

import pose_angles_ref as R
from conftest import load_golden
from synth import seeded_randn, synth_behavior_state, synth_image, synth_state_dict

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _A():
    from behavior_driven_video_synthesis_amd import pose_angles
    return pose_angles


def _tree(arr, pos=True):
    return {"parent": arr["tree.parent"], "offset": arr["tree.offset"], "expmapInd": list(arr["tree.expmapInd"]),
            "posInd": {"ids": arr["tree.posInd"] if pos else None}}


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _held(got, ref, name, extra=0.0):
    """|got - ref| <= 2 U max(1, |ref|) (+ ``extra``, a derived input-propagation term) for every element; prints the figure."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    bound = 2 * U * np.maximum(1.0, np.abs(ref)) + extra
    err = np.abs(got - ref)
    worst = float(np.max(err / bound)) if err.size else 0.0
    print(f"{name}: max |got - ref| = {float(np.max(err)) if err.size else 0.0:.3e}, worst = {worst:.3f} of the bound")
    assert np.isfinite(got).all() and worst <= 1.0, (name, worst)


def _cuda(a):
    return torch.as_tensor(np.asarray(a)).cuda()


# ---- 1. kinematics and the root path against the fixture
@pytest.mark.parametrize("swap", [False, True])
def test_convert_to_3d_vs_the_fixture(swap):
    meta, arr = load_golden("g12_pose_angles")
    A = _A()
    tree = A.KinematicTree(_tree(arr))
    got = A.convert_to_3d(_cuda(arr["fk.angles"]), tree, swap)
    assert got.dtype == torch.float32 and tuple(got.shape) == (6, 20, 32, 3)
    _held(_np(got), arr[f"fk.xyz.swap{int(swap)}"], f"xyz swap_yz={swap}")
    one = A.convert_to_3d(_cuda(arr["fk.angles"][1, 4]), _tree(arr), swap)          # a single pose, the tree as the dataset's dict
    assert torch.equal(one, got[1, 4])


def test_convert_to_3d_normalised_and_without_root_translation_vs_the_fixture():
    meta, arr = load_golden("g12_pose_angles")
    A = _A()
    stats = A.AngleStats(arr["stats.mean"], arr["stats.std"], meta["ignore"])
    got = A.convert_to_3d(_cuda(arr["fk.normalised"]), _tree(arr), stats=stats)
    _held(_np(got), arr["fk.xyz.normalised"], "xyz from normalised output")
    got = A.convert_to_3d(_cuda(arr["fk.angles"][:2]), _tree(arr, pos=False))
    _held(_np(got), arr["fk.xyz.no_pos"], "xyz without posInd")
    with pytest.raises(ValueError):
        A.convert_to_3d(_cuda(arr["fk.angles"]), _tree(arr), stats=stats)            # 99 wide where 54 normalised are expected


@pytest.mark.parametrize("tag", ["identity", "moved"])
def test_revert_coordinate_space_vs_the_fixture(tag):
    meta, arr = load_golden("g12_pose_angles")
    A = _A()
    r0, t0 = (np.eye(3), np.zeros(3)) if tag == "identity" else (arr["revert.R0"], arr["revert.T0"])
    x = _cuda(arr["fk.angles"])
    got = A.revert_coordinate_space(x, r0, t0)
    assert got.dtype == torch.float32 and got.shape == x.shape
    _held(_np(got), arr[f"revert.{tag}"], f"revert {tag}")
    assert torch.equal(got[..., 6:], x[..., 6:])                                     # the other dimensions: copied
    one = A.revert_coordinate_space(x[3], torch.as_tensor(r0), torch.as_tensor(t0))  # [T, D], as the reference takes it
    assert torch.equal(one, got[3])


# ---- 2. the Euler error against the fixture
@pytest.mark.parametrize("tag", ["long", "short"])
def test_euler_error_vs_the_fixture(tag):
    meta, arr = load_golden("g12_pose_angles")
    A = _A()
    hz = meta["horizons"]
    stats = A.AngleStats(arr["stats.mean"], arr["stats.std"], meta["ignore"])
    got = A.euler_error(_cuda(arr[f"euler.{tag}.rec"]), _cuda(arr[f"euler.{tag}.gt"]), stats, hz)
    assert got.dtype == torch.float32 and got.is_cuda
    _held(_np(got), arr[f"euler.{tag}.values"], f"euler {tag}")
    n = got.shape[0]
    assert float(got[n // 2].abs().max()) == 0.0                                     # the sequence standing still
    table = A.EulerErrorTable(meta["actions"], hz, meta["max_len"])
    acts = meta["euler"][tag]["actions"]
    table.add(got[:3], acts[:3])
    table.add(got[3:], acts[3:])
    assert {a: v.shape[0] for a, v in table.lists().items()} == meta["euler"][tag]["list_lengths"]
    summ = table.summary()
    _held([[summ[a][e] for e in hz] for a in meta["actions"]], arr[f"euler.{tag}.table"], f"table {tag}")


# ---- 3. larger sizes against the restatement
def _angles(rng, b, t):
    axis = rng.randn(b, t, 32, 3)
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    x = np.concatenate([rng.randn(b, t, 3) * 40.0, (axis * (3.0 * rng.rand(b, t, 32, 1))).reshape(b, t, 96)], axis=-1)
    return x.astype(np.float32)


def _stats(rng, dtype):
    ignore = sorted((3 + rng.choice(96, size=45, replace=False)).tolist())
    mean = np.concatenate([rng.randn(3) * 300.0, rng.randn(96) * 0.3]).astype(dtype)
    std = np.concatenate([50.0 + 200.0 * rng.rand(3), 0.05 + 0.3 * rng.rand(96)]).astype(dtype)
    return mean, std, ignore


@pytest.mark.parametrize("b,t", [(64, 50), (800, 50), (70, 1), (1, 3)])
def test_kinematics_and_root_path_vs_the_restatement(b, t):
    meta, arr = load_golden("g12_pose_angles")
    A = _A()
    rng = np.random.RandomState(100 * b + t)
    x = _angles(rng, b, t)
    tree = A.KinematicTree(_tree(arr))
    got = A.convert_to_3d(_cuda(x), tree, swap_yz=True)
    _held(_np(got), R.forward_kinematics(x, _tree(arr), True), f"xyz {b}x{t}")
    r0 = R.rotmat_of_expmap(np.array([-0.9, 0.3, 1.4]))
    t0 = np.array([-40.0, 610.0, 75.0])
    got = A.revert_coordinate_space(_cuda(x), r0, t0)
    _held(_np(got), R.revert_root(x, r0, t0), f"revert {b}x{t}")


@pytest.mark.parametrize("dtype", ["float64", "float32"])
@pytest.mark.parametrize("b,t", [(64, 50), (800, 50), (70, 1), (3, 7)])
def test_normalised_kinematics_and_euler_error_vs_the_restatement(b, t, dtype):
    """Both statistics dtypes: float32 statistics put the un-normalisation (and only it) in float32, as the restatement does.
    Horizons past the sequence's end average the frames there are; T = 1 keeps no dimension (every deviation is 0)."""
    meta, arr = load_golden("g12_pose_angles")
    A = _A()
    rng = np.random.RandomState(7 * b + t + (dtype == "float32"))
    mean, std, ignore = _stats(rng, dtype)
    stats = A.AngleStats(mean, std, ignore)
    assert stats.f32_math == (dtype == "float32") and stats.n_use == 54
    gt = rng.randn(b, t, 54).astype(np.float32)
    gt[:, :, 20:26] = gt[:, :1, 20:26]                                               # dimensions that stand still
    if b > 2:
        gt[2] = gt[2, :1]
    rec = (gt + 0.25 * rng.randn(b, t, 54)).astype(np.float32)
    xyz = A.convert_to_3d(_cuda(rec), _tree(arr), stats=stats)
    _held(_np(xyz), R.forward_kinematics(R.unnormalise(rec, mean, std, ignore), _tree(arr)), f"xyz normalised {b}x{t} {dtype}")
    hz = [2, 4, 8, 10, 50, 64]
    got = A.euler_error(_cuda(rec), _cuda(gt), stats, hz)
    want = R.euler_error(rec, gt, mean, std, ignore, hz)
    _held(_np(got), want, f"euler {b}x{t} {dtype}")
    if t == 1:
        assert float(got.abs().max()) == 0.0
    if b > 2:
        assert float(got[2].abs().max()) == 0.0
    assert torch.equal(got[:, hz.index(64)], got[:, hz.index(50)]) or t > 50


def test_euler_error_refuses_a_sequence_that_does_not_fit():
    meta, arr = load_golden("g12_pose_angles")
    A = _A()
    stats = A.AngleStats(arr["stats.mean"], arr["stats.std"], meta["ignore"])
    x = torch.zeros(2, 77, 54, device="cuda")
    with pytest.raises(ValueError, match="LDS"):
        A.euler_error(x, x, stats, [2])
    assert tuple(A.euler_error(x[:, :76], x[:, :76], stats, [2, 80]).shape) == (2, 2)  # the longest that does


# ---- 4. the camera
def _camera(arr, meta, swap=False, stats_dtype="float64", spatial=256, image_size=(1000, 1002)):
    from behavior_driven_video_synthesis_amd.render import AnglePoseCamera
    ang = 0.4
    rot = np.array([[np.cos(ang), 0.0, np.sin(ang)], [0.0, 1.0, 0.0], [-np.sin(ang), 0.0, np.cos(ang)]])
    ext = np.concatenate([rot, np.array([[50.0], [-120.0], [5200.0]])], axis=1)      # the projection fixture's camera
    intr = (1145.0, 512.5, 1143.8, 515.4)
    mean, std = arr["stats.mean"].astype(stats_dtype), arr["stats.std"].astype(stats_dtype)
    use = [d for d in range(99) if d not in set(meta["ignore"])]
    cam = AnglePoseCamera(mean, std, use, _tree(arr), ext, intr, image_size, spatial, swap_yz=swap)
    return cam, (mean, std, ext, intr, image_size, spatial)


def _keypoints_held(kps, poses, arr, meta, swap, geo, name):
    """``kps`` against convert_to_3d on the restatement followed by the projection formulas.  The kernel's joints are fp32: within
    2 U max(1, |xyz|) of the restatement's (the kinematics bound above); ``project_bound`` carries that through the camera to
    first order (doubled for the higher orders), and the keypoints' own fp32 store adds the usual 2 U max(1, |ref|)."""
    mean, std, ext, intr, image_size, spatial = geo
    xyz = R.forward_kinematics(R.unnormalise(poses, mean, std, meta["ignore"]), _tree(arr), swap)
    ref = R.project(xyz, ext, intr, image_size, spatial)
    extra = 2 * R.project_bound(xyz, 2 * U * np.maximum(1.0, np.abs(xyz)), ext, intr, image_size, spatial)
    _held(kps, ref, name, extra=extra)
    return ref


@pytest.mark.parametrize("swap,stats_dtype", [(False, "float64"), (True, "float64"), (False, "float32")])
def test_angle_pose_camera_vs_the_composition(swap, stats_dtype):
    meta, arr = load_golden("g12_pose_angles")
    cam, geo = _camera(arr, meta, swap, stats_dtype)
    assert cam.spatial_size == 256 and cam.n_use == 54
    x = arr["fk.normalised"].reshape(-1, 54)
    got = cam.project(_cuda(x))
    assert got.dtype == torch.float32 and tuple(got.shape) == (120, 32, 2)
    ref = _keypoints_held(_np(got), x, arr, meta, swap, geo, f"keypoints swap_yz={swap} {stats_dtype}")
    assert np.ptp(ref) > 20                                                          # a figure, not a point
    with pytest.raises(ValueError):
        cam.project(torch.zeros(4, 51, device="cuda"))


# ---- 5. end to end at the angle width
def _behavior_state(mod, seed, scale_out=None):
    sd = mod.state_dict()
    stored = {k: v.cpu() for k, v in sd.items() if k.endswith("_shuffle_idx")}
    new = synth_behavior_state({k: list(v.shape) for k, v in sd.items()}, seed, stored)
    if scale_out is not None:
        new["decoder.n_out.weight"] = new["decoder.n_out.weight"] * scale_out
    mod.load_state_dict(new)
    return mod.cuda()


def test_behavior_video_with_an_angle_camera():
    """Config 5 for an ``angle_world_expmap`` model: flow sample -> roll-out at 54 dimensions -> un-normalise + kinematics ->
    camera -> raster -> VunetAlter.transfer.  The frames have the right shape; the keypoints are those of the returned poses."""
    from behavior_driven_video_synthesis_amd.models.flow.simple_flow import UnsupervisedTransformer2
    from behavior_driven_video_synthesis_amd.models.pose_behavior_rnn import ResidualBehaviorNet
    from behavior_driven_video_synthesis_amd.models.vunets import VunetAlter
    from behavior_driven_video_synthesis_amd.render import behavior_video
    meta, arr = load_golden("g12_pose_angles")
    torch.manual_seed(21)
    flow = _behavior_state(UnsupervisedTransformer2(flow_in_channels=64, flow_mid_channels=96, flow_hidden_depth=1, n_flows=2), 21)
    net = _behavior_state(ResidualBehaviorNet(54, information_bottleneck=True, decoder_arch="lstm", linear_in_decoder=False,
                                              dim_hidden_b=64), 21, scale_out=0.05)
    cfg = dict(spatial_size=64, bottleneck_factor=2, box_factor=2, n_scales=0, n_latent_scales=2, conv_layer_type="l1", nf_start=8,
               nf_max=16, subpixel_upsampling=True, dropout_prob=0.0)
    vunet = VunetAlter(**cfg)
    vunet.load_state_dict(synth_state_dict({k: list(v.shape) for k, v in vunet.state_dict().items()}, 21))
    vunet = vunet.cuda().eval()
    cam, geo = _camera(arr, meta, spatial=64, image_size=(1000, 1000))
    bsz, t_in, length = 2, 5, 6
    start = 0.5 * seeded_randn("angle.start", (bsz, t_in, 54), 21)
    z = seeded_randn("angle.z", (bsz, 64), 21)
    app = synth_image("angle.app", (1, 3, 64, 64), 21)
    frames, poses, kps = behavior_video(flow, net, vunet, app.cuda(), start.cuda(), length, cam, z=z.cuda(), dtype="f32",
                                        share_appearance=False)
    assert frames.shape == (bsz, length, 64, 64, 3) and frames.dtype == torch.uint8
    assert tuple(poses.shape) == (bsz, length, 54) and tuple(kps.shape) == (bsz, length, 32, 2)
    assert bool(torch.isfinite(poses).all())
    _keypoints_held(_np(kps), poses.cpu().numpy(), arr, meta, False, geo, "video keypoints")
    assert float(kps.min()) > -64 and float(kps.max()) < 128                          # the figure is on (or near) the canvas
    assert float(frames.float().std()) > 0


# ---- 6. BehaviorNet.evaluate(..., euler=...)
def test_evaluate_fills_the_euler_table_and_is_unchanged_without_it():
    from behavior_driven_video_synthesis_amd import behavior_eval as E
    from behavior_driven_video_synthesis_amd.experiments.behavior_net import BehaviorNet, DEFAULT_CONFIG
    meta, arr = load_golden("g12_pose_angles")
    A = _A()
    cfg = copy.deepcopy(DEFAULT_CONFIG)
    cfg["architecture"].update(dim_hidden_b=64, n_flows=2, flow_mid_channels_factor=2, flow_hidden_depth=1)
    torch.manual_seed(5)
    bn = BehaviorNet(cfg, n_kps=54, device="cuda:0", hip_graph=True)
    _behavior_state(bn.latent_flow, 5)
    _behavior_state(bn.net, 5, scale_out=0.05)
    bsz, t, skip, s = 8, 12, 4, 4
    acts = ["walking", "eating", "walking", "walking", "eating", "walking", "walking", "walking"]
    batches = [{"keypoints": (0.5 * seeded_randn(f"ev{i}.kps", (bsz, t + 1, 54), 5)).cuda(),
                "future_keypoints": (0.5 * seeded_randn(f"ev{i}.fut", (bsz, t + 1, 54), 5)).cuda(), "actions": acts} for i in range(2)]
    z = [seeded_randn(f"ev{i}.z", (s, bsz // skip, 64), 5).cuda() for i in range(2)]
    eps = [seeded_randn(f"ev{i}.eps", (bsz, 64), 5).cuda() for i in range(2)]
    pstats = E.PoseStats(arr["stats.mean"], arr["stats.std"], meta["ignore"])
    astats = A.AngleStats(arr["stats.mean"], arr["stats.std"], meta["ignore"])
    hz = meta["horizons"]
    plain = bn.evaluate(batches, pstats, n_samples=s, skip=skip, z=z, eps=eps)
    assert not hasattr(plain, "euler")
    ev = bn.evaluate(batches, pstats, n_samples=s, skip=skip, z=z, eps=eps, euler=(astats, hz, ["walking", "eating"], 8))
    assert ev.summary() == plain.summary()                                           # the sampling metrics do not move
    rows = []
    for b_, e_ in zip(batches, eps):
        x_s, target = b_["keypoints"][:, :-1].contiguous(), b_["keypoints"][:, 1:].contiguous()
        with torch.no_grad():
            rec = bn.net(x_s, x_s, t, eps=e_)[0]
        rows.append(R.euler_error(rec.cpu().numpy(), target.cpu().numpy(), arr["stats.mean"], arr["stats.std"], meta["ignore"], hz))
    want = R.table_summary(np.concatenate(rows), acts + acts, ["walking", "eating"], hz, 8)
    got = ev.euler.summary()
    assert {a: v.shape[0] for a, v in ev.euler.lists().items()} == {"walking": 9, "eating": 4}   # the cap: 9 of 12, 4 of 4
    for a in ("walking", "eating"):
        _held([got[a][e] for e in hz], [want[a][e] for e in hz], f"evaluate euler {a}")
    # without names every row counts under one action, and nothing is capped
    for b_ in batches:
        del b_["actions"]
    ev = bn.evaluate(batches, pstats, n_samples=s, skip=skip, z=z, eps=eps, euler=(astats, hz))
    assert list(ev.euler.lists()) == ["all"] and ev.euler.lists()["all"].shape == (2 * bsz, len(hz))
    _held(ev.euler.lists()["all"], np.concatenate(rows), "evaluate euler rows")
