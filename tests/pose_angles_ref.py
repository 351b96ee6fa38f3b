"""Plain numpy restatement, in float64, of what csrc/pose_angles.hip computes: the exponential-map conversions, forward
kinematics over a given tree, the root's accumulated path and the Euler-angle error of a reconstruction.  Vectorised over the
leading axes; the tree, the statistics and the horizons are arguments.  tests/test_pose_angles_golden.py holds it to the arrays
the reference's own functions wrote (tests/golden/g12_pose_angles.npz); the GPU tests use it for sizes the fixture lacks."""
import numpy as np

EPS32 = float(np.finfo(np.float32).eps)


def unnormalise(x, mean, std, dims_to_ignore):
    """[..., n_use] normalised -> [..., D] float64: used dimensions x * std + mean, ignored ones 0 * std + mean; in float32
    when both statistics are float32 arrays (numpy's promotion), else float64."""
    mean, std = np.asarray(mean), np.asarray(std)
    f32 = mean.dtype == np.float32 and std.dtype == np.float32
    dt = np.float32 if f32 else np.float64
    ignore = {int(d) for d in np.asarray(dims_to_ignore).reshape(-1)}
    use = [d for d in range(mean.size) if d not in ignore]
    x = np.asarray(x, dtype=np.float32)
    full = np.zeros(x.shape[:-1] + (mean.size,), dtype=dt)
    full[..., use] = x
    return (full * std.astype(dt) + mean.astype(dt)).astype(np.float64)


def rotmat_of_expmap(r):
    """[..., 3] -> [..., 3, 3]: I + sin(t) K + (1 - cos(t)) K K, K the cross-product matrix of r / (|r| + eps32)."""
    r = np.asarray(r, dtype=np.float64)
    theta = np.sqrt(np.sum(r * r, axis=-1))
    a = r / (theta + EPS32)[..., None]
    k = np.zeros(r.shape[:-1] + (3, 3))
    k[..., 0, 1], k[..., 0, 2] = -a[..., 2], a[..., 1]
    k[..., 1, 0], k[..., 1, 2] = a[..., 2], -a[..., 0]
    k[..., 2, 0], k[..., 2, 1] = -a[..., 1], a[..., 0]
    return np.eye(3) + np.sin(theta)[..., None, None] * k + (1.0 - np.cos(theta))[..., None, None] * (k @ k)


def euler_of_rotmat(m):
    """[..., 3, 3] -> [..., 3] Euler angles; where m[0, 2] is exactly +-1 the third angle is 0 and the first takes the rest."""
    m = np.asarray(m, dtype=np.float64)
    s = m[..., 0, 2]
    lock = (s == 1.0) | (s == -1.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        e2 = -np.arcsin(s)
        c = np.cos(e2)
        e1 = np.arctan2(m[..., 1, 2] / c, m[..., 2, 2] / c)
        e3 = np.arctan2(m[..., 0, 1] / c, m[..., 0, 0] / c)
    e1 = np.where(lock, np.arctan2(m[..., 0, 1], s), e1)
    e2 = np.where(lock, np.where(s == -1.0, np.pi / 2, -np.pi / 2), e2)
    e3 = np.where(lock, 0.0, e3)
    return np.stack([e1, e2, e3], axis=-1)


def expmap_of_rotmat(m):
    """[..., 3, 3] -> [..., 3] through the quaternion: axis from m - m^T over (its norm + eps32), angle from atan2(norm / 2,
    (trace - 1) / 2); then axis over (norm + eps32) again, angle 2 atan2 taken mod 2 pi and folded into [0, pi] with a sign flip."""
    m = np.asarray(m, dtype=np.float64)
    ax = np.stack([m[..., 2, 1] - m[..., 1, 2], m[..., 0, 2] - m[..., 2, 0], m[..., 1, 0] - m[..., 0, 1]], axis=-1)
    an = np.sqrt(np.sum(ax * ax, axis=-1))
    half = np.arctan2(an / 2, (np.trace(m, axis1=-2, axis2=-1) - 1.0) / 2) / 2
    q0 = np.cos(half)
    qv = ax / (an + EPS32)[..., None] * np.sin(half)[..., None]
    qn = np.sqrt(np.sum(qv * qv, axis=-1))
    axis = qv / (qn + EPS32)[..., None]
    theta = np.mod(2 * np.arctan2(qn, q0) + 2 * np.pi, 2 * np.pi)
    flip = theta > np.pi
    theta = np.where(flip, 2 * np.pi - theta, theta)
    axis = np.where(flip[..., None], -axis, axis)
    return axis * theta[..., None]


def tree_arrays(tree):
    """The reference's tree dict -> (parent [J], offset [J, 3], expmap_ind [J, 3], pos_ind [3] or None)."""
    parent = np.asarray(tree["parent"]).astype(np.int64).reshape(-1)
    j = parent.size
    offset = np.asarray(tree["offset"], dtype=np.float64).reshape(j, 3)
    expmap = np.asarray([np.asarray(e) for e in tree["expmapInd"]]).astype(np.int64).reshape(j, 3)
    pos = tree.get("posInd")
    ids = None if pos is None else (pos["ids"] if isinstance(pos, dict) else pos)
    return parent, offset, expmap, None if ids is None else np.asarray(ids).astype(np.int64).reshape(3)


def forward_kinematics(angles, tree, swap_yz=False):
    """[..., D] un-normalised angle vectors -> [..., J, 3] joint positions, walking the tree in index order."""
    parent, offset, expmap, pos_ind = tree_arrays(tree)
    a = np.asarray(angles, dtype=np.float64)
    j = parent.size
    rot = rotmat_of_expmap(a[..., expmap])                       # [..., J, 3, 3]
    xyz = np.zeros(a.shape[:-1] + (j, 3))
    world = np.zeros_like(rot)
    for i in range(j):
        p = int(parent[i])
        if p < 0:
            xyz[..., i, :] = offset[i] + (a[..., pos_ind] if pos_ind is not None else 0.0)
            world[..., i, :, :] = rot[..., i, :, :]
        else:
            assert p < i, "parents must precede their children"
            xyz[..., i, :] = np.einsum("r,...rc->...c", offset[i], world[..., p, :, :]) + xyz[..., p, :]
            world[..., i, :, :] = rot[..., i, :, :] @ world[..., p, :, :]
    return xyz[..., [0, 2, 1]] if swap_yz else xyz


def revert_root(channels, r0, t0):
    """[..., T, D] -> [..., T, D] float64: the root's rotation (dimensions 3..5) and translation (0..2) accumulated over the frames
    from (r0, t0); the other dimensions are copied."""
    ch = np.asarray(channels, dtype=np.float64)
    out = ch.copy()
    lead = ch.shape[:-2]
    r_prev = np.broadcast_to(np.asarray(r0, dtype=np.float64).reshape(3, 3), lead + (3, 3)).copy()
    t_prev = np.broadcast_to(np.asarray(t0, dtype=np.float64).reshape(3), lead + (3,)).copy()
    for t in range(ch.shape[-2]):
        r = rotmat_of_expmap(ch[..., t, 3:6]) @ r_prev
        out[..., t, 3:6] = expmap_of_rotmat(r)
        t_prev = t_prev + np.einsum("...rc,...r->...c", r_prev, ch[..., t, :3])
        out[..., t, :3] = t_prev
        r_prev = r
    return out


def euler_error(rec, gt, mean, std, dims_to_ignore, horizons):
    """rec, gt [B, T, n_use] normalised -> [B, n_horizons] float64.  Both un-normalised; every triple from dimension 3 on turned
    into Euler angles; the first six dimensions of gt (not of rec) zeroed; the dimensions whose gt deviation over the frames
    (population) exceeds 1e-4 kept; per frame the norm of gt - rec over those; per horizon e the mean over frames [:e]."""
    g = unnormalise(gt, mean, std, dims_to_ignore)
    r = unnormalise(rec, mean, std, dims_to_ignore)
    b, t, d = g.shape
    for a in (g, r):
        tri = a[..., 3:].reshape(b, t, -1, 3)
        a[..., 3:] = euler_of_rotmat(rotmat_of_expmap(tri)).reshape(b, t, -1)
    g[..., :6] = 0.0
    out = np.zeros((b, len(horizons)))
    for i in range(b):
        kept = np.std(g[i], axis=0) > 1e-4
        per_frame = np.sqrt(np.sum((g[i][:, kept] - r[i][:, kept]) ** 2, axis=1))
        for h, e in enumerate(horizons):
            out[i, h] = np.mean(per_frame[:e])
    return out


def table_summary(values, actions, all_actions, horizons, max_len):
    """The reference's per-action lists with its cap: a sequence is skipped once its action's list already holds MORE than
    max_len entries (so a list ends with max_len + 1).  -> {action: {horizon: mean}}, NaN for an action that got nothing."""
    lists = {a: [] for a in all_actions}
    for row, a in zip(np.asarray(values, dtype=np.float64), actions):
        if len(lists[a]) > max_len:
            continue
        lists[a].append(row)
    return {a: {int(e): (float(np.mean([r[h] for r in rows])) if rows else float("nan")) for h, e in enumerate(horizons)}
            for a, rows in lists.items()}


def project(xyz, extrinsics, intrinsics, image_size, spatial_size):
    """[..., J, 3] world joints -> [..., J, 2] pixel keypoints at the synthesis resolution, the formulas of the projection
    fixture (g9b_projection): [R | t] (x, 1), the pinhole camera (f_x, x_0, f_y, y_0) on (x, y) / z, the rescale by
    spatial_size / image_size.  float64."""
    xyz = np.asarray(xyz, dtype=np.float64)
    ext = np.asarray(extrinsics, dtype=np.float64).reshape(3, 4)
    c = xyz @ ext[:, :3].T + ext[:, 3]
    fx, x0, fy, y0 = [float(v) for v in intrinsics]
    u = c[..., 0] / c[..., 2] * fx + x0
    v = c[..., 1] / c[..., 2] * fy + y0
    return np.stack([u * (float(spatial_size) / image_size[0]), v * (float(spatial_size) / image_size[1])], axis=-1)


def project_bound(xyz, d_xyz, extrinsics, intrinsics, image_size, spatial_size):
    """How far ``project`` moves, to first order, when every coordinate of xyz moves by at most d_xyz: |dc_r| <= sum_k |R_rk|
    d_k through the extrinsics, then |du| <= s f (|dc_x| / |c_z| + |c_x| |dc_z| / c_z^2) through the division."""
    xyz, d_xyz = np.asarray(xyz, dtype=np.float64), np.asarray(d_xyz, dtype=np.float64)
    ext = np.asarray(extrinsics, dtype=np.float64).reshape(3, 4)
    c = xyz @ ext[:, :3].T + ext[:, 3]
    dc = d_xyz @ np.abs(ext[:, :3]).T
    fx, _, fy, _ = [float(v) for v in intrinsics]
    z = np.abs(c[..., 2])
    du = fx * (dc[..., 0] / z + np.abs(c[..., 0]) * dc[..., 2] / z ** 2) * (float(spatial_size) / image_size[0])
    dv = fy * (dc[..., 1] / z + np.abs(c[..., 1]) * dc[..., 2] / z ** 2) * (float(spatial_size) / image_size[1])
    return np.stack([du, dv], axis=-1)
