/*
 * vunet_pose_angles.h -- C ABI of the angle-space pose path (keypoint_type ``angle_world_expmap``), csrc/pose_angles.hip.  Part of
 * libvunet_hip.so; same conventions as vunet_hip.h (plain pointers and sizes, caller-owned device buffers, `stream` =
 * hipStream_t as void*, 0 or a negative VUNET_ERR_* code).  Additive entry points within ABI 12.
 *
 * What it replaces in the reference (CompVis/behavior-driven-video-synthesis, paths relative to the upstream root):
 *   data/data_conversions_3d.py:1047-1066    convert_to_3d: fkl per frame, the optional y/z swap
 *   data/data_conversions_3d.py:608-668      fkl (use_euler=False): the forward-kinematics chain over the joints
 *   data/data_conversions_3d.py:671-703      revert_coordinate_space: the root's rotation and translation accumulated over the frames
 *   data/data_conversions_3d.py:56-175       rotmat2euler, quat2expmap, rotmat2quat, expmap2rotmat
 *   data/data_conversions_3d.py:178-211      unNormalizeData
 *   lib/metrics.py:321-357                   mse_euler: the per-sequence arithmetic
 *
 * All three compute in float64 and round once, on the fp32 store.  The skeleton is an argument, never a constant of the library.
 *
 * Pose vectors.  A pose is D numbers (D = 99 for H3.6M: 3 of root translation, then exponential-map triples).  Where a
 * function takes ``pos_of_dim``, x holds NORMALISED vectors of n_use used dimensions (row stride ldx) and pos_of_dim[d] is the
 * column of dimension d in x, or -1 for an ignored dimension, which holds 0 * std + mean; mean / stdv are D DEVICE doubles.
 * f32_math != 0: x * std + mean in float32 (numpy's promotion when the statistics are float32 arrays), else float64.  With
 * pos_of_dim NULL (vunet_pose_fk only), x holds un-normalised vectors of D numbers and mean / stdv are not read.
 *
 * vunet_pose_fk           x: T poses -> xyz [T][J][3] fp32.  parent [J] int32 (-1: a root; every other entry must be smaller
 *                         than its own index: the walk is in index order), offset [J][3] doubles, expmap_ind [J][3] int32 (the
 *                         dimensions of joint j's exponential map), pos_ind [3] int32 or NULL (the root's translation; NULL:
 *                         zero), all DEVICE arrays; the caller has checked the index tables against D and the parent order.
 *                         R_j = I + sin(t) K + (1 - cos(t)) K K with t = |r|, K the cross-product matrix of r / (t + eps(float32)).
 *                         Root: xyz = offset + translation, rotation = R_j.  Child: xyz = offset . R_parent + xyz_parent (a row
 *                         vector times the matrix), rotation = R_j . R_parent.  swap_yz != 0 stores (x, z, y).  One lane per pose.
 *                         1 <= J <= VUNET_POSE_MAX_JOINTS.
 * vunet_pose_revert_root  ch [B][T][D] fp32 un-normalised -> out [B][T][D] fp32: dimensions 6 .. D-1 copied; with R_prev = R0
 *                         (r0: 9 DEVICE doubles, row-major) and T_prev = T0 (t0: 3 DEVICE doubles), per frame R = R(ch[3..5]) . R_prev,
 *                         out[3..5] = quat2expmap(rotmat2quat(R)) (the float32 eps in both divisions, theta mod 2 pi, the flip for
 *                         theta > pi), out[0..2] = T = T_prev + R_prev^T ch[0..2]; then R_prev = R, T_prev = T, carried in
 *                         float64.  One lane per sequence, sequential in T.  D >= 6.
 * vunet_pose_euler_error  rec, gt [B][T][n_use] fp32 normalised -> out [B][n_h] fp32.  Both un-normalised to D dimensions; every
 *                         triple (3, 4, 5), (6, 7, 8), ... of both replaced by rotmat2euler(expmap2rotmat(.)), its R[0][2] == +-1
 *                         branch included; dimensions 0 .. 5 of gt (NOT of rec) set to 0; kept = the dimensions whose population
 *                         standard deviation of gt over the T frames exceeds 1e-4; n_t = sqrt(sum over kept of (gt - rec)^2);
 *                         out[b][h] = mean of n_t over the first min(horizons[h], T) frames.  horizons: n_h DEVICE int32, each
 *                         >= 1 (checked by the caller).  One workgroup per sequence, fixed summation orders, no atomics.
 *                         D % 3 == 0, D >= 6, 1 <= n_h <= 256; the LDS image bounds the size: D <= VUNET_POSE_EULER_MAX_D and
 *                         T (D + 1) <= VUNET_POSE_EULER_MAX_TD, else VUNET_ERR_UNSUPPORTED (T <= 76 at D = 99).
 * All: no NULL pointer except where said, sizes >= 1, else VUNET_ERR_ARG.
 */
#ifndef VUNET_POSE_ANGLES_H
#define VUNET_POSE_ANGLES_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VUNET_POSE_MAX_JOINTS 32
#define VUNET_POSE_EULER_MAX_D 512
#define VUNET_POSE_EULER_MAX_TD 7680

int vunet_pose_fk(const float* x, int32_t ldx, const int32_t* pos_of_dim, const double* mean, const double* stdv, int32_t f32_math,
                  int32_t D, const int32_t* parent, const double* offset, const int32_t* expmap_ind, const int32_t* pos_ind, int32_t J,
                  int32_t swap_yz, float* xyz, int32_t T, void* stream);

int vunet_pose_revert_root(const float* ch, const double* r0, const double* t0, float* out, int32_t B, int32_t T, int32_t D,
                           void* stream);

int vunet_pose_euler_error(const float* rec, const float* gt, int32_t n_use, const int32_t* pos_of_dim, const double* mean,
                           const double* stdv, int32_t f32_math, int32_t D, const int32_t* horizons, int32_t n_h, float* out, int32_t B,
                           int32_t T, void* stream);

#ifdef __cplusplus
}
#endif
#endif
