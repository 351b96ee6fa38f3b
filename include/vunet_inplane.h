/*
 * vunet_inplane.h -- C ABI of the part-normalised appearance input (``data: inplane_normalize: True``), csrc/inplane.hip.  Part of
 * libvunet_hip.so; same conventions as vunet_hip.h (plain pointers and sizes, caller-owned device buffers, `stream` =
 * hipStream_t as void*, 0 or a negative VUNET_ERR_* code).  Additive entry points within ABI 12.
 *
 * What it replaces in the reference (CompVis/behavior-driven-video-synthesis, paths relative to the upstream root):
 *   lib/utils.py:70-232            t5p, t4p, t3p, t2p: the four source points of a body part and cv2.getPerspectiveTransform
 *   lib/utils.py:515-517           valid_joints
 *   data/base_dataset.py:685-725   _get_pose_img_inplane: one cv2.warpPerspective(BORDER_REPLICATE) per part, stacked on channels
 *
 * A part is (kind, joint ids).  kinds [P] int32 and ids [P][VUNET_INPLANE_MAX_IDS] int32 are DEVICE arrays; unused id slots are
 * not read.  An id outside [0, J) makes the part absent (nothing is read out of bounds).  k(i) below is keypoint ids[i] as (x, y).
 *   VUNET_INPLANE_T4P  4 ids.  source = k(0) k(1) k(2) k(3); destination (0,0) (wh,0) (wh,wh) (0,wh).
 *   VUNET_INPLANE_T5P  5 ids (right hip, right shoulder, neck, left shoulder, left hip).  With ls_to_rs = k(1) - k(3),
 *                      rh_to_rs = k(1) - k(0), lh_to_ls = k(3) - k(4): the two upper corners are neck + lambda_r ls_to_rs and
 *                      neck + lambda_l ls_to_rs (lambda as at :85-94), the lower ones k(4), k(0); destination as T4P.
 *   VUNET_INPLANE_T3P  3 ids (right shoulder, left shoulder, head).  All six coordinates >= 0: neck = (k(0) + k(1)) / 2,
 *                      p0 = neck + 2 (k(2) - neck), p1 = neck, normal n = (-(p1 - p0).y, (p1 - p0).x), a = p0 + n/2, b = p0 - n/2,
 *                      c = p1 - n/2, d = p1 + n/2.  Else, with both shoulders >= 0 (absent otherwise): seg = k(0) - k(1),
 *                      n = (-seg.y, seg.x), negated if n.y > 0; a = k(1) + n, b = k(1), c = k(0), d = k(0) + n.
 *                      source = b c d a; destination (0,0) (0,wh) (wh,wh) (wh,0).
 *   VUNET_INPLANE_T2P  2 ids.  No joint with both coordinates <= 0: p0 = k(0), p1 = k(1).  Else the one joint t with both
 *                      coordinates > 0 (absent if there is none): p0 = k(t), p1 = (k(t).x, oh - 1).  n as above, a = p0 + n/4,
 *                      b = p0 - n/4, c = p1 - n/4, d = p1 + n/4.  source = a b c d; destination (0,0) (0,wh) (wh,wh) (wh,0), each
 *                      coordinate minus 1 (``np.multiply(dst, wh) - 1.0``, :228): (-1,-1) (-1,wh-1) (wh-1,wh-1) (wh-1,-1).
 * wh = s_out for both axes.  Every number is float64 from the fp32 keypoints (the reference rounds the points to float32 first).
 *
 * vunet_inplane_transforms  kps [N][J][2] fp32 -> minv [N][P][9] doubles (row-major 3x3, destination -> source), src [N][P][4][2]
 *                           doubles (the source points in the order above; zeros where the builder returns None) and valid
 *                           [N][P] int32.  The eight-unknown system of cv2.getPerspectiveTransform (bottom-right entry 1) is
 *                           solved by Gaussian elimination with partial pivoting and the 3x3 inverted by its adjugate over the
 *                           determinant.  valid = 0 where the builder returns None, where a source point, a pivot or the determinant is not
 *                           finite (or the determinant is 0), or where a pivot's magnitude is below 1e-9 times the largest
 *                           magnitude in the 8x8 matrix; minv is then nine zeros.  One thread per (image, part).
 * vunet_inplane_warp        img [N][3][Hs][Ws] fp32, minv, valid -> out [N][3 P][s_out][s_out] fp32, part p in channels 3p .. 3p+2.
 *                           Output pixel (x, y): (u, v, w) = minv (x, y, 1) in float64; w == 0 samples (0, 0); else the bilinear
 *                           sample at (u/w, v/w), pixel centres at integers, the coordinate clamped to [0, Ws-1] x [0, Hs-1];
 *                           weights and blend in fp32 (top = a + fx (b - a), bottom alike, out = top + fy (bottom - top)).
 *                           valid == 0 fills `absent`.
 *                           One thread per output pixel serves the three channels.  N <= 65535.
 * Both: no allocation, no synchronisation; no NULL pointer, sizes >= 1, 1 <= P <= VUNET_INPLANE_MAX_PARTS, else VUNET_ERR_ARG.
 */
#ifndef VUNET_INPLANE_H
#define VUNET_INPLANE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VUNET_INPLANE_T2P 2
#define VUNET_INPLANE_T3P 3
#define VUNET_INPLANE_T4P 4
#define VUNET_INPLANE_T5P 5
#define VUNET_INPLANE_MAX_IDS 5
#define VUNET_INPLANE_MAX_PARTS 64

int vunet_inplane_transforms(const float* kps, int32_t N, int32_t J, const int32_t* kinds, const int32_t* ids, int32_t P,
                             int32_t s_out, double oh, double* minv, double* src, int32_t* valid, void* stream);

int vunet_inplane_warp(const float* img, int32_t N, int32_t Hs, int32_t Ws, const double* minv, const int32_t* valid, int32_t P,
                       int32_t s_out, float absent, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
