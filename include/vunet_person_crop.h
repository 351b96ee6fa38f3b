/*
 * vunet_person_crop.h -- C ABI of the person-box crop of run_inference ("IS on masks"), csrc/person_crop.hip.  Part of
 * libvunet_hip.so; same conventions as vunet_hip.h (plain pointers and sizes, caller-owned device buffers, `stream` =
 * hipStream_t as void*, 0 or a negative VUNET_ERR_* code).  Additive entry points within ABI 12.
 *
 * What it replaces in the reference (CompVis/behavior-driven-video-synthesis, paths relative to the upstream root):
 *   lib/utils.py:560-585                    bb_for_pt_kornia: cv2.boundingRect of the valid keypoints, as four corners
 *   lib/utils.py:530-558                    bounding_box_batch: one kp.cpu().numpy() per image, then kornia.crop_and_resize
 *   experiments/shape_and_pose_net.py:888-891  the crop of every reconstruction and transfer before the Inception score
 *   lib/metrics.py:385                      nn.Upsample(299, bilinear) of those crops (vunet_inception_input_boxes)
 *
 * vunet_kp_boxes   kps [N][J][C] fp32, C = 2 or 3, in pixels -> boxes [N][4] int32 (x, y, w, h) and valid [N] int32.
 *                  A keypoint counts only if ALL of its C coordinates are > 0 (``pts[np.all(pts > 0., axis=1)]``, :562; a NaN
 *                  does not count); the box is taken over the first two coordinates of the counted keypoints (:564):
 *                    x = floor(min x), w = floor(max x) - x + 1, y = floor(min y), h = floor(max y) - y + 1.
 *                  cv2.boundingRect on float points is ASSUMED to be this rule -- the one image_input.bounding_box assumes;
 *                  OpenCV is no dependency of this package and the rule is not pinned against it.
 *                  No counted keypoint: valid = 0 and the box (0, 0, 0, 0); else valid = 1.  Coordinates are expected to be
 *                  finite and to fit int32.  One wave per image: a strided pass over the joints, then one min / max
 *                  reduction across the wave.  No host copy, no synchronisation.
 * vunet_box_crop   img [N][Ch][Hs][Ws] fp32, boxes [N][4], valid [N] -> out [N][Ch][S][S] fp32, S >= 2.
 *                  The INTENDED source position of output pixel (i, j) (row i, column j) is
 *                    u = x + (j w) / (S - 1),  v = y + (i h) / (S - 1):
 *                  kornia's four-point homography from the corners (x, y) (x + w, y) (x + w, y + h) (x, y + h) (:578-584) to
 *                  (0, 0) .. (S - 1, S - 1), which for an axis-aligned box is exactly this scale and shift.
 *                  `sampling` chooses the pixel that is sampled:
 *                    VUNET_CROP_REFERENCE  u' = (u Ws) / (Ws - 1) - 0.5, v' = (v Hs) / (Hs - 1) - 0.5.  kornia 0.2.0 normalises
 *                                          pixel coordinates with 2 / (W - 1), and torch 1.3.1's F.grid_sample un-normalises
 *                                          them with its default align_corners=False: ((g + 1) W - 1) / 2.  This reading of
 *                                          kornia 0.2.0 is ASSUMED, not pinned (kornia is absent).  Needs Hs, Ws >= 2.
 *                    VUNET_CROP_EXACT      (u, v) itself: the intended geometry.
 *                  Bilinear with padding_mode="zeros": x0 = floor(u'), y0 = floor(v'), fx = u' - x0, fy = v' - y0; the taps
 *                  (y0, x0) (y0, x0 + 1) (y0 + 1, x0) (y0 + 1, x0 + 1), a tap outside the image contributing 0.
 *                  Coordinates are float64 without fused multiply-adds, in the order written above; fx, fy are rounded to
 *                  fp32 and the three lerps are fp32 fused multiply-adds:
 *                    top = fma(fx, b - a, a), bottom = fma(fx, d - c, c), out = fma(fy, bottom - top, top).
 *                  valid == 0 fills the crop with zeros.  One thread per output pixel serves all channels.
 * vunet_inception_input_boxes
 *                  img [N][3][Hs][Ws], boxes, valid, the crop size S -> y [N][3][299][299]: vunet_inception_input (`mode` as
 *                  there: 0 none, 1 transform, 2 fid) of the S x S crop, without the crop being stored.  Each output pixel takes
 *                  the four taps of the virtual crop, each of those computed from its four source taps by the device function
 *                  vunet_box_crop itself runs, rounded to fp32 as the stored crop would be; the blend is float64 and rounded
 *                  once, as in vunet_inception_input.  Bit-identical to the two launches.
 * All: no allocation, no synchronisation, no atomics.  VUNET_ERR_ARG: a NULL pointer, a size < 1, C outside {2, 3}, S < 2, an
 * unknown sampling / mode, Hs or Ws < 2 with VUNET_CROP_REFERENCE, a tensor of 2^31 elements or more.
 */
#ifndef VUNET_PERSON_CROP_H
#define VUNET_PERSON_CROP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VUNET_CROP_REFERENCE 0
#define VUNET_CROP_EXACT 1

int vunet_kp_boxes(const float* kps, int32_t N, int32_t J, int32_t C, int32_t* boxes, int32_t* valid, void* stream);

int vunet_box_crop(const float* img, int32_t N, int32_t Ch, int32_t Hs, int32_t Ws, const int32_t* boxes, const int32_t* valid,
                   int32_t S, int32_t sampling, float* out, void* stream);

int vunet_inception_input_boxes(const float* img, int32_t N, int32_t Hs, int32_t Ws, const int32_t* boxes, const int32_t* valid,
                                int32_t S, int32_t sampling, int32_t mode, float* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif
