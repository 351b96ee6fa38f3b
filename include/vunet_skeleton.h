/*
 * vunet_skeleton.h -- C ABI of the skeleton-frame rasteriser, csrc/skeleton.hip: the frames of the pose-only videos and the
 * first panel of every evaluation figure, drawn on the GPU.  Part of libvunet_hip.so; same conventions as vunet_hip.h (plain
 * pointers and sizes, caller-owned device buffers, `stream` = hipStream_t as void*, 0 or a negative VUNET_ERR_* code).  An
 * additive entry point within ABI 12.
 *
 * What it replaces in the reference (CompVis/behavior-driven-video-synthesis, paths relative to the upstream root):
 *   lib/utils.py:733-750                   add_joints_to_img: one cv2.line per limb
 *   data/data_conversions_3d.py:1134-1142  the canvas of the camera's image size, filled with the background colour
 *   :1188-1190                             cv2.resize(img, target_size, interpolation=cv2.INTER_NEAREST)
 *   :1176-1184, :1194-1205                 the person-centred strip of the synthesised frame / of the skeleton frame, `masks`
 *   :1210-1214                             the overlay of the skeleton on the synthesised frame
 * Left out: cv2.putText (:1149).  The Hershey font tables are OpenCV's; without the black label the top-left corner of a
 * frame shows background (of an overlay: the synthesised frame) where the reference shows text.
 *
 * vunet_skeleton_raster, for F frames:
 *   kps          fp32 [F][J][2], (x, y) in canvas pixels; limbs int32 [L][2] joint pairs; colors uint8 [L][3]; L <= 64.
 *   Hs, Ws       the canvas size, one per launch.  thickness 0..79 (0 and 1: the thin line); background 0..255, all channels.
 *   sy, sx       int32 [Ht] / [Wt]: the canvas row / column of every output row / column.  NULL: the identity (Ht == Hs resp.
 *                Wt == Ws required).  The values are only compared with, never indexed with.
 *   tw           0: no crop, the output is Wt wide.  > 0: the output is the tw-wide strip (tw <= Wt) that starts at
 *                  int(min(max(0, mean_j(x_j / skel_div) - tw / 2), Wt - tw))           (tw / 2: integer division)
 *                and the rgb strip starts at the same expression with x_j * rgb_mul and the bound Sw - tw.  float64; the
 *                joints are crop_joints[0 .. n_crop) (NULL: all J), added in that order, then divided by their number.
 *   rgb          NULL, or uint8 [F][Ht][Sw][3]; Sw == Wt without a crop, Sw >= tw with one.  Sw may be given without rgb to
 *                have the rgb span computed.
 *   out_skel     NULL, or the skeleton frames, uint8 channels-last: pixel (f, y, x) at out_skel + f skel_fs + y skel_rs + 3 x
 *                (byte strides; skel_rs >= 3 * output width), so a caller can draw into one tile of a larger image.
 *   out_overlay  NULL, or uint8 [F][Ht][Wo][3]: the rgb strip where all three skeleton channels are 255, the skeleton elsewhere.
 *   out_rgb      NULL, or uint8 [F][Ht][Wo][3]: the rgb strip.  Both need rgb.  Wo = tw > 0 ? tw : Wt.
 *   span         NULL, or int32 [F][2][2] (needs tw > 0): (min_x, max_x) of the skeleton strip, then of the rgb strip
 *                ((0, 0) when Sw < tw).
 * Drawing: for each limb in list order cv2.line(img, (int(x_a), int(y_a)), (int(x_b), int(y_b)), color, thickness) as OpenCV
 * 4.1.2 draws it (LINE_8, shift 0), int() truncating toward zero.  No validity rule: a limb with a negative or out-of-canvas
 * end point is drawn and clipped.  The last limb that covers a pixel gives it all three channels.  A limb that names a joint
 * outside [0, J) is not drawn; neither is one with an end point beyond +-VUNET_SKELETON_COORD_LIMIT pixels (OpenCV would
 * walk every row between it and the canvas).  Keypoints must be finite.
 * One launch; no allocation, no synchronisation, no atomics (recordable in a hipGraph).  F == 0 returns 0 without a launch.
 * Overlapping outputs are the caller's business.
 */
#ifndef VUNET_SKELETON_H
#define VUNET_SKELETON_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VUNET_SKELETON_MAX_LIMBS 64
#define VUNET_SKELETON_COORD_LIMIT (1 << 20)

int vunet_skeleton_raster(const float* kps, int32_t F, int32_t J, const int32_t* limbs, const uint8_t* colors, int32_t L,
                          int32_t Hs, int32_t Ws, int32_t thickness, int32_t background, const int32_t* sy, const int32_t* sx,
                          int32_t Ht, int32_t Wt, int32_t tw, const int32_t* crop_joints, int32_t n_crop, double skel_div,
                          double rgb_mul, const uint8_t* rgb, int32_t Sw, uint8_t* out_skel, int64_t skel_fs, int64_t skel_rs,
                          uint8_t* out_overlay, uint8_t* out_rgb, int32_t* span, void* stream);

#ifdef __cplusplus
}
#endif
#endif
