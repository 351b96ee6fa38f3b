/*
 * vunet_image_input.h -- C ABI of the raw-frame input route, csrc/image_input.hip: decoded uint8 RGB frames -> the fp32 images
 * the trainers take, on the GPU.  Part of libvunet_hip.so; same conventions as vunet_hip.h (plain pointers and sizes,
 * caller-owned device buffers, `stream` = hipStream_t as void*, 0 or a negative VUNET_ERR_* code).  Additive entry points
 * within ABI 12.
 *
 * What it replaces in the reference (CompVis/behavior-driven-video-synthesis, paths relative to the upstream root):
 *   data/base_dataset.py:281-315, :461-489   the crop around the keypoints with cv2.copyMakeBorder(BORDER_REFLECT)
 *   data/__init__.py:15-43                    ToPILImage -> Resize([S, S], BICUBIC) -> ToTensor -> x * 2 - 1
 *
 * Input.  frames: uint8 [N][Hmax][Wmax][3], RGB interleaved, a padded stack.  geom: int32 [N][6] on the DEVICE, one row per
 * image: (h, w, x0, y0, cw, ch) -- h x w the valid frame inside the stack, (x0, y0, cw, ch) the crop window in frame
 * coordinates, which may lie partly or wholly outside the frame.  Contract: 1 <= h, ch <= Hmax and 1 <= w, cw <= Wmax.  An image
 * whose row breaks it is never indexed with: status[n] = 1, its output is all -1.0 (fp32) or 0 (uint8).
 *
 * Source fetch.  Window pixel (i, j) is frame pixel (reflect(y0 + i, h), reflect(x0 + j, w)); reflect is cv2.BORDER_REFLECT
 * (fedcba|abcdefgh|hgfedcb): while p is outside [0, len): p = -p - 1 if p < 0, else 2 len - p - 1 -- evaluated as a triangle
 * wave of period 2 len with one modulo in 64-bit integers, which is the same function for every int32 x0, y0.
 *
 * Resample.  The cw x ch window is resampled to S x S exactly as Pillow's 8-bit ImagingResample does with the bicubic filter
 * (a = -0.5), horizontal pass first.  Per axis, in = window size, out = S, all in float64 without fused multiply-adds:
 *   scale = (double)(float)in / out; filterscale = max(scale, 1); support = 2 filterscale; ksize = (int)ceil(support) * 2 + 1;
 *   per output index xx: center = (xx + 0.5) scale; xmin = max((int)(center - support + 0.5), 0);
 *   xmax = min((int)(center + support + 0.5), in) - xmin; w[x] = bicubic((x + xmin - center + 0.5) * (1 / filterscale));
 *   ww = sum of w in index order; if ww != 0: w[x] = w[x] / ww; k[x] = (int)(w[x] 2^22 +- 0.5), sign of w[x], truncated.
 * A pass value is clamp((2^21 + sum pixel * k[x]) >> 22, 0, 255) in int32, stored as uint8 between the passes.  An axis with
 * in == out -- Pillow skips it -- gets the identity table (xmin = xx, xmax = 1, k[0] = 2^22), which yields the same bytes.
 *
 * vunet_image_input_tables    geom -> coef [2][N][S][kmax] int32 (axis 0: horizontal, in = cw; axis 1: vertical, in = ch; zeros
 *                             past xmax), bounds [2][N][S][2] int32 (xmin, xmax) and status [N] int32.  A contract-breaking row:
 *                             zeros throughout, status 1.  kmax must be the ksize of in = max(Hmax, Wmax); it bounds every ksize
 *                             the contract admits.  One thread per (axis, image, output index).  One launch.
 * vunet_image_input_resample  frames, geom and the tables -> exactly one of out_f32 [N][3][S][S] = (float)v / 255.0f * 2.0f - 1.0f
 *                             (torch's ToTensor and the reference's lambda, each operation rounded once) and out_u8
 *                             [N][S][S][3]; the other pointer NULL.  inter: uint8 scratch [N][Hmax][S][3] (rows >= ch are not
 *                             touched).  Two launches: the horizontal pass (one block per window row, lanes along output x, the
 *                             source row through L1) and the vertical pass (one block per output row: coalesced reads of the
 *                             intermediate, coefficients uniform over the block).
 * Both: no allocation, no synchronisation, no atomics (recordable in a hipGraph); no NULL pointer otherwise, 1 <= N, Hmax, Wmax,
 * S <= 65535, else VUNET_ERR_ARG.
 */
#ifndef VUNET_IMAGE_INPUT_H
#define VUNET_IMAGE_INPUT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VUNET_IMAGE_INPUT_PRECISION_BITS 22

int vunet_image_input_tables(const int32_t* geom, int32_t N, int32_t Hmax, int32_t Wmax, int32_t S, int32_t kmax, int32_t* coef,
                             int32_t* bounds, int32_t* status, void* stream);

int vunet_image_input_resample(const uint8_t* frames, const int32_t* geom, int32_t N, int32_t Hmax, int32_t Wmax, int32_t S,
                               int32_t kmax, const int32_t* coef, const int32_t* bounds, const int32_t* status, uint8_t* inter,
                               float* out_f32, uint8_t* out_u8, void* stream);

#ifdef __cplusplus
}
#endif
#endif
