/*
 * vunet_appearance_aug.h -- C ABI of the random appearance augmentation, csrc/appearance_aug.hip: uint8 RGB frames and one affine
 * per image -> Pillow's Image.transform(AFFINE, BILINEAR, fillcolor) of each frame (optionally of its reflect-padded copy, and only
 * a window of the result), on the GPU.  Part of libvunet_hip.so; same conventions as vunet_hip.h (plain pointers and sizes,
 * caller-owned device buffers, `stream` = hipStream_t as void*, 0 or a negative VUNET_ERR_* code).  An additive entry point
 * within ABI 12.
 *
 * What it replaces in the reference (CompVis/behavior-driven-video-synthesis, paths relative to the upstream root), the
 * `inplane_normalize: False` appearance input of its DeepFashion and Market runs:
 *   data/deepfashion.py:92-108, :170-181   RandomAffine(degrees 30, translate (0.3, 0), scale (0.7, 1), BILINEAR, fill white)
 *   data/market.py:52-64, :118-126         Pad(S / 2, reflect) -> RandomRotation(90, BILINEAR) -> CenterCrop(128)
 * (the Resize(S, BICUBIC) -> ToTensor -> x * 2 - 1 that follows both is vunet_image_input.h).  The random draws stay on the host;
 * the kernel takes their matrices.
 *
 * Input.  frames: uint8 [N][Hmax][Wmax][3], RGB interleaved, a padded stack.  hw: int32 [N][2] on the DEVICE, (h, w) of the valid
 * frame inside each slot; contract 1 <= h <= Hmax, 1 <= w <= Wmax.  mats: float64 [N][6] on the DEVICE, one OUTPUT-to-INPUT affine
 * (M0 .. M5) per image, as Pillow takes it.  Uniform arguments: the reflect pad p >= 0, the output window's origin (ox, oy) and size
 * (oh, ow) in the coordinates of the transformed (padded) image, the fill colour.
 *
 * The padded image P has H = h + 2 p rows and W = w + 2 p columns, P[r][c] = frame[refl(r - p, h)][refl(c - p, w)]; refl is NumPy's
 * mode="reflect" (dcb|abcd|cba: the edge is NOT repeated, period 2 (n - 1), applied as often as needed; n = 1 maps everything to
 * 0).  It is never materialised.  Note: this is not the cv2.BORDER_REFLECT of vunet_image_input.h, which repeats the edge.
 *
 * Output pixel (x, y) of the window, all in float64 with every multiply and add rounded on its own (no fused multiply-add):
 *   xin = (x + ox) + 0.5; yin = (y + oy) + 0.5; xs = (M0 xin + M1 yin) + M2; ys = (M3 xin + M4 yin) + M5;
 *   the fill colour unless 0 <= xs < W and 0 <= ys < H; else
 *   xs -= 0.5; ys -= 0.5; x0 = floor(xs); y0 = floor(ys); dx = xs - x0; dy = ys - y0;
 *   taps P[clamp(y0)][clamp(x0)], P[clamp(y0)][clamp(x0 + 1)] (upper row: a, b) and the same of row clamp(y0 + 1), clamped to
 *   [0, H - 1] and [0, W - 1]; per channel v1 = a + (b - a) dx, v2 alike on the lower row, v = v1 + (v2 - v1) dy; the byte is v
 *   truncated toward zero.
 * This is Pillow's ImagingGenericTransform with affine_transform and bilinear_filter32RGB, restated (pinned against Pillow 12.2.0
 * by tests/golden/g22_appearance_aug.npz).
 *
 * An image whose matrix row has a non-finite coefficient, or whose hw row breaks the contract, is never indexed with: its output
 * is all fill and status[n] = 1; status[n] = 0 otherwise.
 *
 * vunet_appearance_affine  exactly one of out_f32 [N][3][oh][ow] = (float)v / 255.0f * 2.0f - 1.0f (torch's ToTensor and the
 *                          reference's lambda, each operation rounded once) and out_u8 [N][oh][ow][3]; the other pointer NULL.
 *                          One launch, one thread per output pixel, lanes along x.  No allocation, no synchronisation, no atomics
 *                          (recordable in a hipGraph).  1 <= N, Hmax, Wmax, oh, ow <= 65535, 0 <= p <= 2^20, |ox|, |oy| <= 2^24,
 *                          0 <= fill_* <= 255, no NULL pointer otherwise, else VUNET_ERR_ARG.
 */
#ifndef VUNET_APPEARANCE_AUG_H
#define VUNET_APPEARANCE_AUG_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int vunet_appearance_affine(const uint8_t* frames, const int32_t* hw, const double* mats, int32_t N, int32_t Hmax, int32_t Wmax,
                            int32_t pad, int32_t ox, int32_t oy, int32_t oh, int32_t ow, int32_t fill_r, int32_t fill_g,
                            int32_t fill_b, float* out_f32, uint8_t* out_u8, int32_t* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
