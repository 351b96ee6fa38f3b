/*
 * vunet_inception.h -- C ABI of the inference-only Inception-v3 path, csrc/inception.hip: a general forward convolution, 3x3
 * pooling, the global average and the resize-to-299 input kernel.  Part of libvunet_hip.so; same conventions as vunet_hip.h
 * (plain pointers and sizes, caller-owned device buffers, `stream` = hipStream_t as void*, 0 or a negative VUNET_ERR_* code).
 * Additive entry points within ABI 12.
 *
 * What it serves in the reference (CompVis/behavior-driven-video-synthesis): models/imagenet_pretrained.py:64-111
 * (FIDInceptionModel) and lib/metrics.py:362-415 (inception_score), both around torchvision's inception_v3.
 *
 * All tensors are fp32 NCHW.  Every entry point: no allocation, no synchronisation, no atomics, a fixed summation order
 * (recordable in a hipGraph, bit-identical from run to run).
 *
 * vunet_convg           y[n, y_coff + m, ho, wo] = act(bias[m] + sum_{c, kh, kw} w[m, c, kh, kw] *
 *                         x[n, x_coff + c, ho stride_h - pad_h + kh, wo stride_w - pad_w + kw]), zeros outside the map; act = ReLU
 *                       where `relu`, else the identity.  x is a channel slice [x_coff, x_coff + C) of a tensor with x_ctot
 *                       channels, y a slice [y_coff, y_coff + M) of one with y_ctot: the last convolution of an Inception
 *                       branch stores straight into the block's concatenated output.  Channels of y outside the slice are not
 *                       touched.  Ho = (H + 2 pad_h - KH) / stride_h + 1, Wo alike (checked).  H = W = 1 is a matrix product.
 *                       w is PACKED: fp32 [Kpad][Mpad], row k = (c KH + kh) KW + kw, zeros for k >= C KH KW and m >= M;
 *                       Kpad a multiple of VUNET_CONVG_KC, Mpad of VUNET_CONVG_MT.  bias: [M] or NULL.
 *                       An implicit GEMM on v_mfma_f32_16x16x4_f32: exact fp32 operands, fp32 accumulation, k ascending.
 *                       `tile`: the workgroup's tile of (output channels x output pixels), 64 (64 x 64) or 32 (32 x 32);
 *                       0 = 64 where M > 32 and that makes >= VUNET_CONVG_FILL workgroups (two per CU), else 32.  Each is bit-identical from
 *                       run to run; the two differ in the last bits (the 32 x 32 form sums even and odd groups of four k
 *                       separately and adds the two sums at the end).
 * vunet_pool2d          3x3 pooling, stride 1 or 2, pad 0 or 1, with the same channel-slice fields.  mode 0: max over the taps
 *                       inside the map; mode 1: average, the sum of the taps inside the map (row by row, left to right) / 9.
 * vunet_global_avgpool  y[i] = mean of x[i][0 .. HW), i < NC.  One wave per row, a fixed tree.
 * vunet_inception_input x [N][3][H][W] -> y [N][3][299][299], bilinear as nn.Upsample / F.interpolate(align_corners=False):
 *                       per axis src = max((dst + 0.5) in / 299 - 0.5, 0), i0 = floor(src), i1 = min(i0 + 1, in - 1),
 *                       l = src - i0; v = (1 - ly)((1 - lx) x00 + lx x01) + ly((1 - lx) x10 + lx x11).  Then per `mode`:
 *                         0  v
 *                         1  v (std_c / 0.5) + (mean_c - 0.5) / 0.5                (torchvision's transform_input)
 *                         2  (clamp((v + 1) / 2, 0, 1) - mean_c) / std_c            (FIDInceptionModel)
 *                       mean = (0.485, 0.456, 0.406), std = (0.229, 0.224, 0.225).  Evaluated in float64 and rounded once.
 * vunet_inception_score logits [N][K] fp32 -> scores [splits] float64 (csrc/inception_score.hip): lib/metrics.py:403-415 with
 *                       scipy.stats.entropy(pk, qk), in float64.  Per row p = softmax by log-sum-exp (max, sum exp(l - max)).
 *                       Split k takes the rows k (N / splits) .. (k + 1) (N / splits) - 1 (integer division; the tail rows belong
 *                       to no split, as in the reference); q = the column mean of its rows; both vectors are renormalised to
 *                       sum 1; KL_i = sum p log(p / q), a term with p == 0 contributing 0; scores[k] = exp(mean_i KL_i).  A split
 *                       without rows (splits > N) scores NaN, the reference's mean of nothing.  `work`: caller-owned scratch of
 *                       4 N + splits K doubles.  Four launches; every sum in a fixed order (strided partial sums, one tree: two
 *                       stages).  splits <= 65535.
 *
 * VUNET_ERR_ARG: a NULL pointer (bias excepted), a size < 1, an inconsistent Ho / Wo, a slice outside its tensor, a packing
 * that is not padded as stated, a tensor of 2^31 elements or more, an unknown mode / tile.
 */
#ifndef VUNET_INCEPTION_H
#define VUNET_INCEPTION_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VUNET_CONVG_KC 64     /* Kpad % KC == 0 (the K rows the 32 x 32 form stages per step; the 64 x 64 form takes 32) */
#define VUNET_CONVG_MT 64     /* Mpad % MT == 0 */
#define VUNET_CONVG_FILL 512  /* tile = 0: 64 x 64 tiles where there are at least this many (measured: profiles/inception_time.txt) */
#define VUNET_INCEPTION_SIZE 299

typedef struct vunet_convg_desc {
  int32_t N, C, H, W, M, Ho, Wo;
  int32_t KH, KW, stride_h, stride_w, pad_h, pad_w;
  int32_t x_ctot, x_coff, y_ctot, y_coff;
  int32_t relu;
  int32_t Kpad, Mpad, tile;
} vunet_convg_desc;

typedef struct vunet_pool2d_desc {
  int32_t N, C, H, W, Ho, Wo;
  int32_t stride, pad, mode;
  int32_t x_ctot, x_coff, y_ctot, y_coff;
} vunet_pool2d_desc;

int vunet_convg(const vunet_convg_desc* d, const float* x, const float* w, const float* bias, float* y, void* stream);

/* the tile (64 or 32) vunet_convg runs `d` with, or VUNET_ERR_ARG */
int vunet_convg_tile(const vunet_convg_desc* d);

int vunet_pool2d(const vunet_pool2d_desc* d, const float* x, float* y, void* stream);

int vunet_global_avgpool(const float* x, float* y, int64_t NC, int32_t HW, void* stream);

int vunet_inception_input(const float* x, float* y, int32_t N, int32_t H, int32_t W, int32_t mode, void* stream);

int vunet_inception_score(const float* logits, int32_t N, int32_t K, int32_t splits, double* work, double* scores, void* stream);

#ifdef __cplusplus
}
#endif
#endif
