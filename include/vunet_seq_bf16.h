/*
 * vunet_seq_bf16.h -- C ABI of the half-size weight form of the flow's MLP layers (csrc/seq_bf16.hip; part of libvunet_hip.so,
 * conventions of vunet_hip.h).  INFERENCE ONLY: the layers of vunet_seq_linear_tiled (include/vunet_seq_tiled.h) with the weight
 * matrices stored as bf16 and multiplied on v_mfma_f32_16x16x32_bf16.  The activations keep all 24 significand bits (below), so a
 * layer computes the fp32-accurate product of x with the bf16-ROUNDED weights; biases, epilogues, ActNorm and vunet_seq_coupling
 * stay fp32 and are the same code paths' arithmetic.
 *
 * Weight image: tile-major, one [16 rows][32 k] chunk contiguous (1 KB), in the A-operand order of the instruction -- lane l of
 * a wave holds row l & 15 and k = 8 (l >> 4) + j, j = 0..7, as 16 contiguous bytes:
 *
 *   wt16[M / 16][K / 32][64][8]      wt16[mt][c][l][j] = bf16(w[16 mt + (l & 15)][32 c + 8 (l >> 4) + j])
 *
 * i.e. element (m, k) of w sits at bf16 index  ((m / 16) (K / 32) + k / 32) 512 + (((k % 32) / 8) 16 + m % 16) 8 + k % 8.
 * bf16() is round-to-nearest-even on the fp32 bit pattern (ties to the even bf16; +-inf stay; every NaN becomes the quiet NaN
 * 0x7FC0; fp32 subnormals round to bf16 subnormals or zero like any other value) -- what torch's float -> bfloat16 cast gives.
 *
 * Operand: fp32 in memory, row-major state rows or the xt tiles of vunet_seq_tiled.h (a lane's eight k of a chunk are the same
 * eight as in the fp32 kernel); outputs are fp32 rows, xt tiles or the split head's raw slabs exactly as there.  In registers
 * each operand value x is split into three bf16 terms by TRUNCATION of the running remainder:
 *
 *   t0 = hi16(x)   r1 = x - t0   t1 = hi16(r1)   r2 = r1 - t1   t2 = hi16(r2)       (hi16: the upper 16 bits of the fp32 pattern)
 *
 * Both subtractions are exact in fp32 and the terms take 8 + 8 + 8 significand bits, so x == t0 + t1 + t2 exactly for every
 * finite x with |x| >= 2^-110, all three terms normal bf16 numbers (below that t1 / t2 fall into bf16's subnormal range and can
 * need bits under its smallest step: an absolute error under 2^-133 per value).  +-inf and NaN operands give NaN terms (inf - inf), where the fp32 kernel would give +-inf for
 * an inf: non-finite either way.  A bf16 x bf16 product is exact in fp32.
 *
 * Order of the sums, fixed by the geometry alone: one fp32 accumulator per (weight tile, batch tile) and wave; per K chunk of 32,
 * chunks ascending, three MFMA into it, smallest term first:  acc += W t2;  acc += W t1;  acc += W t0.  The waves' partial sums
 * are then added in wave order through LDS, as in the fp32 kernel.  Eager and graph-replayed launches are bit-equal.
 *
 *   vunet_seq_pack_tiles_bf16   w [M][ld] row-major fp32 (M % 16 == 0, K % 32 == 0, ld >= K, ld % 4 == 0) -> wt16 (M K bf16)
 *   vunet_seq_linear_bf16w      vunet_seq_linear_tiled on bf16 images: w0 / w1 are wt16 images; `layout` must have bit 1
 *                               (VUNET_SEQ_TILED_W) set, bits 2 / 4 (operand / output tiles) mean what they mean there; layout 1
 *                               (rows in, rows out) serves a single layer.  Descriptor, one or two nets, split head (S > 1: raw
 *                               partial slabs for vunet_seq_coupling), bias and LeakyReLU / Tanh epilogue, B <= 64: as there.
 */
#ifndef VUNET_SEQ_BF16_H
#define VUNET_SEQ_BF16_H
#include "vunet_seq_tiled.h"

#ifdef __cplusplus
extern "C" {
#endif

int vunet_seq_pack_tiles_bf16(const float* w, int32_t ld, int32_t M, int32_t K, uint16_t* wt16, void* stream);
int vunet_seq_linear_bf16w(const vunet_seq_linear_desc* d, int32_t layout, const uint16_t* w0, const uint16_t* w1, const float* x,
                           const float* bias0, const float* bias1, float* y, void* stream);

#ifdef __cplusplus
}
#endif
#endif
