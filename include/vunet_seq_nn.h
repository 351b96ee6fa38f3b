/*
 * vunet_seq_nn.h -- C ABI of the nearest-training-neighbour scans of the behaviour model, csrc/seq_nn.hip.  Part of
 * libvunet_hip.so; same conventions as vunet_hip.h (plain pointers and sizes, caller-owned device buffers, `stream` =
 * hipStream_t as void*, 0 or a negative VUNET_ERR_* code).  Additive entry points within ABI 12.
 *
 * What it replaces in the reference (CompVis/behavior-driven-video-synthesis, paths relative to the upstream root), per query a
 * host scan of the whole training set in numpy:
 *   lib/figures.py:258-262   np.argmin(np.linalg.norm(betas_train - mu, axis=1))                          [N, H] float32 codes
 *   lib/figures.py:268-277   np.argmin(np.sum(np.linalg.norm(xs_aligned - seqs_aligned, axis=-1), axis=(1, 2)))
 *                                                                                                 [N, T, J, 3] float64 poses
 *   lib/figures.py:146-164   seqs_aligned = seqs_train + mean_pelvis - seqs_train[:, :, pelvis]
 *
 * Code space, vunet_nn_codes.  bank: N rows of H fp32 values, row j at bank + j ld (ld >= H floats); q: [Q][H] fp32, dense.
 *   d(q, j) = sqrt(sum_i (fl32(bank[j][i] - q[i]))^2)
 * The difference is one fp32 subtraction (the rounding numpy's float32 subtraction makes); its square is exact in float64, and the
 * sum and the square root are float64.  H <= VUNET_NN_MAX_H (the query tile in LDS), else VUNET_ERR_UNSUPPORTED.
 *
 * Pose space, vunet_nn_poses.  bank: [N][T][n], q: [Q][T][n] normalised fp32 pose vectors, n = 3 J, root in [0, J).  mean / stdv:
 * n DEVICE doubles and f32_math exactly as vunet_seq_eval_pairs takes them (vunet_seq_eval.h).  With u = x std + mean (float64;
 * f32_math != 0: that one expression in float32, two roundings, then widened) and the 3-vectors c_t,k = u_t,k - u_t,root:
 *   D(q, j) = sum_t sum_k || c^q_t,k - c^j_t,k ||_2
 * Everything after the un-normalisation is float64: the centring, the difference, (dx^2 + dy^2) + dz^2 without fusing, the square
 * root and the sum.  The reference adds the training set's mean pelvis to both sides before it subtracts them; that term cancels
 * in the difference and is omitted here.  T n <= VUNET_NN_MAX_TN (the query tile in LDS: VUNET_NN_QT_POSES T n doubles), else
 * VUNET_ERR_UNSUPPORTED.
 *
 * Selection (both): numpy's argmin.  The smallest distance wins, among equal distances the lowest index, a NaN distance ranks
 * below every number and the first NaN wins; best_d is then NaN.  best_d [Q] doubles, best_i [Q] int32.
 *
 * Two phases, no atomics.  Phase 1: workgroup (c, g) streams rows [c CHUNK, (c + 1) CHUNK) of the bank, VUNET_NN_CHUNK rows,
 * against query tile g -- QT queries held in LDS (pose space: already un-normalised and root-centred), QT = VUNET_NN_QT_CODES
 * = 16 in code space and VUNET_NN_QT_POSES = 4 in pose space -- and writes one (d, i) candidate per (chunk, query) to `scratch`.
 * Phase 2: one wave per query folds its candidates; the selection rule is a total order, so the fold equals the fold in chunk
 * order.  The bank is read from memory ceil(Q / QT) times.  A wave owns a row: lane l sums elements 4 (l + 64 k) .. + 3,
 * k = 0, 1, ... (pose space: joints l + 64 k of the T J), then a fixed butterfly adds the 64 lanes.  That order depends on H (or T,
 * J) alone -- not on the row's index, N, Q, the pitch or the grid: two equal rows get equal bits, any call the same bits again.
 * Code space reads a row with 16-byte loads when H % 4 == 0, ld % 4 == 0 and bank is 16-byte aligned, else with 4-byte loads in
 * the same element order.  Pose space reads 4-byte values: a joint is 12 bytes and T n is odd at the reference's size (51 x 51), so
 * rows do not start on 16 bytes.
 *
 * scratch: vunet_nn_scratch_bytes(N, Q) bytes, 8-byte aligned, caller-owned, overwritten by every call:
 *   [Q][chunks] doubles, then [Q][chunks] int32, chunks = ceil(N / VUNET_NN_CHUNK).
 * Arguments: N, Q, H, T, J >= 1, 0 <= root < J, ld >= H, no NULL pointer, else VUNET_ERR_ARG.  N < 2^31; element offsets are 64-bit.
 * Q <= 65535 QT (the grid's second dimension), else VUNET_ERR_UNSUPPORTED.
 */
#ifndef VUNET_SEQ_NN_H
#define VUNET_SEQ_NN_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VUNET_NN_QT_CODES 16
#define VUNET_NN_QT_POSES 4
#define VUNET_NN_CHUNK 128
#define VUNET_NN_MAX_H 1024
#define VUNET_NN_MAX_TN 4096

/* host helper: *bytes = the scratch either scan needs for N bank rows and Q queries */
int vunet_nn_scratch_bytes(int32_t N, int32_t Q, int64_t* bytes);

int vunet_nn_codes(const float* bank, int64_t ld, int32_t N, const float* q, int32_t Q, int32_t H, void* scratch, double* best_d,
                   int32_t* best_i, void* stream);

int vunet_nn_poses(const float* bank, int32_t N, const float* q, int32_t Q, int32_t T, int32_t J, int32_t root, const double* mean,
                   const double* stdv, int32_t f32_math, void* scratch, double* best_d, int32_t* best_i, void* stream);

#ifdef __cplusplus
}
#endif
#endif
