/*
 * vunet_seq_eval.h -- C ABI of the behaviour model's sampling metrics (ASD, FSD, APD, ADE, FDE), csrc/seq_eval.hip.  Part of
 * libvunet_hip.so; same conventions as vunet_hip.h (plain pointers and sizes, caller-owned device buffers, `stream` =
 * hipStream_t as void*, 0 or a negative VUNET_ERR_* code).  Additive entry points within ABI 12.
 *
 * What it replaces in the reference (CompVis/behavior-driven-video-synthesis, paths relative to the upstream root):
 *   data/data_conversions_3d.py:178-211      unNormalizeData: full[dims_to_use] = x, full = full * std + mean
 *   experiments/behavior_net.py:1238-1255    ASD / FSD per sequence (np.sort(dist)[1]), ADE / FDE per batch
 *   lib/logging.py:2079-2093                 APD per sequence
 *
 * Inputs.  x: [N][S][T][n] fp32 normalised pose vectors (n used dimensions), S samples of each of N sequences.  future:
 * [N][T + 1][n] fp32 normalised ground truth; frames 1 .. T are scored (the reference's [:, :, 1:]).  mean / stdv: n DEVICE doubles,
 * the statistics of the used dimensions (the ignored ones hold mean in every vector and add exactly 0 to any difference).
 * f32_math != 0: u = x std + mean and the differences in float32 (numpy's promotion with float32 statistics); else float64.
 * Every sum accumulates in float64.
 *
 * With u the un-normalised vectors and d_t(q, s) = ||u_q,t - u_s,t||_2 over the frame's vector, g_t = future frame t + 1:
 *   A(q, s) = mean_t d_t(q, s)      F(q, s) = d_{T-1}(q, s)      P(q, s) = sqrt(sum_t d_t(q, s)^2)
 *   G(s) = mean_t ||u_s,t - g_t||   GF(s) = ||u_s,T-1 - g_T-1||
 * scratch: N S (3 S + 2) DEVICE doubles, caller-owned, written by vunet_seq_eval_pairs and read by vunet_seq_eval_select:
 *   [A | F | P]: 3 tables of [N][S][S], row q of sequence i at (i S + q) S;  then [G | GF]: 2 x [N][S].
 *
 * vunet_seq_eval_pairs   one workgroup per (sequence, q): sample q un-normalised in LDS (T n doubles, T n <= 8192), each wave
 *                        over the samples s (and the ground truth), lanes over the frames.  Writes rows q of A, F, P and G(q),
 *                        GF(q).  VUNET_ERR_UNSUPPORTED when T n > 8192.
 * vunet_seq_eval_select  one workgroup, a wave per sequence (N <= 4096): per_seq [5][N] = APD, ASD, FSD, minADE, minFDE;
 *                        batch [2] = ADE, FDE (means over the N sequences).  ASD_i = (1/S) sum_q second(A(q, .)), second = element [1] of the row sorted ascending with
 *                        NaN last (np.sort); FSD on F; APD_i = (1/S) sum_q (sum_s P(q, s)) / (S - 1); minADE_i = min_s G(s) and
 *                        minFDE_i = min_s GF(s) propagate NaN (torch.min).  Fixed summation orders, no atomics.
 * Both: S >= 2, T >= 1, N >= 1, n >= 1, no NULL pointer, else VUNET_ERR_ARG.
 */
#ifndef VUNET_SEQ_EVAL_H
#define VUNET_SEQ_EVAL_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VUNET_SEQ_EVAL_MAX_TN 8192

int vunet_seq_eval_pairs(const float* x, const float* future, const double* mean, const double* stdv, int32_t f32_math, int32_t N,
                         int32_t S, int32_t T, int32_t n, double* scratch, void* stream);

int vunet_seq_eval_select(const double* scratch, int32_t N, int32_t S, double* per_seq, double* batch, void* stream);

#ifdef __cplusplus
}
#endif
#endif
