/*
 * vunet_seq_latent.h -- C ABI of the latent diagnostics of the behaviour model's evaluation loop (held-out flow likelihood,
 * Kolmogorov-Smirnov test of the Gaussianised codes), csrc/seq_latent.hip.  Part of libvunet_hip.so; same conventions as
 * vunet_hip.h (plain pointers and sizes, caller-owned device buffers, `stream` = hipStream_t as void*, 0 or a negative
 * VUNET_ERR_* code).  Additive entry points within ABI 12.
 *
 * What it replaces in the reference (CompVis/behavior-driven-video-synthesis, paths relative to the upstream root):
 *   lib/losses.py:295-311, :330-331      FlowLoss: nll = 0.5 sum z^2 per row, its mean, -mean(logdet), their sum, and the same
 *                                        mean over a fresh standard-normal draw
 *   lib/logging.py:2549-2556             scipy.stats.kstest(column, "norm") for every dimension of the Gaussianised codes
 *
 * vunet_seq_latent_nll   z: [B][C] fp32 with leading dimension ldz >= C; logdet: [B] fp32; noise: [B][C] fp32 (contiguous) or
 *                        NULL.  per_row: [2][B] doubles, nll_i = 0.5 sum_c z_ic^2 and logp_i = -nll_i + logdet_i - 0.5 C
 *                        log(2 pi).  scalars: [4] doubles, flow_loss, reference_nll_loss, nlogdet_loss, nll_loss (the order of
 *                        vunet_seq_flow_loss): nll_loss = mean_i nll_i, nlogdet_loss = -mean_i logdet_i, flow_loss = their sum,
 *                        reference_nll_loss = mean_i 0.5 sum_c noise_ic^2 or NaN without noise.  Everything accumulates in
 *                        float64.  Two launches: a wave per row (lanes over the columns, a fixed butterfly), then one
 *                        workgroup that sums the rows in a fixed order; between them per_row[1] carries the noise rows'
 *                        values.  Any B >= 1, C >= 1.
 *
 * vunet_seq_ks_norm      the one-sample two-sided Kolmogorov-Smirnov statistic of each of C columns of N fp32 values against
 *                        N(0, 1).  col_major != 0: x is [C][ld] (column c at x + c ld, ld >= N); else [N][ld] (ld >= C).
 *                        Per column: sort ascending, F_i = 0.5 erfc(-x_(i) / sqrt 2) in float64, D+ = max_i (i / N - F_i),
 *                        D- = max_i (F_i - (i - 1) / N), D = max(D+, D-), i = 1 .. N.  stat: [3][C] doubles D, D+, D-.
 *                        p_asym: [C] doubles, the Kolmogorov series 2 sum_{k >= 1} (-1)^(k-1) exp(-2 k^2 t^2), t = D sqrt N,
 *                        summed until a term is below 1e-17 and clamped to [0, 1]; for t < 0.2 the theta-function form
 *                        1 - sqrt(2 pi) / t sum_{k >= 1} exp(-(2k - 1)^2 pi^2 / (8 t^2)).  A column with a NaN gives NaN in all
 *                        four outputs; +-inf are ordinary values.
 *                        sorted == 0: N <= VUNET_SEQ_KS_MAX_LDS_N, one workgroup sorts its columns wholly in LDS (a bitonic
 *                        network over the next power of two of N; several columns share a workgroup when they are short).
 *                        sorted != 0: the columns are ascending already, any N, only the statistic is evaluated.
 *                        scratch: unused, may be NULL.  Max reductions only: results are bit-identical from run to run.
 * NULL x / stat / p_asym (or z / logdet / per_row / scalars), N, C, B < 1, a leading dimension below its extent:
 * VUNET_ERR_ARG; sorted == 0 with N above the cap: VUNET_ERR_UNSUPPORTED.  Nothing is launched then.
 */
#ifndef VUNET_SEQ_LATENT_H
#define VUNET_SEQ_LATENT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VUNET_SEQ_KS_MAX_LDS_N 32768

int vunet_seq_latent_nll(const float* z, int64_t ldz, const float* logdet, const float* noise, int32_t B, int32_t C, double* per_row,
                         double* scalars, void* stream);

int vunet_seq_ks_norm(const float* x, int64_t ld, int32_t col_major, int32_t N, int32_t C, int32_t sorted, double* stat,
                      double* p_asym, void* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif
