/*
 * vunet_fid.h -- C ABI of the FID statistic on the device, csrc/fid.hip.  Part of libvunet_hip.so; same conventions as
 * vunet_hip.h (plain pointers and sizes, caller-owned device buffers, `stream` = hipStream_t as void*, 0 or a negative
 * VUNET_ERR_* code).  Additive entry points within ABI 12.
 *
 * What it replaces in the reference (CompVis/behavior-driven-video-synthesis, paths relative to the upstream root):
 *   lib/metrics.py:211-212, :272-275   np.mean / np.cov of the [N, 2048] pool features, on the host
 *   lib/metrics.py:285-322             _calculate_fid: scipy.linalg.sqrtm of the 2048 x 2048 covariance product
 * The statistic is restated with matrix products only ("FID by a polar iteration"); the products are float64 on
 * the matrix cores (v_mfma_f64_16x16x4_f64).
 *
 * vunet_f64_gemm   C = alpha * op(A) * op(B) + diag * I on row-major float64; op(A) is [M][K], op(B) is [K][N], C is [M][N]
 *                  (I: ones where row == column).  trans_a == 0: A is stored [M][K] with leading dimension lda >= K;
 *                  trans_a == 1: A is stored [K][M], lda >= M.  trans_b == 0: B stored [K][N], ldb >= N; trans_b == 1: B stored
 *                  [N][K], ldb >= K.  ldc >= N.  Any M, N, K >= 1: tiles are zero-padded inside the kernel, nothing outside
 *                  the three matrices is read and nothing outside C's M x N elements is written.  C must not overlap A or B.
 *                  One workgroup per 64 x 64 tile of C walks K in steps of 16, in order, through LDS; there is no split-K and
 *                  no atomic: every element is summed in one fixed order, so two runs agree bit for bit and op(A) = X^T,
 *                  op(B) = X gives a bit-symmetric C (C[i][j] and C[j][i] are the same products in the same order).
 *                  The epilogue is v = alpha * acc, then v + diag on the diagonal, without fused multiply-adds.
 * vunet_fid_center / vunet_fid_center_f64
 *                  features [N][D] (fp32 / float64), N >= 2 -> mu [D] float64, the column means (16 strided partial sums per
 *                  column, then one LDS tree: a fixed order), and Y [N][D] float64 = (x - mu) / sqrt(N - 1), so that Y^T Y is
 *                  np.cov(x, rowvar=False).  Two launches.
 * vunet_f64_dot    out[0] = sum_i a[i] * b[i] over n float64 values in a fixed order: per-thread strided partial sums over at most
 *                  256 workgroups, one LDS tree per workgroup, then one tree over the workgroups' sums (two launches, no
 *                  atomics).  `work`: VUNET_F64_DOT_WORK doubles.
 * vunet_f64_scale  y[i] = alpha * x[i], n values; y may be x.
 * vunet_f64_symmetrize
 *                  a [n][n] with leading dimension ld, in place: a[i][j] = a[j][i] = 0.5 * (a[i][j] + a[j][i]).
 * All: no allocation, no synchronisation, no atomics.  VUNET_ERR_ARG: a NULL pointer, a size < 1 (N < 2 for the centring), a
 * leading dimension smaller than its row, a transpose flag outside {0, 1}.
 */
#ifndef VUNET_FID_H
#define VUNET_FID_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VUNET_F64_DOT_WORK 256

int vunet_f64_gemm(const double* A, int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc, int32_t M, int32_t N,
                   int32_t K, int32_t trans_a, int32_t trans_b, double alpha, double diag, void* stream);

int vunet_fid_center(const float* feats, int32_t N, int32_t D, double* mu, double* Y, void* stream);

int vunet_fid_center_f64(const double* feats, int32_t N, int32_t D, double* mu, double* Y, void* stream);

int vunet_f64_dot(const double* a, const double* b, int64_t n, double* work, double* out, void* stream);

int vunet_f64_scale(const double* x, int64_t n, double alpha, double* y, void* stream);

int vunet_f64_symmetrize(double* a, int32_t n, int64_t ld, void* stream);

#ifdef __cplusplus
}
#endif
#endif
