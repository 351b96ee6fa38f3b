// The Inception score's statistic on the device: logits [N][K] -> one float64 score per split.  Interface: vunet_inception_score in
// include/vunet_inception.h; the arithmetic restates lib/metrics.py:403-415 with scipy.stats.entropy(pk, qk).
//
// Four launches on the caller's stream, float64 throughout, every sum in a fixed order (per-thread strided partial sums, then one
// LDS tree: two stages, no atomics), so two runs agree bit for bit:
//   1. is_row_stats_kernel   one workgroup per row: m = max, s = sum exp(l - m), t = sum_k p_k with p_k = exp(l_k - m) / s
//                            (scipy renormalises pk; t is 1 up to rounding).
//   2. is_col_mean_kernel    one thread per (split, column): q_k = (sum over the split's rows, in row order, of p_ik) / rows.
//   3. is_row_kl_kernel      one workgroup per row: Q = sum_k q_k, then KL_i = sum_k ph log(ph / qh), ph = p_ik / t_i, qh = q_k / Q,
//                            a term with ph == 0 contributing 0.
//   4. is_split_kernel       one workgroup per split: exp(mean_i KL_i).
// The exponentials are recomputed in 2 and 3 instead of stored: N K doubles would be 64 MB at 8000 x 1000, the logits are 32 MB.
#include "common.h"
#include "../../include/vunet_inception.h"

namespace {

constexpr int T = 256;

// fixed tree over the workgroup's 256 values; every thread gets the result
template <bool MAX>
__device__ __forceinline__ double block_reduce(double v, double* lds) {
  const int t = threadIdx.x;
  __syncthreads();   // lds may still be read from the previous reduction
  lds[t] = v;
  __syncthreads();
#pragma unroll
  for (int o = T / 2; o > 0; o >>= 1) {
    if (t < o) lds[t] = MAX ? fmax(lds[t], lds[t + o]) : lds[t] + lds[t + o];
    __syncthreads();
  }
  return lds[0];
}

__global__ __launch_bounds__(T) void is_row_stats_kernel(const float* __restrict__ logits, int K, double* __restrict__ stats) {
#pragma clang fp contract(off)
  __shared__ double lds[T];
  const int64_t i = blockIdx.x;
  const float* l = logits + i * K;
  double m = -__builtin_huge_val();
  for (int k = threadIdx.x; k < K; k += T) m = fmax(m, (double)l[k]);
  m = block_reduce<true>(m, lds);
  double s = 0.0;
  for (int k = threadIdx.x; k < K; k += T) s += exp((double)l[k] - m);
  s = block_reduce<false>(s, lds);
  double t = 0.0;
  for (int k = threadIdx.x; k < K; k += T) t += exp((double)l[k] - m) / s;
  t = block_reduce<false>(t, lds);
  if (threadIdx.x == 0) {
    stats[3 * i] = m;
    stats[3 * i + 1] = s;
    stats[3 * i + 2] = t;
  }
}

__global__ __launch_bounds__(T) void is_col_mean_kernel(const float* __restrict__ logits, int K, int rows, const double* __restrict__ stats,
                                                        double* __restrict__ q) {
#pragma clang fp contract(off)
  const int k = blockIdx.x * T + threadIdx.x, split = blockIdx.y;
  if (k >= K) return;
  const int64_t first = (int64_t)split * rows;
  double acc = 0.0;
  for (int64_t i = first; i < first + rows; ++i) acc += exp((double)logits[i * K + k] - stats[3 * i]) / stats[3 * i + 1];
  q[(int64_t)split * K + k] = acc / (double)rows;
}

__global__ __launch_bounds__(T) void is_row_kl_kernel(const float* __restrict__ logits, int K, int rows, const double* __restrict__ stats,
                                                      const double* __restrict__ q, double* __restrict__ kl) {
#pragma clang fp contract(off)
  __shared__ double lds[T];
  const int64_t i = blockIdx.x;   // < splits * rows: the tail rows belong to no split
  const double* qs = q + (i / rows) * K;
  const float* l = logits + i * K;
  double Q = 0.0;
  for (int k = threadIdx.x; k < K; k += T) Q += qs[k];
  Q = block_reduce<false>(Q, lds);
  const double m = stats[3 * i], s = stats[3 * i + 1], t = stats[3 * i + 2];
  double acc = 0.0;
  for (int k = threadIdx.x; k < K; k += T) {
    const double ph = (exp((double)l[k] - m) / s) / t;
    if (ph > 0.0) acc += ph * log(ph / (qs[k] / Q));
  }
  acc = block_reduce<false>(acc, lds);
  if (threadIdx.x == 0) kl[i] = acc;
}

__global__ __launch_bounds__(T) void is_split_kernel(const double* __restrict__ kl, int rows, double* __restrict__ scores) {
#pragma clang fp contract(off)
  __shared__ double lds[T];
  const int64_t first = (int64_t)blockIdx.x * rows;
  double acc = 0.0;
  for (int i = threadIdx.x; i < rows; i += T) acc += kl[first + i];
  acc = block_reduce<false>(acc, lds);
  if (threadIdx.x == 0) scores[blockIdx.x] = exp(acc / (double)rows);   // rows == 0: 0 / 0, not a number, as the reference's empty mean
}

}  // namespace

extern "C" int vunet_inception_score(const float* logits, int32_t N, int32_t K, int32_t splits, double* work, double* scores,
                                     void* stream) {
  if (!logits || !work || !scores || N < 1 || K < 1 || splits < 1 || splits > 65535 || (int64_t)N * K >= ((int64_t)1 << 31) ||
      (int64_t)splits * K >= ((int64_t)1 << 31))
    return VUNET_ERR_ARG;
  const int rows = N / splits;
  double* stats = work;                         // [N][3]
  double* kl = work + 3 * (int64_t)N;           // [N]
  double* q = work + 4 * (int64_t)N;            // [splits][K]
  hipStream_t st = (hipStream_t)stream;
  if (rows > 0) {
    const unsigned used = (unsigned)(rows * splits);
    VUNET_LAUNCH(is_row_stats_kernel, dim3(used), dim3(T), 0, st, logits, (int)K, stats);
    if (vunet_check_launch() != VUNET_OK) return VUNET_ERR_LAUNCH;
    VUNET_LAUNCH(is_col_mean_kernel, dim3((unsigned)((K + T - 1) / T), (unsigned)splits), dim3(T), 0, st, logits, (int)K, rows, stats, q);
    if (vunet_check_launch() != VUNET_OK) return VUNET_ERR_LAUNCH;
    VUNET_LAUNCH(is_row_kl_kernel, dim3(used), dim3(T), 0, st, logits, (int)K, rows, stats, q, kl);
    if (vunet_check_launch() != VUNET_OK) return VUNET_ERR_LAUNCH;
  }
  VUNET_LAUNCH(is_split_kernel, dim3((unsigned)splits), dim3(T), 0, st, kl, rows, scores);
  return vunet_check_launch();
}
