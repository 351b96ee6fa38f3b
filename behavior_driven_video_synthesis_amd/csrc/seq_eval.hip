// The behaviour model's sampling metrics (experiments/behavior_net.py:1238-1255, lib/logging.py:2079-2093).  Interface:
// include/vunet_seq_eval.h.
//
// The reference copies every sampled sequence to the host, un-normalises it in numpy and then builds, per sequence and per
// sample q, a row of distances to the other samples with two host syncs per row.  Here:
//   * seq_eval_pairs_kernel: one workgroup per (sequence, q).  Sample q, un-normalised, sits in LDS; each wave takes samples
//     s = wave, wave + 4, ... (s = S is the ground truth) and streams them from global memory (the whole batch is L2-resident).
//     Lanes run over the frames: a lane sums its frame's n squared differences itself, so the only cross-lane reductions are the
//     two per pair (sum of d_t, sum of d_t^2), a fixed butterfly.
//   * seq_eval_select_kernel: one workgroup, a wave per sequence: the np.sort(...)[1] selections, the row sums of P, the
//     NaN-propagating minima and the batch means, every sum in a fixed order.
// No atomics, no hand-off between workgroups: the two launches are deterministic.
#include "common.h"
#include "../../include/vunet_seq_eval.h"

namespace {

// unNormalizeData (data/data_conversions_3d.py:178-211) of one used dimension, with numpy's promotion: float32 statistics keep
// x * std + mean in float32, float64 ones in float64.  Two roundings, as numpy does: no fused multiply-add.
__device__ __forceinline__ double unnormalise(float v, double sd, double m, int f32) {
#pragma clang fp contract(off)
  if (f32) return (double)(v * (float)sd + (float)m);
  return (double)v * sd + m;
}

// the difference of two un-normalised values in the statistics' precision (exact in float64 for the float32 case's operands)
__device__ __forceinline__ double pose_diff(double a, double b, int f32) {
  return f32 ? (double)((float)a - (float)b) : a - b;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);   // butterfly: every lane ends with the same value
  return v;
}

__device__ __forceinline__ double nan_min(double a, double b) {   // torch.min: NaN wins
  return (a != a || b != b) ? __longlong_as_double(0x7ff8000000000000LL) : fmin(a, b);
}

__device__ __forceinline__ double wave_nan_min(double v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v = nan_min(v, __shfl_xor(v, o));
  return v;
}

// element [1] of the row sorted ascending with NaN last (np.sort): the second smallest finite-or-infinite value counted with
// multiplicity, NaN when fewer than two values are not NaN
__device__ __forceinline__ double second_smallest(const double* __restrict__ row, int S) {
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  double m1 = inf, m2 = inf;
  int cnt = 0;
  for (int s = 0; s < S; ++s) {
    const double v = row[s];
    if (v != v) continue;
    ++cnt;
    if (v < m1) {
      m2 = m1;
      m1 = v;
    } else if (v < m2) {
      m2 = v;
    }
  }
  return cnt >= 2 ? m2 : __longlong_as_double(0x7ff8000000000000LL);
}

__global__ __launch_bounds__(256) void seq_eval_pairs_kernel(const float* __restrict__ x, const float* __restrict__ future,
                                                             const double* __restrict__ mean, const double* __restrict__ stdv, int f32,
                                                             int N, int S, int T, int n, double* __restrict__ scratch) {
  extern __shared__ double uq[];   // [T][n]: sample q un-normalised
  const int q = blockIdx.x, i = blockIdx.y;
  const int TN = T * n;
  const float* xi = x + (size_t)i * S * TN;
  const float* xq = xi + (size_t)q * TN;
  for (int k = threadIdx.x; k < TN; k += 256) {
    const int d = k % n;
    uq[k] = unnormalise(xq[k], stdv[d], mean[d], f32);
  }
  __syncthreads();
  const size_t SS = (size_t)S * S, NSS = (size_t)N * SS, NS = (size_t)N * S;
  double* A = scratch + ((size_t)i * S + q) * S;
  double* F = A + NSS;
  double* P = A + 2 * NSS;
  double* G = scratch + 3 * NSS + (size_t)i * S + q;
  double* GF = G + NS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int s = wave; s <= S; s += 4) {
    // s == S: the ground truth, frames 1 .. T of the future sequence
    const float* xs = s < S ? xi + (size_t)s * TN : future + ((size_t)i * (T + 1) + 1) * n;
    double sum_d = 0.0, sum_sq = 0.0, last = 0.0;
    for (int t = lane; t < T; t += 64) {
      const double* a = uq + t * n;
      const float* b = xs + (size_t)t * n;
      double sq = 0.0;
      for (int d = 0; d < n; ++d) {
        const double e = pose_diff(a[d], unnormalise(b[d], stdv[d], mean[d], f32), f32);
        sq += e * e;
      }
      const double dt = sqrt(sq);
      sum_d += dt;
      sum_sq += sq;
      if (t == T - 1) last = dt;
    }
    sum_d = wave_sum(sum_d);
    sum_sq = wave_sum(sum_sq);
    last = __shfl(last, (T - 1) & 63);
    if (lane == 0) {
      if (s < S) {
        A[s] = sum_d / (double)T;
        F[s] = last;
        P[s] = sqrt(sum_sq);
      } else {
        *G = sum_d / (double)T;
        *GF = last;
      }
    }
  }
}

__global__ __launch_bounds__(256) void seq_eval_select_kernel(const double* __restrict__ scratch, int N, int S, double* __restrict__ per_seq,
                                                              double* __restrict__ batch) {
  extern __shared__ double mins[];   // [2][N]: minADE, minFDE per sequence
  const size_t NSS = (size_t)N * S * S, NS = (size_t)N * S;
  const double *A = scratch, *F = scratch + NSS, *P = scratch + 2 * NSS, *G = scratch + 3 * NSS, *GF = G + NS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  for (int i = wave; i < N; i += 4) {
    double asd = 0.0, fsd = 0.0, apd = 0.0, g = inf, gf = inf;
    for (int q = lane; q < S; q += 64) {
      const size_t r = ((size_t)i * S + q) * S;
      asd += second_smallest(A + r, S);
      fsd += second_smallest(F + r, S);
      double p = 0.0;
      for (int s = 0; s < S; ++s) p += P[r + s];
      apd += p / (double)(S - 1);
      g = nan_min(g, G[(size_t)i * S + q]);
      gf = nan_min(gf, GF[(size_t)i * S + q]);
    }
    asd = wave_sum(asd);
    fsd = wave_sum(fsd);
    apd = wave_sum(apd);
    g = wave_nan_min(g);
    gf = wave_nan_min(gf);
    if (lane == 0) {
      per_seq[i] = apd / (double)S;
      per_seq[N + i] = asd / (double)S;
      per_seq[2 * N + i] = fsd / (double)S;
      per_seq[3 * N + i] = g;
      per_seq[4 * N + i] = gf;
      mins[i] = g;
      mins[N + i] = gf;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double ade = 0.0, fde = 0.0;
    for (int i = 0; i < N; ++i) {
      ade += mins[i];
      fde += mins[N + i];
    }
    batch[0] = ade / (double)N;
    batch[1] = fde / (double)N;
  }
}

}  // namespace

extern "C" int vunet_seq_eval_pairs(const float* x, const float* future, const double* mean, const double* stdv, int32_t f32_math,
                                    int32_t N, int32_t S, int32_t T, int32_t n, double* scratch, void* stream) {
  if (!x || !future || !mean || !stdv || !scratch || N < 1 || S < 2 || T < 1 || n < 1 || N > 65535 || S > 65535) return VUNET_ERR_ARG;
  if ((int64_t)T * n > VUNET_SEQ_EVAL_MAX_TN) return VUNET_ERR_UNSUPPORTED;
  VUNET_LAUNCH(seq_eval_pairs_kernel, dim3((unsigned)S, (unsigned)N), dim3(256), (size_t)T * n * sizeof(double), (hipStream_t)stream,
               x, future, mean, stdv, f32_math ? 1 : 0, N, S, T, n, scratch);
  return vunet_check_launch();
}

extern "C" int vunet_seq_eval_select(const double* scratch, int32_t N, int32_t S, double* per_seq, double* batch, void* stream) {
  if (!scratch || !per_seq || !batch || N < 1 || S < 2 || N > 4096) return VUNET_ERR_ARG;
  VUNET_LAUNCH(seq_eval_select_kernel, dim3(1), dim3(256), (size_t)2 * N * sizeof(double), (hipStream_t)stream, scratch, N, S, per_seq,
               batch);
  return vunet_check_launch();
}
