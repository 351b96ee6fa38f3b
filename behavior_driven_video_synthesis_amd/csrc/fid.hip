// The FID statistic's float64 building blocks on the device.  Interface: include/vunet_fid.h; the derivation that turns
// |mu1 - mu2|^2 + tr S1 + tr S2 - 2 tr sqrtm(S1 S2) into matrix products only is DESIGN.md 4 ("FID by a polar iteration").
//
//   f64_gemm_kernel   C = alpha op(A) op(B) + diag I on v_mfma_f64_16x16x4_f64.  One workgroup (4 waves) per 64 x 64 tile of C,
//                     each wave a 32 x 32 quarter (2 x 2 MFMA tiles, 16 accumulator doubles per lane).  K is walked in steps of 16:
//                     the next step's operands are fetched into registers (zero where the tile leaves the matrix) while the
//                     current step's 16 MFMAs run from LDS.  Both operands sit in LDS k-major, As[k][m] and Bs[k][n], so
//                     a fragment read is 16 consecutive doubles per k row whichever way the operand lies in memory; rows are
//                     padded to 80 doubles, which puts the four k rows a wave reads at once on disjoint bank halves (an f64
//                     spans two banks).  The instruction's lane map (NOT the f32 16x16x4 one for C/D):
//                       A: lane l holds op(A)[row l & 15][k l >> 4];  B: op(B)[k l >> 4][col l & 15];
//                       C/D: register r of lane l is C[row (l >> 4) + 4 r][col l & 15].
//                     One fixed summation order per element: no split-K, no atomics.
//   col_mean_kernel / center_kernel   column means (16 strided partials per column + a tree) and Y = (x - mu) / sqrt(N - 1).
//   dot_partial_kernel / dot_final_kernel   sum a * b: strided partials, a tree per workgroup, a tree over the workgroups.
//   scale_kernel, symmetrize_kernel   the two element-wise passes the iteration needs besides the GEMM's alpha / diag epilogue.
#include "common.h"
#include "../../include/vunet_fid.h"

namespace {

typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int T = 256;       // threads per workgroup, every kernel here
constexpr int BT = 64;       // C tile edge
constexpr int KT = 16;       // K step
constexpr int LS = 80;       // LDS row stride in doubles: 64 + 16, see above

// fixed tree over the workgroup's 256 values; thread 0's return value is the sum
__device__ __forceinline__ double block_sum(double v, double* lds) {
  const int t = threadIdx.x;
  lds[t] = v;
  __syncthreads();
#pragma unroll
  for (int o = T / 2; o > 0; o >>= 1) {
    if (t < o) lds[t] = lds[t] + lds[t + o];
    __syncthreads();
  }
  return lds[0];
}

// One operand's 64 x 16 tile, four elements per thread.  KC: k is the contiguous axis in memory (A not transposed, B
// transposed): 16 consecutive k per row of 16 lanes; else the tile's other axis x is (A transposed, B not): 64 consecutive x
// per wave.  Element (x, k) lies at p[x * ld + k] (KC) or p[k * ld + x].  Outside X x K: zero, and no load.
template <bool KC>
__device__ __forceinline__ void tile_fetch(const double* __restrict__ p, int64_t ld, int x0, int k0, int X, int K, double (&r)[4]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int gx = x0 + (KC ? (t >> 4) + 16 * i : (t & 63));
    const int gk = k0 + (KC ? (t & 15) : (t >> 6) + 4 * i);
    r[i] = (gx < X && gk < K) ? p[KC ? (int64_t)gx * ld + gk : (int64_t)gk * ld + gx] : 0.0;
  }
}

template <bool KC>
__device__ __forceinline__ void tile_store(double* __restrict__ s, const double (&r)[4]) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int x = KC ? (t >> 4) + 16 * i : (t & 63);
    const int k = KC ? (t & 15) : (t >> 6) + 4 * i;
    s[k * LS + x] = r[i];
  }
}

template <bool AKC, bool BKC>
__global__ __launch_bounds__(T) void f64_gemm_kernel(const double* __restrict__ A, int64_t lda, const double* __restrict__ B, int64_t ldb,
                                                     double* __restrict__ C, int64_t ldc, int M, int N, int K, double alpha, double diag) {
#pragma clang fp contract(off)
  __shared__ double As[KT * LS];
  __shared__ double Bs[KT * LS];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int lr = lane & 15, lk = lane >> 4;
  const int wm = (w >> 1) * 32, wn = (w & 1) * 32;
  const int m0 = blockIdx.y * BT, n0 = blockIdx.x * BT;

  f64x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f64x4{0.0, 0.0, 0.0, 0.0};

  double ra[4], rb[4];
  tile_fetch<AKC>(A, lda, m0, 0, M, K, ra);
  tile_fetch<BKC>(B, ldb, n0, 0, N, K, rb);
  for (int k0 = 0; k0 < K; k0 += KT) {
    tile_store<AKC>(As, ra);
    tile_store<BKC>(Bs, rb);
    __syncthreads();
    if (k0 + KT < K) {   // uniform across the workgroup
      tile_fetch<AKC>(A, lda, m0, k0 + KT, M, K, ra);
      tile_fetch<BKC>(B, ldb, n0, k0 + KT, N, K, rb);
    }
#pragma unroll
    for (int kk = 0; kk < KT; kk += 4) {
      const double* as = As + (kk + lk) * LS + wm + lr;
      const double* bs = Bs + (kk + lk) * LS + wn + lr;
      const double a0 = as[0], a1 = as[16], b0 = bs[0], b1 = bs[16];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();   // every wave is done with this step's tiles before the next store
  }

#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = m0 + wm + 16 * i + lk + 4 * r, col = n0 + wn + 16 * j + lr;
        if (row < M && col < N) {
          double v = alpha * acc[i][j][r];
          if (row == col) v = v + diag;
          C[(int64_t)row * ldc + col] = v;
        }
      }
}

// 16 columns x 16 row lanes per workgroup: lane ry sums rows ry, ry + 16, ... of its column in that order, then a tree over ry
template <typename TI>
__global__ __launch_bounds__(T) void col_mean_kernel(const TI* __restrict__ x, int N, int D, double* __restrict__ mu) {
#pragma clang fp contract(off)
  __shared__ double lds[16][17];
  const int cx = threadIdx.x & 15, ry = threadIdx.x >> 4;
  const int c = blockIdx.x * 16 + cx;
  double acc = 0.0;
  if (c < D)
    for (int r = ry; r < N; r += 16) acc += (double)x[(int64_t)r * D + c];
  lds[ry][cx] = acc;
  __syncthreads();
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) {
    if (ry < o) lds[ry][cx] = lds[ry][cx] + lds[ry + o][cx];
    __syncthreads();
  }
  if (ry == 0 && c < D) mu[c] = lds[0][cx] / (double)N;
}

template <typename TI>
__global__ __launch_bounds__(T) void center_kernel(const TI* __restrict__ x, int64_t total, int D, const double* __restrict__ mu, double s,
                                                   double* __restrict__ Y) {
#pragma clang fp contract(off)
  const int64_t stride = (int64_t)gridDim.x * T;
  for (int64_t i = (int64_t)blockIdx.x * T + threadIdx.x; i < total; i += stride) Y[i] = ((double)x[i] - mu[i % D]) / s;
}

__global__ __launch_bounds__(T) void dot_partial_kernel(const double* __restrict__ a, const double* __restrict__ b, int64_t n,
                                                        double* __restrict__ work) {
#pragma clang fp contract(off)
  __shared__ double lds[T];
  const int64_t stride = (int64_t)gridDim.x * T;
  double acc = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * T + threadIdx.x; i < n; i += stride) acc += a[i] * b[i];
  acc = block_sum(acc, lds);
  if (threadIdx.x == 0) work[blockIdx.x] = acc;
}

__global__ __launch_bounds__(T) void dot_final_kernel(const double* __restrict__ work, int G, double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double lds[T];
  const double v = block_sum((int)threadIdx.x < G ? work[threadIdx.x] : 0.0, lds);
  if (threadIdx.x == 0) out[0] = v;
}

__global__ __launch_bounds__(T) void scale_kernel(const double* x, int64_t n, double alpha, double* y) {
  const int64_t stride = (int64_t)gridDim.x * T;
  for (int64_t i = (int64_t)blockIdx.x * T + threadIdx.x; i < n; i += stride) y[i] = alpha * x[i];
}

// one thread per pair i < j; the diagonal stays
__global__ __launch_bounds__(T) void symmetrize_kernel(double* __restrict__ a, int n, int64_t ld) {
#pragma clang fp contract(off)
  if (blockIdx.x < blockIdx.y) return;   // the tile lies below the diagonal
  const int j = blockIdx.x * 16 + (threadIdx.x & 15), i = blockIdx.y * 16 + (threadIdx.x >> 4);
  if (i < j && j < n) {
    const double v = 0.5 * (a[(int64_t)i * ld + j] + a[(int64_t)j * ld + i]);
    a[(int64_t)i * ld + j] = v;
    a[(int64_t)j * ld + i] = v;
  }
}

inline unsigned stride_blocks(int64_t n, int64_t cap) {
  const int64_t b = (n + T - 1) / T;
  return (unsigned)(b < cap ? b : cap);
}

template <typename TI>
int fid_center(const TI* feats, int32_t N, int32_t D, double* mu, double* Y, void* stream) {
  if (!feats || !mu || !Y || N < 2 || D < 1) return VUNET_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  VUNET_LAUNCH(col_mean_kernel<TI>, dim3((unsigned)((D + 15) / 16)), dim3(T), 0, st, feats, (int)N, (int)D, mu);
  if (vunet_check_launch() != VUNET_OK) return VUNET_ERR_LAUNCH;
  const int64_t total = (int64_t)N * D;
  VUNET_LAUNCH(center_kernel<TI>, dim3(stride_blocks(total, 8192)), dim3(T), 0, st, feats, total, (int)D, (const double*)mu,
               sqrt((double)(N - 1)), Y);
  return vunet_check_launch();
}

}  // namespace

extern "C" int vunet_f64_gemm(const double* A, int64_t lda, const double* B, int64_t ldb, double* C, int64_t ldc, int32_t M, int32_t N,
                              int32_t K, int32_t trans_a, int32_t trans_b, double alpha, double diag, void* stream) {
  if (!A || !B || !C || M < 1 || N < 1 || K < 1 || (trans_a != 0 && trans_a != 1) || (trans_b != 0 && trans_b != 1) ||
      lda < (trans_a ? M : K) || ldb < (trans_b ? K : N) || ldc < N)
    return VUNET_ERR_ARG;
  const dim3 grid((unsigned)((N + BT - 1) / BT), (unsigned)((M + BT - 1) / BT));
  if (grid.y > 65535u) return VUNET_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  // A not transposed: k contiguous; B not transposed: n contiguous
  if (!trans_a && !trans_b)
    VUNET_LAUNCH((f64_gemm_kernel<true, false>), grid, dim3(T), 0, st, A, lda, B, ldb, C, ldc, (int)M, (int)N, (int)K, alpha, diag);
  else if (trans_a && !trans_b)
    VUNET_LAUNCH((f64_gemm_kernel<false, false>), grid, dim3(T), 0, st, A, lda, B, ldb, C, ldc, (int)M, (int)N, (int)K, alpha, diag);
  else if (!trans_a && trans_b)
    VUNET_LAUNCH((f64_gemm_kernel<true, true>), grid, dim3(T), 0, st, A, lda, B, ldb, C, ldc, (int)M, (int)N, (int)K, alpha, diag);
  else
    VUNET_LAUNCH((f64_gemm_kernel<false, true>), grid, dim3(T), 0, st, A, lda, B, ldb, C, ldc, (int)M, (int)N, (int)K, alpha, diag);
  return vunet_check_launch();
}

extern "C" int vunet_fid_center(const float* feats, int32_t N, int32_t D, double* mu, double* Y, void* stream) {
  return fid_center<float>(feats, N, D, mu, Y, stream);
}

extern "C" int vunet_fid_center_f64(const double* feats, int32_t N, int32_t D, double* mu, double* Y, void* stream) {
  return fid_center<double>(feats, N, D, mu, Y, stream);
}

extern "C" int vunet_f64_dot(const double* a, const double* b, int64_t n, double* work, double* out, void* stream) {
  if (!a || !b || !work || !out || n < 1) return VUNET_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const unsigned G = stride_blocks(n, VUNET_F64_DOT_WORK);
  VUNET_LAUNCH(dot_partial_kernel, dim3(G), dim3(T), 0, st, a, b, n, work);
  if (vunet_check_launch() != VUNET_OK) return VUNET_ERR_LAUNCH;
  VUNET_LAUNCH(dot_final_kernel, dim3(1), dim3(T), 0, st, (const double*)work, (int)G, out);
  return vunet_check_launch();
}

extern "C" int vunet_f64_scale(const double* x, int64_t n, double alpha, double* y, void* stream) {
  if (!x || !y || n < 1) return VUNET_ERR_ARG;
  VUNET_LAUNCH(scale_kernel, dim3(stride_blocks(n, 8192)), dim3(T), 0, (hipStream_t)stream, x, n, alpha, y);
  return vunet_check_launch();
}

extern "C" int vunet_f64_symmetrize(double* a, int32_t n, int64_t ld, void* stream) {
  if (!a || n < 1 || ld < n) return VUNET_ERR_ARG;
  const unsigned g = (unsigned)((n + 15) / 16);
  if (g > 65535u) return VUNET_ERR_ARG;
  VUNET_LAUNCH(symmetrize_kernel, dim3(g, g), dim3(T), 0, (hipStream_t)stream, a, (int)n, ld);
  return vunet_check_launch();
}
