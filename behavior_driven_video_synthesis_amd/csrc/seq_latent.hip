// The latent diagnostics of the behaviour model's evaluation loop (lib/logging.py eval_nets :2228-2262, :2549-2562;
// lib/losses.py:295-311, :330-331).  Interface: include/vunet_seq_latent.h.
//
// The reference evaluates FlowLoss in fp32 torch per batch, and runs the Gaussianity check as a host loop of one
// scipy.stats.kstest per code dimension over up to 20 000 rows after copying every code to the host.  Here:
//   * latent_nll_rows_kernel / latent_nll_reduce_kernel: a wave per row sums z^2 (and the reference draw's) in float64 with a
//     fixed butterfly; one workgroup then adds the rows in a fixed order (a thread's rows in row order, then a tree over the
//     threads) and turns the noise rows' slot into log_prob.  Any number of rows.
//   * ks_norm_kernel: one workgroup owns G columns of P = next power of two >= N slots each, all in LDS.  Values become
//     order-preserving unsigned keys, the slots past N hold the largest key, a bitonic network sorts every column ascending (the
//     direction bit is taken from the index INSIDE the column, so all G columns of the shared array end up ascending), and the
//     column's waves take the two maxima of the statistic over the first N slots (key mapping, padding,
//     which steps run in registers, the LDS budget).  The column's first thread sums the
//     Kolmogorov series.  At the cap (32768 values, 128 KiB of keys) a workgroup is 1024 threads and owns one column -- the CU
//     has 160 KiB of LDS, a second column does not fit; up to 4096 values a workgroup is 256 threads over 2048 slots or one
//     column, so short columns neither pay for the cap's slots nor leave a CU to one workgroup.
// Only max reductions and fixed-order sums, no atomics: both entry points are bit-identical from run to run.
#include "common.h"
#include "../../include/vunet_seq_latent.h"

namespace {

constexpr double LOG_2PI = 1.8378770664093454835606594728112;
constexpr double PI = 3.14159265358979323846264338327950288;

__device__ __forceinline__ double qnan() { return __longlong_as_double(0x7ff8000000000000LL); }

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);   // butterfly: a fixed order, every lane ends with the same value
  return v;
}

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
  for (int o = 32; o; o >>= 1) v = fmax(v, __shfl_xor(v, o));
  return v;
}

// ---- FlowLoss entries

__global__ __launch_bounds__(256) void latent_nll_rows_kernel(const float* __restrict__ z, int64_t ldz, const float* __restrict__ noise,
                                                              int B, int C, double* __restrict__ per_row) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t row = (int64_t)blockIdx.x * 4 + wave;
  if (row >= B) return;
  const float* zr = z + row * ldz;
  double s = 0.0;
  for (int c = lane; c < C; c += 64) {
    const double v = (double)zr[c];
    s += v * v;
  }
  s = wave_sum_f64(s);
  double r = qnan();
  if (noise) {
    const float* nr = noise + row * (int64_t)C;
    r = 0.0;
    for (int c = lane; c < C; c += 64) {
      const double v = (double)nr[c];
      r += v * v;
    }
    r = 0.5 * wave_sum_f64(r);
  }
  if (lane == 0) {
    per_row[row] = 0.5 * s;
    per_row[(int64_t)B + row] = r;   // the noise row's value until the reduce launch replaces it by log_prob
  }
}

__global__ __launch_bounds__(256) void latent_nll_reduce_kernel(const float* __restrict__ logdet, int B, int C, double* __restrict__ per_row,
                                                                double* __restrict__ scalars) {
  __shared__ double red[3][256];
  const int t = threadIdx.x;
  double a = 0.0, l = 0.0, r = 0.0;
  const double cst = 0.5 * (double)C * LOG_2PI;
  for (int64_t i = t; i < B; i += 256) {
    const double nll = per_row[i], ld = (double)logdet[i];
    a += nll;
    l += ld;
    r += per_row[(int64_t)B + i];
    per_row[(int64_t)B + i] = -nll + ld - cst;
  }
  red[0][t] = a;
  red[1][t] = l;
  red[2][t] = r;
  __syncthreads();
  for (int o = 128; o; o >>= 1) {
    if (t < o) {
      red[0][t] += red[0][t + o];
      red[1][t] += red[1][t + o];
      red[2][t] += red[2][t + o];
    }
    __syncthreads();
  }
  if (t == 0) {
    const double nll_loss = red[0][0] / (double)B, nlogdet = -(red[1][0] / (double)B);
    scalars[0] = nll_loss + nlogdet;
    scalars[1] = red[2][0] / (double)B;
    scalars[2] = nlogdet;
    scalars[3] = nll_loss;
  }
}

// ---- Kolmogorov-Smirnov

// float -> unsigned key with the same order: negative values flip every bit, the others set the sign bit.  -inf < ... < -0 < +0 <
// ... < +inf < (positive NaNs); the padding key 0xffffffff is not below any of them.
__device__ __forceinline__ uint32_t key_of(float v) {
  const uint32_t u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float value_of(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// the asymptotic two-sided p-value: the Kolmogorov distribution's survival function at t = D sqrt(N)
__device__ double kolmogorov_sf(double t) {
  if (!(t > 0.0)) return t != t ? t : 1.0;
  double p;
  if (t < 0.2) {   // the alternating series cancels here: the theta-function form of the cdf (its terms vanish fast for small t)
    const double w = PI * PI / (8.0 * t * t);
    double s = 0.0;
    for (int k = 1; k <= 256; ++k) {
      const double m = (double)(2 * k - 1), term = exp(-m * m * w);
      s += term;
      if (term < 1e-17) break;
    }
    p = 1.0 - sqrt(2.0 * PI) / t * s;
  } else {
    double s = 0.0, sign = 1.0;
    for (int k = 1; k <= 256; ++k) {
      const double term = exp(-2.0 * (double)k * (double)k * t * t);
      s += sign * term;
      sign = -sign;
      if (term < 1e-17) break;
    }
    p = 2.0 * s;
  }
  return fmin(fmax(p, 0.0), 1.0);
}

constexpr int KS_RUN = 16;   // slots a thread sorts in registers: the steps of distance < KS_RUN stay inside an aligned run

// one step of distance J on a run held in registers; `base` is the run's first slot, `dir` the phase's direction bit
template <int J>
__device__ __forceinline__ void ks_run_step(uint32_t (&r)[KS_RUN], int base, int dir) {
#pragma unroll
  for (int m = 0; m < KS_RUN / 2; ++m) {
    const int i = ((m & ~(J - 1)) << 1) | (m & (J - 1)), l = i + J;
    const bool asc = ((base + i) & dir) == 0;
    const uint32_t a = r[i], b = r[l];
    const bool sw = (a > b) == asc;
    r[i] = sw ? b : a;
    r[l] = sw ? a : b;
  }
}

// k == 2: the phases 2, 4, 8, 16 whole; else the last four steps (distance 8, 4, 2, 1) of phase k.  P >= KS_RUN.
template <int THREADS>
__device__ __forceinline__ void ks_run_pass(uint32_t* keys, int total, int P, int k, int tid) {
  for (int base = tid * KS_RUN; base < total; base += THREADS * KS_RUN) {
    uint4* q = reinterpret_cast<uint4*>(keys + base);   // (the keys start 16-byte aligned and a run is 64 bytes)
    uint32_t r[KS_RUN];
#pragma unroll
    for (int v = 0; v < KS_RUN / 4; ++v) {
      const uint4 t = q[v];
      r[4 * v] = t.x;
      r[4 * v + 1] = t.y;
      r[4 * v + 2] = t.z;
      r[4 * v + 3] = t.w;
    }
    if (k == 2) {
      ks_run_step<1>(r, base, 2);
      ks_run_step<2>(r, base, 4);
      ks_run_step<1>(r, base, 4);
      ks_run_step<4>(r, base, 8);
      ks_run_step<2>(r, base, 8);
      ks_run_step<1>(r, base, 8);
    }
    const int dir = (k == 2 ? KS_RUN : k) & (P - 1);
    ks_run_step<8>(r, base, dir);
    ks_run_step<4>(r, base, dir);
    ks_run_step<2>(r, base, dir);
    ks_run_step<1>(r, base, dir);
#pragma unroll
    for (int v = 0; v < KS_RUN / 4; ++v) q[v] = make_uint4(r[4 * v], r[4 * v + 1], r[4 * v + 2], r[4 * v + 3]);
  }
}

// LDS: [2][THREADS / 64] doubles (the waves' maxima) | 16 ints (a NaN flag per column of the workgroup) | G P keys
template <int THREADS>
__global__ __launch_bounds__(THREADS) void ks_norm_kernel(const float* __restrict__ x, int64_t ld, int col_major, int N, int C, int sorted,
                                                          int P, int G, double* __restrict__ stat, double* __restrict__ p_asym) {
  constexpr int WAVES = THREADS / 64;
  extern __shared__ __attribute__((aligned(16))) unsigned char ks_smem[];
  double* red = reinterpret_cast<double*>(ks_smem);
  int* nanflag = reinterpret_cast<int*>(red + 2 * WAVES);
  uint32_t* keys = reinterpret_cast<uint32_t*>(nanflag + 16);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tpc = THREADS / G;           // threads per column: G <= WAVES, a column owns whole waves
  const int g = tid / tpc, lt = tid - g * tpc;
  const int64_t c0 = (int64_t)blockIdx.x * G, col = c0 + g;
  if (tid < 16) nanflag[tid] = 0;
  __syncthreads();
  if (!sorted) {
    const int total = G * P;
    if (col_major) {
      for (int i = lt; i < P; i += tpc) {
        uint32_t k = 0xffffffffu;
        if (i < N && col < C) {
          const float v = x[col * ld + i];
          if (v != v) nanflag[g] = 1;
          k = key_of(v);
        }
        keys[g * P + i] = k;
      }
    } else {   // consecutive threads take consecutive columns of one row
      for (int idx = tid; idx < total; idx += THREADS) {
        const int gg = idx % G, i = idx / G;
        uint32_t k = 0xffffffffu;
        if (i < N && c0 + gg < C) {
          const float v = x[(int64_t)i * ld + c0 + gg];
          if (v != v) nanflag[gg] = 1;
          k = key_of(v);
        }
        keys[gg * P + i] = k;
      }
    }
    __syncthreads();
    // Bitonic network.  In phase k the direction bit of slot i is i & k, taken inside the column (k & (P - 1) is 0 in the last
    // phase: every column ends ascending).  Steps of distance j >= 16 go through LDS, one barrier each; the steps of distance
    // 8, 4, 2, 1 that end every phase stay inside aligned runs of 16 slots, so a thread takes a run into registers and does all
    // four there (phases 2 .. 16 are one such pass altogether): 66 LDS steps and 12 register passes at P = 32768, not 120 steps.
    const int half = total >> 1;
    if (P >= KS_RUN) {
      ks_run_pass<THREADS>(keys, total, P, 2, tid);
      __syncthreads();
    }
    for (int k = P >= KS_RUN ? 2 * KS_RUN : 2; k <= P; k <<= 1) {
      const int dir = k & (P - 1);
      for (int j = k >> 1; j > 0; j >>= 1) {
        if (j < KS_RUN && P >= KS_RUN) {
          ks_run_pass<THREADS>(keys, total, P, k, tid);
          __syncthreads();
          break;
        }
        for (int p = tid; p < half; p += THREADS) {
          const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), l = i + j;
          const uint32_t a = keys[i], b = keys[l];
          const bool asc = (i & dir) == 0;
          if ((a > b) == asc) {
            keys[i] = b;
            keys[l] = a;
          }
        }
        __syncthreads();
      }
    }
  }
  const double inf = __longlong_as_double(0x7ff0000000000000LL);
  double dp = -inf, dm = -inf;
  if (col < C) {
    const double n = (double)N;
    for (int i = lt; i < N; i += tpc) {
      float v;
      if (sorted) {
        v = col_major ? x[col * ld + i] : x[(int64_t)i * ld + col];
        if (v != v) nanflag[g] = 1;
      } else {
        v = value_of(keys[g * P + i]);
      }
      const double f = 0.5 * erfc(-(double)v / sqrt(2.0));
      dp = fmax(dp, (double)(i + 1) / n - f);
      dm = fmax(dm, f - (double)i / n);
    }
  }
  dp = wave_max_f64(dp);
  dm = wave_max_f64(dm);
  if (lane == 0) {
    red[wave] = dp;
    red[WAVES + wave] = dm;
  }
  __syncthreads();
  if (lt == 0 && col < C) {
    const int w0 = g * (tpc >> 6), w1 = w0 + (tpc >> 6);
    dp = red[w0];
    dm = red[WAVES + w0];
    for (int w = w0 + 1; w < w1; ++w) {
      dp = fmax(dp, red[w]);
      dm = fmax(dm, red[WAVES + w]);
    }
    double d = fmax(dp, dm), p;
    if (nanflag[g]) {
      d = dp = dm = p = qnan();
    } else {
      p = kolmogorov_sf(d * sqrt((double)N));
    }
    stat[col] = d;
    stat[(int64_t)C + col] = dp;
    stat[2 * (int64_t)C + col] = dm;
    p_asym[col] = p;
  }
}

template <int THREADS>
int launch_ks(const float* x, int64_t ld, int col_major, int N, int C, int sorted, int P, double* stat, double* p_asym, hipStream_t stream) {
  constexpr int WAVES = THREADS / 64, SLOTS = 8 * THREADS;
  int G = sorted ? 1 : SLOTS / P;
  G = G < 1 ? 1 : (G > WAVES ? WAVES : G);
  if (G > C) {   // (a power of two still: tpc = THREADS / G stays a multiple of 64)
    G = 1;
    while (2 * G <= C) G *= 2;
  }
  const size_t lds = 2 * WAVES * sizeof(double) + 16 * sizeof(int) + (sorted ? 0 : (size_t)G * P * sizeof(uint32_t));
  if (lds > 64 * 1024) {   // above 64 KiB a kernel's dynamic LDS limit has to be raised, once per device
    static bool raised[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return VUNET_ERR_LAUNCH;
    if (!raised[dev]) {
      const size_t cap = 2 * WAVES * sizeof(double) + 16 * sizeof(int) + (size_t)VUNET_SEQ_KS_MAX_LDS_N * sizeof(uint32_t);
      if (hipFuncSetAttribute(reinterpret_cast<const void*>(&ks_norm_kernel<THREADS>), hipFuncAttributeMaxDynamicSharedMemorySize,
                              (int)cap) != hipSuccess)
        return VUNET_ERR_LAUNCH;
      raised[dev] = true;
    }
  }
  const unsigned blocks = (unsigned)(((int64_t)C + G - 1) / G);
  VUNET_LAUNCH(ks_norm_kernel<THREADS>, dim3(blocks), dim3(THREADS), lds, stream, x, ld, col_major, N, C, sorted, P, G, stat, p_asym);
  return vunet_check_launch();
}

}  // namespace

extern "C" int vunet_seq_latent_nll(const float* z, int64_t ldz, const float* logdet, const float* noise, int32_t B, int32_t C,
                                    double* per_row, double* scalars, void* stream) {
  if (!z || !logdet || !per_row || !scalars || B < 1 || C < 1 || ldz < C) return VUNET_ERR_ARG;
  VUNET_LAUNCH(latent_nll_rows_kernel, dim3((unsigned)(((int64_t)B + 3) / 4)), dim3(256), 0, (hipStream_t)stream, z, ldz, noise, B, C,
               per_row);
  int rc = vunet_check_launch();
  if (rc != VUNET_OK) return rc;
  VUNET_LAUNCH(latent_nll_reduce_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logdet, B, C, per_row, scalars);
  return vunet_check_launch();
}

extern "C" int vunet_seq_ks_norm(const float* x, int64_t ld, int32_t col_major, int32_t N, int32_t C, int32_t sorted, double* stat,
                                 double* p_asym, void* scratch, void* stream) {
  (void)scratch;
  if (!x || !stat || !p_asym || N < 1 || C < 1 || ld < (col_major ? N : C)) return VUNET_ERR_ARG;
  if (!sorted && N > VUNET_SEQ_KS_MAX_LDS_N) return VUNET_ERR_UNSUPPORTED;
  int P = 1;
  if (!sorted)
    while (P < N) P <<= 1;
  if (P <= 4096) return launch_ks<256>(x, ld, col_major ? 1 : 0, N, C, sorted ? 1 : 0, P, stat, p_asym, (hipStream_t)stream);
  return launch_ks<1024>(x, ld, col_major ? 1 : 0, N, C, sorted ? 1 : 0, P, stat, p_asym, (hipStream_t)stream);
}
