// Spherical interpolation between behaviour codes (lib/utils.py:920-925 as lib/logging.py:994-1012 calls it): every step of
// both directions of every pair in one launch, instead of one device -> host -> device round trip per step and direction.
//
// One 256-thread workgroup per pair.  The three sums (|a|^2, |b|^2, a.b), the angle and the two coefficients of a step are
// float64; an output element is rounded once, at its store.  The sums are reduced by butterfly shuffles inside a wave and in
// wave order across the four waves: no atomics, the same bits on every run.
#include "common.h"

#define SLERP_THREADS 256
#define SLERP_MAX_STEPS 64

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// VEC_OUT: h % 4 == 0 and a 16-byte aligned `out`, so every output row starts on 16 bytes; VEC_IN: the same for the two inputs
// and their row pitch.
template <bool VEC_OUT, bool VEC_IN>
__global__ __launch_bounds__(SLERP_THREADS) void seq_slerp_kernel(const float* __restrict__ b1, const float* __restrict__ b2,
                                                                  int64_t ld_in, int pairs, int h, const double* __restrict__ steps,
                                                                  int n_steps, float* __restrict__ out) {
  __shared__ double red[3][SLERP_THREADS / 64];
  __shared__ double coef[SLERP_MAX_STEPS][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t p = blockIdx.x;
  const float* a = b1 + p * ld_in;
  const float* b = b2 + p * ld_in;

  double saa = 0.0, sbb = 0.0, sab = 0.0;
  for (int i = tid; i < h; i += SLERP_THREADS) {
    const double x = (double)a[i], y = (double)b[i];
    saa += x * x;
    sbb += y * y;
    sab += x * y;
  }
  saa = wave_sum_f64(saa);
  sbb = wave_sum_f64(sbb);
  sab = wave_sum_f64(sab);
  if (lane == 0) {
    red[0][wave] = saa;
    red[1][wave] = sbb;
    red[2][wave] = sab;
  }
  __syncthreads();
  if (tid < n_steps) {
    const double aa = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
    const double bb = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    const double ab = ((red[2][0] + red[2][1]) + red[2][2]) + red[2][3];
    // a zero row: 0 / 0 = NaN, which the comparisons below pass on (numpy's clip does too) -> NaN coefficients, NaN rows
    double c = ab / (sqrt(aa) * sqrt(bb));
    c = c < -1.0 ? -1.0 : (c > 1.0 ? 1.0 : c);
    const double omega = acos(c), so = sin(omega), v = steps[tid];
    // a.b is symmetric bit for bit, so slerp(v, b2, b1) has the coefficients of slerp(v, b1, b2): (lo, hi) serves both directions
    double lo, hi;
    if (so == 0.0) {
      lo = 1.0 - v;
      hi = v;
    } else {
      lo = sin((1.0 - v) * omega) / so;
      hi = sin(v * omega) / so;
    }
    coef[tid][0] = lo;
    coef[tid][1] = hi;
  }
  __syncthreads();

  const int64_t row = h, dir = (int64_t)pairs * n_steps * row;
  float* o0 = out + p * n_steps * row;   // out[0][p]: from b1 to b2
  float* o1 = o0 + dir;                  // out[1][p]: from b2 to b1
  if constexpr (VEC_OUT) {
    for (int i = 4 * tid; i < h; i += 4 * SLERP_THREADS) {
      float4 xa, xb;
      if constexpr (VEC_IN) {
        xa = *reinterpret_cast<const float4*>(a + i);
        xb = *reinterpret_cast<const float4*>(b + i);
      } else {
        xa = make_float4(a[i], a[i + 1], a[i + 2], a[i + 3]);
        xb = make_float4(b[i], b[i + 1], b[i + 2], b[i + 3]);
      }
      const double ax = xa.x, ay = xa.y, az = xa.z, aw = xa.w, bx = xb.x, by = xb.y, bz = xb.z, bw = xb.w;
      for (int s = 0; s < n_steps; ++s) {
        const double lo = coef[s][0], hi = coef[s][1];
        *reinterpret_cast<float4*>(o0 + s * row + i) =
            make_float4((float)(lo * ax + hi * bx), (float)(lo * ay + hi * by), (float)(lo * az + hi * bz), (float)(lo * aw + hi * bw));
        *reinterpret_cast<float4*>(o1 + s * row + i) =
            make_float4((float)(lo * bx + hi * ax), (float)(lo * by + hi * ay), (float)(lo * bz + hi * az), (float)(lo * bw + hi * aw));
      }
    }
  } else {
    for (int i = tid; i < h; i += SLERP_THREADS) {
      const double x = (double)a[i], y = (double)b[i];
      for (int s = 0; s < n_steps; ++s) {
        const double lo = coef[s][0], hi = coef[s][1];
        o0[s * row + i] = (float)(lo * x + hi * y);
        o1[s * row + i] = (float)(lo * y + hi * x);
      }
    }
  }
}

extern "C" int vunet_seq_slerp(const float* b1, const float* b2, int64_t ld_in, int pairs, int h, const double* steps, int n_steps,
                               float* out, void* stream) {
  if (!b1 || !b2 || !steps || !out || pairs < 1 || h < 1 || ld_in < h || n_steps < 1 || n_steps > SLERP_MAX_STEPS) return VUNET_ERR_ARG;
  const dim3 grid((unsigned)pairs), block(SLERP_THREADS);
  const bool vec_out = h % 4 == 0 && (uintptr_t)out % 16 == 0;
  const bool vec_in = vec_out && ld_in % 4 == 0 && (uintptr_t)b1 % 16 == 0 && (uintptr_t)b2 % 16 == 0;
  if (vec_in)
    VUNET_LAUNCH((seq_slerp_kernel<true, true>), grid, block, 0, (hipStream_t)stream, b1, b2, ld_in, pairs, h, steps, n_steps, out);
  else if (vec_out)
    VUNET_LAUNCH((seq_slerp_kernel<true, false>), grid, block, 0, (hipStream_t)stream, b1, b2, ld_in, pairs, h, steps, n_steps, out);
  else
    VUNET_LAUNCH((seq_slerp_kernel<false, false>), grid, block, 0, (hipStream_t)stream, b1, b2, ld_in, pairs, h, steps, n_steps, out);
  return vunet_check_launch();
}
