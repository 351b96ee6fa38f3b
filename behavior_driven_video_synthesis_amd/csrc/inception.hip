// Inference-only Inception-v3 (models/inception.py): a general forward convolution as an implicit GEMM on the fp32 matrix
// instruction, 3x3 pooling, the global average and the resize-to-299 input kernel.  Interface: include/vunet_inception.h.
//
// convg_kernel<T, KC>.  D[m][p] = sum_k Wp[k][m] X[k][p], k = (c KH + kh) KW + kw ascending, p = (n Ho + ho) Wo + wo.  A
// workgroup of 4 waves owns a T x T tile of D (T = 64: each wave 32 x 32 = 2 x 2 MFMA tiles; T = 32: each wave 16 x 16) and walks
// K in steps of KC rows: the packed weights (zero-padded in k and m: no bounds checks) and the gathered activations (pixel
// tail, K tail and the map's border masked to zero) go through LDS, the next step's global loads are issued before the current
// step's matrix instructions.  <64, 32> is the form for grids that fill the device twice over.  <32, 64> is the form for
// smaller grids (the 8 x 8 and 17 x 17 maps, the 35 x 35 maps at small batch) and for M <= 32: four times the tiles, and 64 rows
// per step because a workgroup with few neighbours on its CU pays a global-load latency per step -- so fewer, longer steps; its
// one 16 x 16 tile per wave alternates between two accumulators (even / odd k groups, added at the end) so that consecutive
// matrix instructions do not wait for each other.
// v_mfma_f32_16x16x4_f32: lane (i = lane % 16, q = lane / 16) supplies A[i][q] = Wp[k + q][m + i] and B[q][i] = X[k + q][p + i],
// and holds D[4 q + v][i].  So 16 lanes store 16 consecutive pixels of one channel.
// The LDS rows are T + 16 floats apart: the two k rows a 32-lane read group touches fall into different halves of the 32 banks.
// Each staging thread keeps (c, kh, kw) of its k rows and advances them by KC with two carries: no division in the loop.
#include "common.h"
#include "../../include/vunet_inception.h"

namespace {

template <int T, int KC>
__global__ __launch_bounds__(256) void convg_kernel(vunet_convg_desc d, const float* __restrict__ x, const float* __restrict__ wp,
                                                    const float* __restrict__ bias, float* __restrict__ y) {
  constexpr int LD = T + 16;          // LDS row pitch
  constexpr int F = T / 32;           // MFMA tiles per wave and dimension
  constexpr int XE = KC * T / 256;    // activation elements a thread stages per step
  constexpr int KS = 256 / T;         // k rows between a thread's elements
  constexpr int NW4 = T / 4;          // float4s per weight row
  constexpr int WE = KC * NW4 / 256;  // weight float4s a thread stages per step
  constexpr int NA = F == 1 ? 2 : 1;  // accumulators per MFMA tile
  __shared__ float ws[KC * LD];
  __shared__ float xs[KC * LD];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
  const int wm = wave & 1, wq = wave >> 1;
  const int p0 = blockIdx.x * T, m0 = blockIdx.y * T;
  const int HoWo = d.Ho * d.Wo, P = d.N * HoWo, KHW = d.KH * d.KW;

  // ---- this thread's pixel of the activation tile
  const int pl = tid % T, kr0 = tid / T;
  const int p = p0 + pl;
  int hi0 = -(1 << 28), wi0 = 0;     // a pixel past the tail fails every bounds check
  const float* xb = x;
  if (p < P) {
    const int n = p / HoWo, r = p - n * HoWo, ho = r / d.Wo, wo = r - ho * d.Wo;
    hi0 = ho * d.stride_h - d.pad_h;
    wi0 = wo * d.stride_w - d.pad_w;
    xb = x + ((size_t)n * d.x_ctot + d.x_coff) * ((size_t)d.H * d.W);
  }
  // (c, kh, kw) of this thread's k rows kr0 + KS j: one decode, then mixed-radix additions (the carries of step())
  struct Step { int c, h, w; };
  auto decode = [&](int k) {
    Step r;
    r.c = k / KHW;
    const int t = k - r.c * KHW;
    r.h = t / d.KW;
    r.w = t - r.h * d.KW;
    return r;
  };
  auto step = [&](int& c, int& h, int& w, const Step& by) {
    w += by.w;
    if (w >= d.KW) { w -= d.KW; ++h; }
    h += by.h;
    if (h >= d.KH) { h -= d.KH; ++c; }
    c += by.c;
  };
  const Step first = decode(kr0), by_ks = decode(KS), by_kc = decode(KC);
  int kc[XE], kh[XE], kw[XE];
  kc[0] = first.c, kh[0] = first.h, kw[0] = first.w;
#pragma unroll
  for (int j = 1; j < XE; ++j) {
    kc[j] = kc[j - 1], kh[j] = kh[j - 1], kw[j] = kw[j - 1];
    step(kc[j], kh[j], kw[j], by_ks);
  }

  const int wrow = tid / NW4, wc4 = tid - wrow * NW4;     // + 256 / NW4 rows per further element
  const float* wsrc = wp + (size_t)wrow * d.Mpad + m0 + 4 * wc4;

  float xv[XE];
  f32x4 wv[WE];
  auto fetch = [&](int chunk) {
#pragma unroll
    for (int e = 0; e < WE; ++e)
      wv[e] = *reinterpret_cast<const f32x4*>(wsrc + ((size_t)chunk * KC + e * (256 / NW4)) * d.Mpad);
#pragma unroll
    for (int j = 0; j < XE; ++j) {
      const int hi = hi0 + kh[j], wi = wi0 + kw[j];
      const bool ok = kc[j] < d.C && (unsigned)hi < (unsigned)d.H && (unsigned)wi < (unsigned)d.W;
      const float v = xb[ok ? ((size_t)kc[j] * d.H + hi) * d.W + wi : 0];   // element 0 of the slice is always there: no branch
      xv[j] = ok ? v : 0.f;
      step(kc[j], kh[j], kw[j], by_kc);
    }
  };

  f32x4 acc[NA][F][F];
#pragma unroll
  for (int a = 0; a < NA; ++a)
#pragma unroll
    for (int i = 0; i < F; ++i)
#pragma unroll
      for (int j = 0; j < F; ++j) acc[a][i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nchunks = (d.C * KHW + KC - 1) / KC;    // <= Kpad / KC: Kpad is a multiple of 64
  fetch(0);
  for (int ch = 0; ch < nchunks; ++ch) {
#pragma unroll
    for (int e = 0; e < WE; ++e) *reinterpret_cast<f32x4*>(&ws[(wrow + e * (256 / NW4)) * LD + 4 * wc4]) = wv[e];
#pragma unroll
    for (int j = 0; j < XE; ++j) xs[(kr0 + KS * j) * LD + pl] = xv[j];
    __syncthreads();
    if (ch + 1 < nchunks) fetch(ch + 1);
#pragma unroll
    for (int s = 0; s < KC / 4; s += NA)
#pragma unroll
      for (int u = 0; u < NA; ++u) {
        const int kk = 4 * (s + u) + lk;
        float a[F], b[F];
#pragma unroll
        for (int i = 0; i < F; ++i) a[i] = ws[kk * LD + wm * 16 * F + 16 * i + li];
#pragma unroll
        for (int j = 0; j < F; ++j) b[j] = xs[kk * LD + wq * 16 * F + 16 * j + li];
#pragma unroll
        for (int i = 0; i < F; ++i)
#pragma unroll
          for (int j = 0; j < F; ++j) acc[u][i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[u][i][j], 0, 0, 0);
      }
    __syncthreads();
  }

  // ---- epilogue: bias, ReLU, the channel slice of y
#pragma unroll
  for (int j = 0; j < F; ++j) {
    const int po = p0 + wq * 16 * F + 16 * j + li;
    if (po >= P) continue;
    const int n = po / HoWo, r = po - n * HoWo;
    float* yb = y + ((size_t)n * d.y_ctot + d.y_coff) * (size_t)HoWo + r;
#pragma unroll
    for (int i = 0; i < F; ++i)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int m = m0 + wm * 16 * F + 16 * i + 4 * lk + v;
        if (m >= d.M) continue;
        float o = (NA == 2 ? acc[0][i][j][v] + acc[NA - 1][i][j][v] : acc[0][i][j][v]) + (bias ? bias[m] : 0.f);
        if (d.relu) o = fmaxf(o, 0.f);
        yb[(size_t)m * HoWo] = o;
      }
  }
}

__global__ __launch_bounds__(256) void pool2d_kernel(vunet_pool2d_desc d, const float* __restrict__ x, float* __restrict__ y) {
  const int64_t total = (int64_t)d.N * d.C * d.Ho * d.Wo, e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int wo = (int)(e % d.Wo);
  int64_t t = e / d.Wo;
  const int ho = (int)(t % d.Ho);
  t /= d.Ho;
  const int c = (int)(t % d.C), n = (int)(t / d.C);
  const float* xp = x + ((size_t)n * d.x_ctot + d.x_coff + c) * ((size_t)d.H * d.W);
  const int h0 = ho * d.stride - d.pad, w0 = wo * d.stride - d.pad;
  float acc = d.mode == 0 ? -INFINITY : 0.f;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const int hi = h0 + i, wi = w0 + j;
      if ((unsigned)hi < (unsigned)d.H && (unsigned)wi < (unsigned)d.W) {
        const float v = xp[(size_t)hi * d.W + wi];
        acc = d.mode == 0 ? fmaxf(acc, v) : acc + v;
      }
    }
  if (d.mode == 1) acc = acc / 9.f;
  y[(((size_t)n * d.y_ctot + d.y_coff + c) * d.Ho + ho) * d.Wo + wo] = acc;
}

__global__ __launch_bounds__(256) void global_avgpool_kernel(const float* __restrict__ x, float* __restrict__ y, int64_t NC, int HW) {
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= NC) return;
  const int lane = threadIdx.x & 63;
  const float* xr = x + row * HW;
  float s = 0.f;
  for (int i = lane; i < HW; i += 64) s += xr[i];
  s = wave_sum(s);
  if (lane == 0) y[row] = s / (float)HW;
}

__global__ __launch_bounds__(256) void inception_input_kernel(const float* __restrict__ x, float* __restrict__ y, int N, int H, int W,
                                                              int mode) {
  constexpr int S = VUNET_INCEPTION_SIZE;
  const int64_t total = (int64_t)N * 3 * S * S, e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int ox = (int)(e % S);
  int64_t t = e / S;
  const int oy = (int)(t % S);
  t /= S;
  const int c = (int)(t % 3);
  const double sy = fmax((oy + 0.5) * ((double)H / S) - 0.5, 0.0), sx = fmax((ox + 0.5) * ((double)W / S) - 0.5, 0.0);
  const int y0 = min((int)sy, H - 1), x0 = min((int)sx, W - 1);
  const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
  const double ly = sy - y0, lx = sx - x0;
  const float* xp = x + (size_t)t * H * W;    // t = n * 3 + c
  const double v00 = xp[(size_t)y0 * W + x0], v01 = xp[(size_t)y0 * W + x1], v10 = xp[(size_t)y1 * W + x0], v11 = xp[(size_t)y1 * W + x1];
  double v = (1.0 - ly) * ((1.0 - lx) * v00 + lx * v01) + ly * ((1.0 - lx) * v10 + lx * v11);
  const double mean = c == 0 ? 0.485 : (c == 1 ? 0.456 : 0.406), sd = c == 0 ? 0.229 : (c == 1 ? 0.224 : 0.225);
  if (mode == 1) v = v * (sd / 0.5) + (mean - 0.5) / 0.5;
  else if (mode == 2) v = (fmin(fmax((v + 1.0) / 2.0, 0.0), 1.0) - mean) / sd;
  y[e] = (float)v;
}

constexpr int64_t LIM = (int64_t)1 << 31;

int convg_tile_of(const vunet_convg_desc& d) {
  if (d.tile == 64 || d.tile == 32) return d.tile;
  if (d.tile != 0) return 0;
  const int64_t P = (int64_t)d.N * d.Ho * d.Wo;
  return (d.M > 32 && ((P + 63) / 64) * ((d.M + 63) / 64) >= VUNET_CONVG_FILL) ? 64 : 32;
}

bool convg_ok(const vunet_convg_desc* d) {
  if (!d) return false;
  if (d->N < 1 || d->C < 1 || d->H < 1 || d->W < 1 || d->M < 1 || d->Ho < 1 || d->Wo < 1 || d->KH < 1 || d->KW < 1 || d->stride_h < 1 ||
      d->stride_w < 1 || d->pad_h < 0 || d->pad_w < 0)
    return false;
  if (d->H + 2 * d->pad_h < d->KH || d->W + 2 * d->pad_w < d->KW) return false;
  if (d->Ho != (d->H + 2 * d->pad_h - d->KH) / d->stride_h + 1 || d->Wo != (d->W + 2 * d->pad_w - d->KW) / d->stride_w + 1) return false;
  if (d->x_coff < 0 || d->y_coff < 0 || (int64_t)d->x_coff + d->C > d->x_ctot || (int64_t)d->y_coff + d->M > d->y_ctot) return false;
  const int64_t K = (int64_t)d->C * d->KH * d->KW;
  if (d->Kpad < K || d->Kpad % VUNET_CONVG_KC || d->Mpad < d->M || d->Mpad % VUNET_CONVG_MT) return false;
  if ((int64_t)d->N * d->x_ctot * d->H * d->W >= LIM || (int64_t)d->N * d->y_ctot * d->Ho * d->Wo >= LIM ||
      (int64_t)d->Kpad * d->Mpad >= LIM)
    return false;
  return convg_tile_of(*d) != 0;
}

}  // namespace

extern "C" int vunet_convg_tile(const vunet_convg_desc* d) { return convg_ok(d) ? convg_tile_of(*d) : VUNET_ERR_ARG; }

extern "C" int vunet_convg(const vunet_convg_desc* d, const float* x, const float* w, const float* bias, float* y, void* stream) {
  if (!convg_ok(d) || !x || !w || !y) return VUNET_ERR_ARG;
  const int T = convg_tile_of(*d);
  const int64_t P = (int64_t)d->N * d->Ho * d->Wo;
  const dim3 grid((unsigned)((P + T - 1) / T), (unsigned)((d->M + T - 1) / T));
  if (grid.y > 65535u) return VUNET_ERR_ARG;
  if (T == 64) VUNET_LAUNCH((convg_kernel<64, 32>), grid, dim3(256), 0, (hipStream_t)stream, *d, x, w, bias, y);
  else VUNET_LAUNCH((convg_kernel<32, 64>), grid, dim3(256), 0, (hipStream_t)stream, *d, x, w, bias, y);
  return vunet_check_launch();
}

extern "C" int vunet_pool2d(const vunet_pool2d_desc* d, const float* x, float* y, void* stream) {
  if (!d || !x || !y) return VUNET_ERR_ARG;
  if (d->N < 1 || d->C < 1 || d->H < 1 || d->W < 1 || (d->stride != 1 && d->stride != 2) || (d->pad != 0 && d->pad != 1) ||
      (d->mode != 0 && d->mode != 1) || d->H + 2 * d->pad < 3 || d->W + 2 * d->pad < 3)
    return VUNET_ERR_ARG;
  if (d->Ho != (d->H + 2 * d->pad - 3) / d->stride + 1 || d->Wo != (d->W + 2 * d->pad - 3) / d->stride + 1) return VUNET_ERR_ARG;
  if (d->x_coff < 0 || d->y_coff < 0 || (int64_t)d->x_coff + d->C > d->x_ctot || (int64_t)d->y_coff + d->C > d->y_ctot) return VUNET_ERR_ARG;
  if ((int64_t)d->N * d->x_ctot * d->H * d->W >= LIM || (int64_t)d->N * d->y_ctot * d->Ho * d->Wo >= LIM) return VUNET_ERR_ARG;
  const int64_t total = (int64_t)d->N * d->C * d->Ho * d->Wo;
  VUNET_LAUNCH(pool2d_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, *d, x, y);
  return vunet_check_launch();
}

extern "C" int vunet_global_avgpool(const float* x, float* y, int64_t NC, int32_t HW, void* stream) {
  if (!x || !y || NC < 1 || HW < 1 || NC * HW >= LIM) return VUNET_ERR_ARG;
  VUNET_LAUNCH(global_avgpool_kernel, dim3((unsigned)((NC + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, y, NC, (int)HW);
  return vunet_check_launch();
}

extern "C" int vunet_inception_input(const float* x, float* y, int32_t N, int32_t H, int32_t W, int32_t mode, void* stream) {
  if (!x || !y || N < 1 || H < 1 || W < 1 || mode < 0 || mode > 2) return VUNET_ERR_ARG;
  if ((int64_t)N * 3 * H * W >= LIM || (int64_t)N * 3 * VUNET_INCEPTION_SIZE * VUNET_INCEPTION_SIZE >= LIM) return VUNET_ERR_ARG;
  const int64_t total = (int64_t)N * 3 * VUNET_INCEPTION_SIZE * VUNET_INCEPTION_SIZE;
  VUNET_LAUNCH(inception_input_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, (int)N, (int)H,
               (int)W, (int)mode);
  return vunet_check_launch();
}
