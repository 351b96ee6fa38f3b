// The raw-frame input route: decoded uint8 RGB frames -> crop window with the border reflected -> Pillow's 8-bit bicubic resize ->
// the fp32 [-1, 1] images the trainers take.  Interface and the rules restated from Pillow and the reference:
// include/vunet_image_input.h.
//
// The reference does this on the host per image (cv2.copyMakeBorder, PIL Image.resize, ToTensor; data/base_dataset.py:281-315,
// data/__init__.py:15-43).  Here, three launches:
//   * image_tables_kernel: one thread per (axis, image, output index) builds that index's bounds and fixed-point taps.  float64
//     without fused multiply-adds, in Pillow's order of operations (a reordered sum or a contraction moves a tap by one unit); the
//     taps are evaluated twice (for their sum, then normalised) so that no thread keeps a runtime-indexed array.
//   * image_hpass_kernel: one block per window row, lanes along output x.  A lane's taps are a few consecutive source pixels and its
//     neighbours' overlap them: the row segment (3 KB for a 1000-pixel frame) is served by L1.  Source indices are reflected
//     per tap, with a branch that only the lanes outside the frame take.
//   * image_vpass_kernel: one block per output row, lanes along output x: the intermediate is read coalesced (three consecutive
//     bytes per lane), bounds and taps are the same for the whole block.
// Integer sums are exact, so nothing but the tables depends on floating point; the fp32 output is (float)v / 255.0f * 2.0f - 1.0f
// with every operation rounded once.  No LDS, no atomics.
#include <math.h>

#include "common.h"
#include "../../include/vunet_image_input.h"

namespace {

constexpr int PB = VUNET_IMAGE_INPUT_PRECISION_BITS;

struct Geom {
  int h, w, x0, y0, cw, ch;
  bool ok;
};

__device__ __forceinline__ Geom load_geom(const int32_t* __restrict__ geom, int n, int Hmax, int Wmax) {
  const int32_t* g = geom + (size_t)n * 6;
  Geom r;
  r.h = g[0], r.w = g[1], r.x0 = g[2], r.y0 = g[3], r.cw = g[4], r.ch = g[5];
  r.ok = r.h >= 1 && r.h <= Hmax && r.w >= 1 && r.w <= Wmax && r.cw >= 1 && r.cw <= Wmax && r.ch >= 1 && r.ch <= Hmax;
  return r;
}

// cv2.BORDER_REFLECT of any 64-bit index: inside [0, len) as it is, else the triangle wave of period 2 len
__device__ __forceinline__ int reflect(int64_t p, int len) {
  if (p >= 0 && p < len) return (int)p;
  const int64_t period = 2 * (int64_t)len;
  int64_t m = p % period;
  if (m < 0) m += period;
  return (int)(m >= len ? period - 1 - m : m);
}

__device__ __forceinline__ double bicubic(double t) {
#pragma clang fp contract(off)
  const double a = -0.5;
  t = fabs(t);
  if (t < 1.0) return ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0;
  if (t < 2.0) return (((t - 5.0) * t + 8.0) * t - 4.0) * a;
  return 0.0;
}

__device__ __forceinline__ int clip8(int acc) { return min(max(acc >> PB, 0), 255); }

__global__ __launch_bounds__(64) void image_tables_kernel(const int32_t* __restrict__ geom, int N, int Hmax, int Wmax, int S, int kmax,
                                                          int32_t* __restrict__ coef, int32_t* __restrict__ bounds,
                                                          int32_t* __restrict__ status) {
#pragma clang fp contract(off)
  const int xx = blockIdx.x * 64 + threadIdx.x, n = blockIdx.y, axis = blockIdx.z;
  if (xx >= S) return;
  const Geom g = load_geom(geom, n, Hmax, Wmax);
  if (axis == 0 && xx == 0) status[n] = g.ok ? 0 : 1;
  const size_t slot = ((size_t)axis * N + n) * S + xx;
  int32_t* k = coef + slot * kmax;
  int32_t* b = bounds + slot * 2;
  const int in = axis == 0 ? g.cw : g.ch;
  int xmin = 0, xmax = 0;
  if (g.ok && in == S) {   // the axis Pillow skips: the identity tap
    xmin = xx;
    xmax = 1;
    k[0] = 1 << PB;
  } else if (g.ok) {
    const double scale = (double)(float)in / (double)S;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * filterscale;
    const double ss = 1.0 / filterscale;
    const double center = ((double)xx + 0.5) * scale;
    xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    xmax = (int)(center + support + 0.5);
    if (xmax > in) xmax = in;
    xmax -= xmin;
    xmax = min(max(xmax, 0), kmax);   // (kmax >= ksize >= xmax for every in the contract admits: this never cuts a tap)
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww = ww + bicubic(((double)(x + xmin) - center + 0.5) * ss);
    for (int x = 0; x < xmax; ++x) {
      double w = bicubic(((double)(x + xmin) - center + 0.5) * ss);
      if (ww != 0.0) w = w / ww;
      k[x] = w < 0.0 ? (int)(-0.5 + w * (double)(1 << PB)) : (int)(0.5 + w * (double)(1 << PB));
    }
  }
  for (int x = xmax; x < kmax; ++x) k[x] = 0;
  b[0] = xmin;
  b[1] = xmax;
}

__global__ __launch_bounds__(256) void image_hpass_kernel(const uint8_t* __restrict__ frames, const int32_t* __restrict__ geom,
                                                          int N, int Hmax, int Wmax, int S, int kmax, const int32_t* __restrict__ coef,
                                                          const int32_t* __restrict__ bounds, const int32_t* __restrict__ status,
                                                          uint8_t* __restrict__ inter) {
  const int xx = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y, n = blockIdx.z;
  if (status[n] != 0) return;
  const Geom g = load_geom(geom, n, Hmax, Wmax);
  if (!g.ok || i >= g.ch || xx >= S) return;
  const int sy = reflect((int64_t)g.y0 + i, g.h);
  const uint8_t* row = frames + ((size_t)n * Hmax + sy) * Wmax * 3;
  const size_t slot = (size_t)n * S + xx;   // axis 0
  const int32_t* k = coef + slot * kmax;
  const int xmin = bounds[slot * 2], xmax = min(bounds[slot * 2 + 1], kmax);
  int r = 1 << (PB - 1), gr = r, bl = r;
  const int64_t first = (int64_t)g.x0 + xmin;
  for (int t = 0; t < xmax; ++t) {
    const uint8_t* p = row + (size_t)reflect(first + t, g.w) * 3;
    const int kk = k[t];
    r += (int)p[0] * kk;
    gr += (int)p[1] * kk;
    bl += (int)p[2] * kk;
  }
  uint8_t* o = inter + (((size_t)n * Hmax + i) * S + xx) * 3;
  o[0] = (uint8_t)clip8(r);
  o[1] = (uint8_t)clip8(gr);
  o[2] = (uint8_t)clip8(bl);
}

__global__ __launch_bounds__(256) void image_vpass_kernel(const uint8_t* __restrict__ inter, int N, int Hmax, int S, int kmax,
                                                          const int32_t* __restrict__ coef, const int32_t* __restrict__ bounds,
                                                          const int32_t* __restrict__ status, const int32_t* __restrict__ geom,
                                                          float* __restrict__ out_f32, uint8_t* __restrict__ out_u8) {
#pragma clang fp contract(off)
  const int xx = blockIdx.x * blockDim.x + threadIdx.x, yy = blockIdx.y, n = blockIdx.z;
  if (xx >= S) return;
  int v[3] = {0, 0, 0};
  const bool ok = status[n] == 0;
  if (ok) {
    const size_t slot = ((size_t)N + n) * S + yy;   // axis 1
    const int32_t* k = coef + slot * kmax;
    const int ch = geom[(size_t)n * 6 + 5];         // (status 0: 1 <= ch <= Hmax)
    const int ymin = max(bounds[slot * 2], 0), ymax = min(min(bounds[slot * 2 + 1], kmax), ch - ymin);   // rows < ch only
    int r = 1 << (PB - 1), gr = r, bl = r;
    for (int t = 0; t < ymax; ++t) {
      const uint8_t* p = inter + (((size_t)n * Hmax + ymin + t) * S + xx) * 3;
      const int kk = k[t];
      r += (int)p[0] * kk;
      gr += (int)p[1] * kk;
      bl += (int)p[2] * kk;
    }
    v[0] = clip8(r), v[1] = clip8(gr), v[2] = clip8(bl);
  }
  if (out_u8) {
    uint8_t* o = out_u8 + (((size_t)n * S + yy) * S + xx) * 3;
    for (int c = 0; c < 3; ++c) o[c] = (uint8_t)v[c];
  } else {
    const size_t plane = (size_t)S * S;
    float* o = out_f32 + (size_t)n * 3 * plane + (size_t)yy * S + xx;
    for (int c = 0; c < 3; ++c) o[c * plane] = ok ? (float)v[c] / 255.0f * 2.0f - 1.0f : -1.0f;
  }
}

bool sizes_ok(int N, int Hmax, int Wmax, int S, int kmax) {
  if (N < 1 || N > 65535 || Hmax < 1 || Hmax > 65535 || Wmax < 1 || Wmax > 65535 || S < 1 || S > 65535) return false;
  const double scale = (double)(float)(Hmax > Wmax ? Hmax : Wmax) / (double)S;
  return kmax == (int)ceil(2.0 * (scale < 1.0 ? 1.0 : scale)) * 2 + 1;
}

unsigned lanes_of(int S) { return S >= 256 ? 256u : (unsigned)((S + 63) / 64 * 64); }

}  // namespace

extern "C" int vunet_image_input_tables(const int32_t* geom, int32_t N, int32_t Hmax, int32_t Wmax, int32_t S, int32_t kmax,
                                        int32_t* coef, int32_t* bounds, int32_t* status, void* stream) {
  if (!geom || !coef || !bounds || !status || !sizes_ok(N, Hmax, Wmax, S, kmax)) return VUNET_ERR_ARG;
  VUNET_LAUNCH(image_tables_kernel, dim3((unsigned)((S + 63) / 64), (unsigned)N, 2), dim3(64), 0, (hipStream_t)stream, geom, N, Hmax,
               Wmax, S, kmax, coef, bounds, status);
  return vunet_check_launch();
}

extern "C" int vunet_image_input_resample(const uint8_t* frames, const int32_t* geom, int32_t N, int32_t Hmax, int32_t Wmax, int32_t S,
                                          int32_t kmax, const int32_t* coef, const int32_t* bounds, const int32_t* status,
                                          uint8_t* inter, float* out_f32, uint8_t* out_u8, void* stream) {
  if (!frames || !geom || !coef || !bounds || !status || !inter || (out_f32 == nullptr) == (out_u8 == nullptr) ||
      !sizes_ok(N, Hmax, Wmax, S, kmax))
    return VUNET_ERR_ARG;
  const unsigned lanes = lanes_of(S), bx = (unsigned)((S + (int)lanes - 1) / (int)lanes);
  VUNET_LAUNCH(image_hpass_kernel, dim3(bx, (unsigned)Hmax, (unsigned)N), dim3(lanes), 0, (hipStream_t)stream, frames, geom, N, Hmax,
               Wmax, S, kmax, coef, bounds, status, inter);
  int rc = vunet_check_launch();
  if (rc != VUNET_OK) return rc;
  VUNET_LAUNCH(image_vpass_kernel, dim3(bx, (unsigned)S, (unsigned)N), dim3(lanes), 0, (hipStream_t)stream, inter, N, Hmax, S, kmax,
               coef, bounds, status, geom, out_f32, out_u8);
  return vunet_check_launch();
}
