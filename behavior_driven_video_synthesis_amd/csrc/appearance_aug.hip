// The random appearance augmentation: uint8 RGB frames and one output-to-input affine per image -> Pillow's
// Image.transform(AFFINE, BILINEAR, fillcolor) of each (virtually reflect-padded) frame, cut to an output window, as bytes or as the
// fp32 [-1, 1] images the trainers take.  Interface and the rule restated from Pillow: include/vunet_appearance_aug.h.
//
// The reference does this on the host per image (torchvision's RandomAffine, and Pad -> RandomRotation -> CenterCrop;
// data/deepfashion.py:92-108, data/market.py:52-64).  Here, one launch: one thread per output pixel, lanes along output x, one
// block row per output row.  The matrix row is uniform over an image; the four taps of neighbouring lanes are neighbouring source
// pixels (a gather of a few megabytes served by L1 / L2); stores along x are coalesced.  Pillow's bilinear transform is plain double
// arithmetic with a truncating store: float64 without fused multiply-adds, in its order of operations, gives its bytes.  The fp32
// output is (float)v / 255.0f * 2.0f - 1.0f with every operation rounded once.  No LDS, no atomics.
#include <math.h>

#include "common.h"
#include "../../include/vunet_appearance_aug.h"

namespace {

// NumPy's mode="reflect" of any index (dcb|abcd|cba): the triangle wave of period 2 (n - 1); n == 1 maps everything to 0
__device__ __forceinline__ int refl(int i, int n) {
  if (i >= 0 && i < n) return i;
  if (n == 1) return 0;
  const int period = 2 * (n - 1);
  int m = i % period;
  if (m < 0) m += period;
  return m >= n ? period - m : m;
}

__device__ __forceinline__ int clampi(int v, int hi) { return min(max(v, 0), hi); }

__global__ __launch_bounds__(256) void appearance_affine_kernel(const uint8_t* __restrict__ frames, const int32_t* __restrict__ hw,
                                                                const double* __restrict__ mats, int Hmax, int Wmax, int pad, int ox,
                                                                int oy, int oh, int ow, int fr, int fg, int fb,
                                                                float* __restrict__ out_f32, uint8_t* __restrict__ out_u8,
                                                                int32_t* __restrict__ status) {
#pragma clang fp contract(off)
  const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y, n = blockIdx.z;
  const int h = hw[(size_t)n * 2], w = hw[(size_t)n * 2 + 1];
  const double* M = mats + (size_t)n * 6;
  const double m0 = M[0], m1 = M[1], m2 = M[2], m3 = M[3], m4 = M[4], m5 = M[5];
  const bool ok = h >= 1 && h <= Hmax && w >= 1 && w <= Wmax && isfinite(m0) && isfinite(m1) && isfinite(m2) && isfinite(m3) &&
                  isfinite(m4) && isfinite(m5);
  if (x == 0 && y == 0) status[n] = ok ? 0 : 1;
  if (x >= ow) return;
  int v[3] = {fr, fg, fb};
  if (ok) {
    const int H = h + 2 * pad, W = w + 2 * pad;
    const double xin = (double)(x + ox) + 0.5, yin = (double)(y + oy) + 0.5;
    double xs = (m0 * xin + m1 * yin) + m2;
    double ys = (m3 * xin + m4 * yin) + m5;
    if (xs >= 0.0 && xs < (double)W && ys >= 0.0 && ys < (double)H) {   // (a NaN from inf - inf passes neither comparison)
      xs = xs - 0.5;
      ys = ys - 0.5;
      const int x0 = (int)floor(xs), y0 = (int)floor(ys);
      const double dx = xs - (double)x0, dy = ys - (double)y0;
      const uint8_t* img = frames + (size_t)n * Hmax * Wmax * 3;
      const uint8_t* up = img + (size_t)refl(clampi(y0, H - 1) - pad, h) * Wmax * 3;
      const uint8_t* lo = img + (size_t)refl(clampi(y0 + 1, H - 1) - pad, h) * Wmax * 3;
      const int ca = refl(clampi(x0, W - 1) - pad, w) * 3, cb = refl(clampi(x0 + 1, W - 1) - pad, w) * 3;
      for (int c = 0; c < 3; ++c) {
        const double a = (double)up[ca + c], b = (double)up[cb + c];
        const double v1 = a + (b - a) * dx;
        const double a2 = (double)lo[ca + c], b2 = (double)lo[cb + c];
        const double v2 = a2 + (b2 - a2) * dx;
        v[c] = (int)(v1 + (v2 - v1) * dy);
      }
    }
  }
  if (out_u8) {
    uint8_t* o = out_u8 + (((size_t)n * oh + y) * ow + x) * 3;
    for (int c = 0; c < 3; ++c) o[c] = (uint8_t)v[c];
  } else {
    const size_t plane = (size_t)oh * ow;
    float* o = out_f32 + (size_t)n * 3 * plane + (size_t)y * ow + x;
    for (int c = 0; c < 3; ++c) o[c * plane] = (float)v[c] / 255.0f * 2.0f - 1.0f;
  }
}

bool side_ok(int v) { return v >= 1 && v <= 65535; }
bool byte_ok(int v) { return v >= 0 && v <= 255; }

}  // namespace

extern "C" int vunet_appearance_affine(const uint8_t* frames, const int32_t* hw, const double* mats, int32_t N, int32_t Hmax,
                                       int32_t Wmax, int32_t pad, int32_t ox, int32_t oy, int32_t oh, int32_t ow, int32_t fill_r,
                                       int32_t fill_g, int32_t fill_b, float* out_f32, uint8_t* out_u8, int32_t* status,
                                       void* stream) {
  if (!frames || !hw || !mats || !status || (out_f32 == nullptr) == (out_u8 == nullptr) || !side_ok(N) || !side_ok(Hmax) ||
      !side_ok(Wmax) || !side_ok(oh) || !side_ok(ow) || pad < 0 || pad > (1 << 20) || ox < -(1 << 24) || ox > (1 << 24) ||
      oy < -(1 << 24) || oy > (1 << 24) || !byte_ok(fill_r) || !byte_ok(fill_g) || !byte_ok(fill_b))
    return VUNET_ERR_ARG;
  const unsigned lanes = ow >= 256 ? 256u : (unsigned)((ow + 63) / 64 * 64);
  VUNET_LAUNCH(appearance_affine_kernel, dim3((unsigned)((ow + (int)lanes - 1) / (int)lanes), (unsigned)oh, (unsigned)N), dim3(lanes),
               0, (hipStream_t)stream, frames, hw, mats, (int)Hmax, (int)Wmax, (int)pad, (int)ox, (int)oy, (int)oh, (int)ow,
               (int)fill_r, (int)fill_g, (int)fill_b, out_f32, out_u8, status);
  return vunet_check_launch();
}
