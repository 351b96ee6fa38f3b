// The person-box crop of run_inference: the bounding rectangle of an image's valid keypoints, the crop of that rectangle resized
// to S x S, and the same crop written straight into the Inception network's 299 x 299 input.  Interface and the rules restated
// from the reference: include/vunet_person_crop.h.
//
// The reference does this on the host per image (lib/utils.py:530-585: kp.cpu().numpy(), cv2.boundingRect, then
// kornia.crop_and_resize) and up-samples the stored crops a second time before the classifier (lib/metrics.py:385).  Here:
//   * kp_boxes_kernel: one wave per image; every lane takes joints lane, lane + 64, ..., then a butterfly min / max.
//   * box_crop_kernel: one thread per output pixel, threads along x, all channels from one coordinate.
//   * inception_input_boxes_kernel: one thread per pixel of the 299 x 299 input, the three channels from one set of taps: the four
//     taps of the virtual crop are box_sample() of the crop kernel, so the crop is never stored and never read back.
// The coordinates are float64 without fused multiply-adds (the sums are written in the order the CPU restatement of the tests
// uses), the bilinear weights fp32 and the three lerps explicit fmaf -- the same instructions wherever box_sample is inlined.
#include "common.h"
#include "../../include/vunet_inception.h"
#include "../../include/vunet_person_crop.h"

namespace {

__global__ __launch_bounds__(64) void kp_boxes_kernel(const float* __restrict__ kps, int J, int C, int* __restrict__ boxes,
                                                      int* __restrict__ valid) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const float* k = kps + (size_t)n * J * C;
  const float inf = __builtin_huge_valf();
  float xmin = inf, xmax = -inf, ymin = inf, ymax = -inf;
  for (int j = lane; j < J; j += 64) {
    const float x = k[(size_t)j * C], y = k[(size_t)j * C + 1];
    bool ok = x > 0.f && y > 0.f;
    if (C == 3) ok = ok && k[(size_t)j * C + 2] > 0.f;
    if (ok) {
      xmin = fminf(xmin, x);
      xmax = fmaxf(xmax, x);
      ymin = fminf(ymin, y);
      ymax = fmaxf(ymax, y);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    xmin = fminf(xmin, __shfl_xor(xmin, o, 64));
    xmax = fmaxf(xmax, __shfl_xor(xmax, o, 64));
    ymin = fminf(ymin, __shfl_xor(ymin, o, 64));
    ymax = fmaxf(ymax, __shfl_xor(ymax, o, 64));
  }
  if (lane == 0) {
    const bool any = xmax > 0.f;   // a counted keypoint has x > 0; none leaves -inf
    int x = 0, y = 0, w = 0, h = 0;
    if (any) {
      x = (int)floorf(xmin);
      y = (int)floorf(ymin);
      w = (int)floorf(xmax) - x + 1;
      h = (int)floorf(ymax) - y + 1;
    }
    boxes[4 * n] = x;
    boxes[4 * n + 1] = y;
    boxes[4 * n + 2] = w;
    boxes[4 * n + 3] = h;
    valid[n] = any ? 1 : 0;
  }
}

// The four source taps of crop pixel (i, j): their top-left index, which of them lie inside the image, and the two weights.
struct BoxTaps {
  int x0, y0;
  bool in_x0, in_x1, in_y0, in_y1;
  float fx, fy;
};

// one axis: the sampled coordinate of crop index `idx` of a box starting at `lo` with extent `ext` on an axis of `size` pixels
__device__ __forceinline__ void box_axis(int lo, int ext, int idx, int S, int size, int sampling, int& i0, bool& in0, bool& in1,
                                         float& frac) {
#pragma clang fp contract(off)
  double u = (double)lo + ((double)idx * (double)ext) / (double)(S - 1);
  if (sampling == VUNET_CROP_REFERENCE) u = (u * (double)size) / (double)(size - 1) - 0.5;
  const double f0 = floor(u);
  if (!(f0 >= -1.0 && f0 <= (double)(size - 1))) {   // both taps outside (or a coordinate that is not a number): zeros
    i0 = 0;
    in0 = in1 = false;
    frac = 0.f;
    return;
  }
  i0 = (int)f0;
  in0 = i0 >= 0;
  in1 = i0 + 1 <= size - 1;
  frac = (float)(u - f0);
}

__device__ __forceinline__ BoxTaps box_taps(const int* __restrict__ box, int i, int j, int S, int Hs, int Ws, int sampling) {
  BoxTaps t;
  box_axis(box[0], box[2], j, S, Ws, sampling, t.x0, t.in_x0, t.in_x1, t.fx);
  box_axis(box[1], box[3], i, S, Hs, sampling, t.y0, t.in_y0, t.in_y1, t.fy);
  return t;
}

// bilinear sample of one plane with zero padding: three fp32 lerps, each one fused multiply-add
__device__ __forceinline__ float box_sample(const float* __restrict__ plane, int Ws, const BoxTaps& t) {
  const size_t r0 = (size_t)t.y0 * Ws, r1 = r0 + Ws;
  const float a = (t.in_y0 && t.in_x0) ? plane[r0 + t.x0] : 0.f;
  const float b = (t.in_y0 && t.in_x1) ? plane[r0 + t.x0 + 1] : 0.f;
  const float c = (t.in_y1 && t.in_x0) ? plane[r1 + t.x0] : 0.f;
  const float d = (t.in_y1 && t.in_x1) ? plane[r1 + t.x0 + 1] : 0.f;
  const float top = fmaf(t.fx, b - a, a), bot = fmaf(t.fx, d - c, c);
  return fmaf(t.fy, bot - top, top);
}

__global__ __launch_bounds__(256) void box_crop_kernel(const float* __restrict__ img, int N, int Ch, int Hs, int Ws,
                                                       const int* __restrict__ boxes, const int* __restrict__ valid, int S, int sampling,
                                                       float* __restrict__ out) {
  const int64_t plane = (int64_t)S * S, e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)N * plane) return;
  const int n = (int)(e / plane), pix = (int)(e - (int64_t)n * plane);
  float* o = out + (size_t)n * Ch * plane + pix;
  if (!valid[n]) {
    for (int c = 0; c < Ch; ++c) o[(size_t)c * plane] = 0.f;
    return;
  }
  const int i = pix / S, j = pix - i * S;
  const BoxTaps t = box_taps(boxes + 4 * n, i, j, S, Hs, Ws, sampling);
  const size_t src_plane = (size_t)Hs * Ws;
  const float* s = img + (size_t)n * Ch * src_plane;
  for (int c = 0; c < Ch; ++c) o[(size_t)c * plane] = box_sample(s + c * src_plane, Ws, t);
}

__global__ __launch_bounds__(256) void inception_input_boxes_kernel(const float* __restrict__ img, int N, int Hs, int Ws,
                                                                    const int* __restrict__ boxes, const int* __restrict__ valid, int S,
                                                                    int sampling, int mode, float* __restrict__ y) {
  constexpr int Q = VUNET_INCEPTION_SIZE;
  const int64_t plane = (int64_t)Q * Q, e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)N * plane) return;
  const int n = (int)(e / plane), pix = (int)(e - (int64_t)n * plane);
  const int oy = pix / Q, ox = pix - oy * Q;
  // the resize of vunet_inception_input over the S x S crop (csrc/inception.hip: inception_input_kernel), expression for expression
  const double sy = fmax((oy + 0.5) * ((double)S / Q) - 0.5, 0.0), sx = fmax((ox + 0.5) * ((double)S / Q) - 0.5, 0.0);
  const int y0 = min((int)sy, S - 1), x0 = min((int)sx, S - 1);
  const int y1 = min(y0 + 1, S - 1), x1 = min(x0 + 1, S - 1);
  const double ly = sy - y0, lx = sx - x0;
  const bool ok = valid[n] != 0;
  BoxTaps t00, t01, t10, t11;
  if (ok) {
    const int* box = boxes + 4 * n;
    t00 = box_taps(box, y0, x0, S, Hs, Ws, sampling);
    t01 = box_taps(box, y0, x1, S, Hs, Ws, sampling);
    t10 = box_taps(box, y1, x0, S, Hs, Ws, sampling);
    t11 = box_taps(box, y1, x1, S, Hs, Ws, sampling);
  }
  const size_t src_plane = (size_t)Hs * Ws;
  const float* s = img + (size_t)n * 3 * src_plane;
  float* o = y + (size_t)n * 3 * plane + pix;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* sp = s + c * src_plane;
    double v00 = 0.0, v01 = 0.0, v10 = 0.0, v11 = 0.0;
    if (ok) {
      v00 = box_sample(sp, Ws, t00);
      v01 = box_sample(sp, Ws, t01);
      v10 = box_sample(sp, Ws, t10);
      v11 = box_sample(sp, Ws, t11);
    }
    double v = (1.0 - ly) * ((1.0 - lx) * v00 + lx * v01) + ly * ((1.0 - lx) * v10 + lx * v11);
    const double mean = c == 0 ? 0.485 : (c == 1 ? 0.456 : 0.406), sd = c == 0 ? 0.229 : (c == 1 ? 0.224 : 0.225);
    if (mode == 1) v = v * (sd / 0.5) + (mean - 0.5) / 0.5;
    else if (mode == 2) v = (fmin(fmax((v + 1.0) / 2.0, 0.0), 1.0) - mean) / sd;
    o[(size_t)c * plane] = (float)v;
  }
}

constexpr int64_t LIM = (int64_t)1 << 31;

bool crop_args_ok(int32_t N, int32_t Ch, int32_t Hs, int32_t Ws, int32_t S, int32_t sampling) {
  if (N < 1 || Ch < 1 || Hs < 1 || Ws < 1 || S < 2) return false;
  if (sampling != VUNET_CROP_REFERENCE && sampling != VUNET_CROP_EXACT) return false;
  if (sampling == VUNET_CROP_REFERENCE && (Hs < 2 || Ws < 2)) return false;
  return (int64_t)N * Ch * Hs * Ws < LIM;
}

}  // namespace

extern "C" int vunet_kp_boxes(const float* kps, int32_t N, int32_t J, int32_t C, int32_t* boxes, int32_t* valid, void* stream) {
  if (!kps || !boxes || !valid || N < 1 || J < 1 || (C != 2 && C != 3) || (int64_t)N * J * C >= LIM) return VUNET_ERR_ARG;
  VUNET_LAUNCH(kp_boxes_kernel, dim3((unsigned)N), dim3(64), 0, (hipStream_t)stream, kps, (int)J, (int)C, boxes, valid);
  return vunet_check_launch();
}

extern "C" int vunet_box_crop(const float* img, int32_t N, int32_t Ch, int32_t Hs, int32_t Ws, const int32_t* boxes,
                              const int32_t* valid, int32_t S, int32_t sampling, float* out, void* stream) {
  if (!img || !boxes || !valid || !out || !crop_args_ok(N, Ch, Hs, Ws, S, sampling)) return VUNET_ERR_ARG;
  if ((int64_t)N * Ch * S * S >= LIM) return VUNET_ERR_ARG;
  const int64_t total = (int64_t)N * S * S;
  VUNET_LAUNCH(box_crop_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, img, (int)N, (int)Ch, (int)Hs,
               (int)Ws, boxes, valid, (int)S, (int)sampling, out);
  return vunet_check_launch();
}

extern "C" int vunet_inception_input_boxes(const float* img, int32_t N, int32_t Hs, int32_t Ws, const int32_t* boxes,
                                           const int32_t* valid, int32_t S, int32_t sampling, int32_t mode, float* y, void* stream) {
  if (!img || !boxes || !valid || !y || !crop_args_ok(N, 3, Hs, Ws, S, sampling) || mode < 0 || mode > 2) return VUNET_ERR_ARG;
  if ((int64_t)N * 3 * VUNET_INCEPTION_SIZE * VUNET_INCEPTION_SIZE >= LIM || (int64_t)S * S >= LIM) return VUNET_ERR_ARG;
  const int64_t total = (int64_t)N * VUNET_INCEPTION_SIZE * VUNET_INCEPTION_SIZE;
  VUNET_LAUNCH(inception_input_boxes_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, img, (int)N,
               (int)Hs, (int)Ws, boxes, valid, (int)S, (int)sampling, (int)mode, y);
  return vunet_check_launch();
}
