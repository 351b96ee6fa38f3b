// The part-normalised appearance input (``data: inplane_normalize: True``): one homography per (image, body part) from the
// keypoints, then every part warped into a square.  Interface and the rules restated from the reference: include/vunet_inplane.h.
//
// The reference does this on the host per image: ten cv2.getPerspectiveTransform + cv2.warpPerspective calls
// (data/base_dataset.py:685-725, lib/utils.py:70-232).  Here:
//   * inplane_transforms_kernel: one thread per (image, part).  The 8x9 system sits in the thread's private memory (the pivot
//     search indexes it dynamically); the launch is N * P threads, a few hundred, nothing in it is worth a layout of its own.
//   * inplane_warp_kernel: one thread per output pixel, threads along x, the three channels of the part from one coordinate.
//     The nine doubles of a part are the same for the whole block.  No LDS, no atomics.
// The coordinates are float64 without fused multiply-adds (the sums are written in the order the CPU restatement of the tests
// uses), the bilinear weights and the blend fp32.
#include "common.h"
#include "../../include/vunet_inplane.h"

namespace {

struct P2 {
  double x, y;
};

__device__ __forceinline__ P2 mk(double x, double y) {
  P2 p;
  p.x = x;
  p.y = y;
  return p;
}

// a, b, c, d of a segment p0 -> p1 widened by alpha times its normal (lib/utils.py:173-180, :207-222)
__device__ __forceinline__ void segment_box(P2 p0, P2 p1, double alpha, P2& a, P2& b, P2& c, P2& d) {
#pragma clang fp contract(off)
  const double nx = -(p1.y - p0.y), ny = p1.x - p0.x;
  a = mk(p0.x + alpha * nx, p0.y + alpha * ny);
  b = mk(p0.x - alpha * nx, p0.y - alpha * ny);
  c = mk(p1.x - alpha * nx, p1.y - alpha * ny);
  d = mk(p1.x + alpha * nx, p1.y + alpha * ny);
}

// The four source points of one part; false where the reference's builder returns None.  dst: the destination corners.
__device__ bool part_points(const float* __restrict__ kps, int J, int kind, const int* __restrict__ ids, double wh, double oh, P2* src,
                            P2* dst) {
#pragma clang fp contract(off)
  const int n_ids = kind == VUNET_INPLANE_T2P ? 2 : kind == VUNET_INPLANE_T3P ? 3 : kind == VUNET_INPLANE_T4P ? 4
                    : kind == VUNET_INPLANE_T5P ? 5 : 0;
  if (n_ids == 0) return false;
  P2 k[VUNET_INPLANE_MAX_IDS];
  for (int i = 0; i < n_ids; ++i) {
    const int j = ids[i];
    if (j < 0 || j >= J) return false;
    k[i] = mk((double)kps[2 * j], (double)kps[2 * j + 1]);
  }
  if (kind == VUNET_INPLANE_T2P || kind == VUNET_INPLANE_T3P) {   // (0,0) (0,wh) (wh,wh) (wh,0); t2p: minus 1 throughout (:228)
    const double o = kind == VUNET_INPLANE_T2P ? 1.0 : 0.0;
    dst[0] = mk(0.0 - o, 0.0 - o);
    dst[1] = mk(0.0 - o, wh - o);
    dst[2] = mk(wh - o, wh - o);
    dst[3] = mk(wh - o, 0.0 - o);
  } else {                                                        // (0,0) (wh,0) (wh,wh) (0,wh)
    dst[0] = mk(0.0, 0.0);
    dst[1] = mk(wh, 0.0);
    dst[2] = mk(wh, wh);
    dst[3] = mk(0.0, wh);
  }
  if (kind == VUNET_INPLANE_T4P) {
    for (int i = 0; i < 4; ++i) src[i] = k[i];
    return true;
  }
  if (kind == VUNET_INPLANE_T5P) {   // :70-133
    const P2 rhip = k[0], neck = k[2], lhip = k[4];
    const P2 ls_to_rs = mk(k[1].x - k[3].x, k[1].y - k[3].y);
    const P2 rh_to_rs = mk(k[1].x - k[0].x, k[1].y - k[0].y);
    const P2 lh_to_ls = mk(k[3].x - k[4].x, k[3].y - k[4].y);
    const double den_l = ls_to_rs.y * lh_to_ls.x - ls_to_rs.x * lh_to_ls.y;
    const double den_r = ls_to_rs.y * rh_to_rs.x - ls_to_rs.x * rh_to_rs.y;
    const double lambda_l = (lhip.y - neck.y) * lh_to_ls.x / den_l + (neck.x - lhip.x) * lh_to_ls.y / den_l;
    const double lambda_r = (rhip.y - neck.y) * rh_to_rs.x / den_r + (neck.x - rhip.x) * rh_to_rs.y / den_r;
    src[0] = mk(neck.x + lambda_r * ls_to_rs.x, neck.y + lambda_r * ls_to_rs.y);
    src[1] = mk(neck.x + lambda_l * ls_to_rs.x, neck.y + lambda_l * ls_to_rs.y);
    src[2] = lhip;
    src[3] = rhip;
    return true;
  }
  P2 a, b, c, d;
  if (kind == VUNET_INPLANE_T3P) {   // :150-192; k = right shoulder, left shoulder, head
    const bool shoulders = k[0].x >= 0.0 && k[0].y >= 0.0 && k[1].x >= 0.0 && k[1].y >= 0.0;
    if (shoulders && k[2].x >= 0.0 && k[2].y >= 0.0) {
      const P2 neck = mk(0.5 * (k[0].x + k[1].x), 0.5 * (k[0].y + k[1].y));
      const P2 top = mk(neck.x + 2.0 * (k[2].x - neck.x), neck.y + 2.0 * (k[2].y - neck.y));
      segment_box(top, neck, 0.5, a, b, c, d);
    } else {
      if (!shoulders) return false;
      double nx = -(k[0].y - k[1].y), ny = k[0].x - k[1].x;
      if (ny > 0.0) {
        nx = -nx;
        ny = -ny;
      }
      a = mk(k[1].x + nx, k[1].y + ny);
      b = k[1];
      c = k[0];
      d = mk(k[0].x + nx, k[0].y + ny);
    }
    src[0] = b;
    src[1] = c;
    src[2] = d;
    src[3] = a;
    return true;
  }
  // t2p, :195-232
  const bool low0 = k[0].x <= 0.0 && k[0].y <= 0.0, low1 = k[1].x <= 0.0 && k[1].y <= 0.0;
  if (low0 || low1) {   // the leg fallback: from the one joint with both coordinates > 0 straight down to row oh - 1
    const bool pos0 = k[0].x > 0.0 && k[0].y > 0.0, pos1 = k[1].x > 0.0 && k[1].y > 0.0;
    if (!pos0 && !pos1) return false;
    const P2 t = pos0 ? k[0] : k[1];
    segment_box(t, mk(t.x, oh - 1.0), 0.25, a, b, c, d);
  } else {
    segment_box(k[0], k[1], 0.25, a, b, c, d);
  }
  src[0] = a;
  src[1] = b;
  src[2] = c;
  src[3] = d;
  return true;
}

// cv2.getPerspectiveTransform(src, dst) by Gaussian elimination with partial pivoting, then the inverse of the 3x3: minv maps
// destination to source.  false: a pivot or the determinant is not usable (see the header).
__device__ bool solve_inverse(const P2* src, const P2* dst, double* __restrict__ minv) {
#pragma clang fp contract(off)
  double A[8][9];
  double amax = 0.0;
  for (int i = 0; i < 4; ++i) {
    const double x = src[i].x, y = src[i].y, X = dst[i].x, Y = dst[i].y;
    const double r0[9] = {x, y, 1.0, 0.0, 0.0, 0.0, -x * X, -y * X, X};
    const double r1[9] = {0.0, 0.0, 0.0, x, y, 1.0, -x * Y, -y * Y, Y};
    for (int j = 0; j < 9; ++j) {
      A[i][j] = r0[j];
      A[i + 4][j] = r1[j];
      if (j < 8) amax = fmax(amax, fmax(fabs(r0[j]), fabs(r1[j])));
    }
  }
  if (!isfinite(amax)) return false;
  const double tiny = 1e-9 * amax;
  for (int c = 0; c < 8; ++c) {
    int r = c;
    double best = fabs(A[c][c]);
    for (int i = c + 1; i < 8; ++i) {
      const double v = fabs(A[i][c]);
      if (v > best) {
        best = v;
        r = i;
      }
    }
    if (!isfinite(best) || best < tiny) return false;
    if (r != c)
      for (int j = 0; j < 9; ++j) {
        const double t = A[c][j];
        A[c][j] = A[r][j];
        A[r][j] = t;
      }
    for (int i = c + 1; i < 8; ++i) {
      const double f = A[i][c] / A[c][c];
      for (int j = c + 1; j < 9; ++j) A[i][j] = A[i][j] - f * A[c][j];
      A[i][c] = 0.0;
    }
  }
  double h[9];
  for (int c = 7; c >= 0; --c) {
    double s = A[c][8];
    for (int j = c + 1; j < 8; ++j) s = s - A[c][j] * h[j];
    h[c] = s / A[c][c];
  }
  h[8] = 1.0;
  const double c0 = h[4] * h[8] - h[5] * h[7], c1 = h[3] * h[8] - h[5] * h[6], c2 = h[3] * h[7] - h[4] * h[6];
  const double det = (h[0] * c0 - h[1] * c1) + h[2] * c2;
  if (!isfinite(det) || det == 0.0) return false;
  minv[0] = c0 / det;
  minv[1] = (h[2] * h[7] - h[1] * h[8]) / det;
  minv[2] = (h[1] * h[5] - h[2] * h[4]) / det;
  minv[3] = -c1 / det;
  minv[4] = (h[0] * h[8] - h[2] * h[6]) / det;
  minv[5] = (h[2] * h[3] - h[0] * h[5]) / det;
  minv[6] = c2 / det;
  minv[7] = (h[1] * h[6] - h[0] * h[7]) / det;
  minv[8] = (h[0] * h[4] - h[1] * h[3]) / det;
  for (int i = 0; i < 9; ++i)
    if (!isfinite(minv[i])) return false;
  return true;
}

__global__ __launch_bounds__(64) void inplane_transforms_kernel(const float* __restrict__ kps, int N, int J, const int* __restrict__ kinds,
                                                                const int* __restrict__ ids, int P, double wh, double oh,
                                                                double* __restrict__ minv, double* __restrict__ src_out,
                                                                int* __restrict__ valid) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= N * P) return;
  const int n = t / P, p = t - n * P;
  P2 src[4], dst[4];
  double m[9];
  bool ok = part_points(kps + (size_t)n * J * 2, J, kinds[p], ids + p * VUNET_INPLANE_MAX_IDS, wh, oh, src, dst);
  if (!ok)
    for (int i = 0; i < 4; ++i) src[i] = mk(0.0, 0.0);
  for (int i = 0; i < 4; ++i) ok = ok && isfinite(src[i].x) && isfinite(src[i].y);
  ok = ok && solve_inverse(src, dst, m);
  for (int i = 0; i < 4; ++i) {
    src_out[(size_t)t * 8 + 2 * i] = src[i].x;
    src_out[(size_t)t * 8 + 2 * i + 1] = src[i].y;
  }
  for (int i = 0; i < 9; ++i) minv[(size_t)t * 9 + i] = ok ? m[i] : 0.0;
  valid[t] = ok ? 1 : 0;
}

__global__ __launch_bounds__(256) void inplane_warp_kernel(const float* __restrict__ img, int Hs, int Ws, const double* __restrict__ minv,
                                                           const int* __restrict__ valid, int P, int S, float absent,
                                                           float* __restrict__ out) {
#pragma clang fp contract(off)
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= S * S) return;
  const int p = blockIdx.y, n = blockIdx.z;
  const size_t part = (size_t)n * P + p, plane = (size_t)S * S;
  float* o = out + part * 3 * plane + pix;
  if (!valid[part]) {
    o[0] = absent;
    o[plane] = absent;
    o[2 * plane] = absent;
    return;
  }
  const double* m = minv + part * 9;
  const int yi = pix / S, xi = pix - yi * S;
  const double x = (double)xi, y = (double)yi;
  const double u = (m[0] * x + m[1] * y) + m[2], v = (m[3] * x + m[4] * y) + m[5], w = (m[6] * x + m[7] * y) + m[8];
  double sx = 0.0, sy = 0.0;
  if (w != 0.0) {
    sx = u / w;
    sy = v / w;
  }
  // BORDER_REPLICATE: the clamped coordinate (fmax / fmin drop a NaN: it lands on 0)
  sx = fmin(fmax(sx, 0.0), (double)(Ws - 1));
  sy = fmin(fmax(sy, 0.0), (double)(Hs - 1));
  const double fx0 = floor(sx), fy0 = floor(sy);
  const int x0 = (int)fx0, y0 = (int)fy0, x1 = min(x0 + 1, Ws - 1), y1 = min(y0 + 1, Hs - 1);
  const float fx = (float)(sx - fx0), fy = (float)(sy - fy0);
  const size_t src_plane = (size_t)Hs * Ws;
  const float* s = img + (size_t)n * 3 * src_plane;
  const size_t i00 = (size_t)y0 * Ws + x0, i01 = (size_t)y0 * Ws + x1, i10 = (size_t)y1 * Ws + x0, i11 = (size_t)y1 * Ws + x1;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float* sc = s + c * src_plane;
    const float a = sc[i00], b = sc[i01], cc = sc[i10], d = sc[i11];
    const float top = a + fx * (b - a), bot = cc + fx * (d - cc);
    o[c * plane] = top + fy * (bot - top);
  }
}

}  // namespace

extern "C" int vunet_inplane_transforms(const float* kps, int32_t N, int32_t J, const int32_t* kinds, const int32_t* ids, int32_t P,
                                        int32_t s_out, double oh, double* minv, double* src, int32_t* valid, void* stream) {
  if (!kps || !kinds || !ids || !minv || !src || !valid || N < 1 || J < 1 || P < 1 || P > VUNET_INPLANE_MAX_PARTS || s_out < 1 ||
      (int64_t)N * P > 0x7FFFFFFF)
    return VUNET_ERR_ARG;
  VUNET_LAUNCH(inplane_transforms_kernel, dim3((unsigned)((N * P + 63) / 64)), dim3(64), 0, (hipStream_t)stream, kps, N, J, kinds, ids, P,
               (double)s_out, oh, minv, src, valid);
  return vunet_check_launch();
}

extern "C" int vunet_inplane_warp(const float* img, int32_t N, int32_t Hs, int32_t Ws, const double* minv, const int32_t* valid,
                                  int32_t P, int32_t s_out, float absent, float* out, void* stream) {
  if (!img || !minv || !valid || !out || N < 1 || N > 65535 || Hs < 1 || Ws < 1 || P < 1 || P > VUNET_INPLANE_MAX_PARTS || s_out < 1 ||
      s_out > 32768)
    return VUNET_ERR_ARG;
  VUNET_LAUNCH(inplane_warp_kernel, dim3((unsigned)((s_out * s_out + 255) / 256), (unsigned)P, (unsigned)N), dim3(256), 0,
               (hipStream_t)stream, img, Hs, Ws, minv, valid, P, s_out, absent, out);
  return vunet_check_launch();
}
