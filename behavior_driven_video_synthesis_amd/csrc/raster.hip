// Pose "stickman" rasteriser on the GPU (lib/utils.py:325-512 make_joint_img; data/human36m.py:808-848).
//
// The reference draws each frame on the CPU with cv2.fillPoly / cv2.line, one Python call per
// primitive.  Here every pixel decides for itself: a workgroup first reduces the frame's draw list to
// integer parameters in LDS (clipped, left-to-right-normalised Bresenham lines; the polygon's 16.16
// fixed-point edge table), then each thread evaluates, for four adjacent pixels, the *closed forms* of
// the two OpenCV primitives -- "is (x, y) the pixel LineIterator visits at its major-axis step?" and
// "does (x, y) fall in an even-odd scan-line span?" -- and keeps the colour of the last command that
// covers it (draw order = overwrite order).  Command kinds: 0 body polygon, 1 line between two joints, 4 head line
// (a line that also feeds the "throat length"), 2 neck line (midpoint of the two shoulders -> head joint, drawn
// when the model has no head lines, lib/utils.py:407-433), 3 face line (drawn only if shorter than the throat
// length, :468-505).  Pure integer work (plus the double-precision clip intersection OpenCV itself uses and the
// float64 midpoint / Euclidean lengths of the neck and face rules): bit-exact against the sequential restatement in
// oracle/stickman_oracle.c.  Stores are 4 bytes per lane, 256 B per wavefront; the optional fp32 output
// applies ToTensor and *2-1 (data/base_dataset.py:183-190, data/__init__.py:23-24).
#include "common.h"
#include "raster_forms.h"

__global__ __launch_bounds__(256) void stickman_raster_kernel(const float* __restrict__ kps, int J,
                                                              const int* __restrict__ body, int n_body,
                                                              const int* __restrict__ cmds, int n_cmds,
                                                              uint8_t* __restrict__ out_u8, float* __restrict__ out_f32,
                                                              int H, int W, int thickness) {
  extern __shared__ __attribute__((aligned(16))) unsigned char thick_raw[];   // RThick[n_cmds] when thickness > 1
  RThick* const thick = reinterpret_cast<RThick*>(thick_raw);
  __shared__ int chw[R_MAXRAD + 1];   // filled-circle half widths per row offset (thickness > 1)
  const int radius = thickness > 1 ? ((thickness << (XY_SHIFT - 1)) + (XY_ONE >> 1)) >> XY_SHIFT : 0;
  __shared__ RLine lines[R_MAXCMD];
  __shared__ RPoly poly;
  __shared__ int ckind[R_MAXCMD], cplane[R_MAXCMD], ccolor[R_MAXCMD];
  __shared__ double clen[R_MAXCMD];   // Euclidean length of the command's segment (float64, as np.linalg.norm)
  const int b = blockIdx.x, tid = threadIdx.x;
  const float* k = kps + (size_t)b * J * 2;

  if (tid < n_cmds) {
    const int* c = cmds + 6 * tid;    // {kind, joint a, joint b, joint c, plane, colour}
    ckind[tid] = c[0];
    cplane[tid] = c[4];
    ccolor[tid] = c[5];
    RLine L;
    L.valid = 0;
    double len = 0.0;
    if (c[0] == 1 || c[0] == 3 || c[0] == 4) {
      const float ax = k[2 * c[1]], ay = k[2 * c[1] + 1], bx = k[2 * c[2]], by = k[2 * c[2] + 1];
      if (ax >= 0.f && ay >= 0.f && bx >= 0.f && by >= 0.f) {
        L = r_make_line((long long)ax, (long long)ay, (long long)bx, (long long)by, W, H);
        if (thickness > 1) {
          r_make_thick(thick[tid], (long long)ax, (long long)ay, (long long)bx, (long long)by, thickness, W, H);
          L.valid |= 1;   // a thick line is drawn whether or not its centre line survives the clip
        }
        const double dx = (double)ax - (double)bx, dy = (double)ay - (double)by;
        len = __dsqrt_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)));
        if (c[0] == 3) L.valid |= 2;   // face line: still waits for the throat-length test (bit 1)
        if (c[0] == 4) L.valid |= 4;   // head line: clipped away or not, a valid one feeds the throat length (bit 2)
      }
    } else if (c[0] == 2) {
      // neck = 0.5 * (rshoulder + lshoulder) if neither has a negative coordinate, else (-1, -1)  (:408-413)
      const float rx = k[2 * c[1]], ry = k[2 * c[1] + 1], lx = k[2 * c[2]], ly = k[2 * c[2] + 1];
      const float hx = k[2 * c[3]], hy = k[2 * c[3] + 1];
      if (rx >= 0.f && ry >= 0.f && lx >= 0.f && ly >= 0.f && hx >= 0.f && hy >= 0.f) {
        const double nx = 0.5 * ((double)rx + (double)lx), ny = 0.5 * ((double)ry + (double)ly);
        L = r_make_line((long long)nx, (long long)ny, (long long)hx, (long long)hy, W, H);
        if (thickness > 1) {
          r_make_thick(thick[tid], (long long)nx, (long long)ny, (long long)hx, (long long)hy, thickness, W, H);
          L.valid |= 1;
        }
        const double dx = nx - (double)hx, dy = ny - (double)hy;
        len = __dsqrt_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)));
        L.valid |= 4;                  // drawn or not, a valid neck segment defines the throat length
      }
    }
    lines[tid] = L;
    clen[tid] = len;
  }
  if (tid == 254 && thickness > 1) {   // OpenCV Circle(fill): the midpoint iteration, widest span per row offset
    for (int r = 0; r <= radius; ++r) chw[r] = -1;
    int err = 0, dx = radius, dy = 0, plus = 1, minus = (radius << 1) - 1;
    while (dx >= dy) {
      chw[dy] = max(chw[dy], dx);
      chw[dx] = max(chw[dx], dy);
      dy++;
      err += plus;
      plus += 2;
      const int mask = (err <= 0) - 1;
      err -= minus & mask;
      dx += mask;
      minus -= mask & 2;
    }
  }
  if (tid == 255) {  // the body polygon (shared by every polygon command)
    RPoly P;
    P.valid = 0;
    P.fill_valid = 0;
    P.nv = P.ne = 0;
    long long vx[R_MAXV], vy[R_MAXV];
    int n = 0;
    if (n_body > 2)
      for (int i = 0; i < n_body && n < R_MAXV; ++i) {
        const float x = k[2 * body[i]], y = k[2 * body[i] + 1];
        if (x >= 0.f && y >= 0.f) { vx[n] = (long long)x; vy[n] = (long long)y; ++n; }
      }
    if (n > 2) {
      P.valid = 1;
      P.nv = n;
      long long px = vx[n - 1] << XY_SHIFT, py = vy[n - 1];
      int ymax = INT_MIN, ymin = INT_MAX;
      long long xmax = -1, xmin = LLONG_MAX;
      for (int i = 0; i < n; ++i) {
        const long long qx = vx[i] << XY_SHIFT, qy = vy[i];
        P.bl[i] = r_make_line((px + (XY_ONE >> 1)) >> XY_SHIFT, py, (qx + (XY_ONE >> 1)) >> XY_SHIFT, qy, W, H);
        if (py != qy) {
          const int e = P.ne++;
          if (py < qy) { P.ey0[e] = (int)py; P.ey1[e] = (int)qy; P.ex[e] = px; }
          else { P.ey0[e] = (int)qy; P.ey1[e] = (int)py; P.ex[e] = qx; }
          P.edx[e] = (qx - px) / (qy - py);
          const long long x1 = P.ex[e] + (long long)(P.ey1[e] - P.ey0[e]) * P.edx[e];
          ymin = min(ymin, P.ey0[e]);
          ymax = max(ymax, P.ey1[e]);
          xmin = min(xmin, min(P.ex[e], x1));
          xmax = max(xmax, max(P.ex[e], x1));
        }
        px = qx;
        py = qy;
      }
      P.ymin = ymin;
      P.ymax = ymax;
      P.fill_valid = P.ne >= 2 && !(ymax < 0 || ymin >= H || xmax < 0 || xmin >= ((long long)W << XY_SHIFT));
    }
    poly = P;
  }
  __syncthreads();
  if (tid == 0) {   // throat length = longest valid head / neck segment (:415-417, :466-467); then the face-line test
    double throat = 0.0;
    for (int c = 0; c < n_cmds; ++c)
      if ((ckind[c] == 2 || ckind[c] == 4) && (lines[c].valid & 4)) throat = fmax(throat, clen[c]);
    for (int c = 0; c < n_cmds; ++c) {
      int v = lines[c].valid;
      if (ckind[c] == 3) v = ((v & 2) && clen[c] < throat) ? (v & 1) : 0;
      lines[c].valid = v & 1;
    }
  }
  __syncthreads();

  const int W4 = W >> 2;  // W % 4 == 0 (checked by the host)
  for (int q = blockIdx.y * 256 + tid; q < H * W4; q += gridDim.y * 256) {
    const int y = q / W4, x0 = (q - y * W4) * 4;
    uint32_t packed[3] = {0u, 0u, 0u};
#pragma unroll
    for (int dxp = 0; dxp < 4; ++dxp) {
      const int x = x0 + dxp;
      int val[3] = {0, 0, 0};
      const bool inp = r_in_poly(poly, x, y, H);
      for (int c = 0; c < n_cmds; ++c) {
        const bool hit = ckind[c] == 0 ? inp
                         : (thickness > 1 ? (lines[c].valid && r_in_thick(thick[c], chw, radius, x, y, W))
                                          : r_on_line(lines[c], x, y));
        if (hit) val[cplane[c]] = ccolor[c];
      }
#pragma unroll
      for (int p = 0; p < 3; ++p) packed[p] |= (uint32_t)(val[p] & 255) << (8 * dxp);
    }
#pragma unroll
    for (int p = 0; p < 3; ++p) {
      const size_t o = (((size_t)b * 3 + p) * H + y) * W + x0;
      if (out_u8) *reinterpret_cast<uint32_t*>(out_u8 + o) = packed[p];
      if (out_f32) {
        float4 f;
        f.x = ((float)(packed[p] & 255u) / 255.0f) * 2.0f - 1.0f;
        f.y = ((float)((packed[p] >> 8) & 255u) / 255.0f) * 2.0f - 1.0f;
        f.z = ((float)((packed[p] >> 16) & 255u) / 255.0f) * 2.0f - 1.0f;
        f.w = ((float)(packed[p] >> 24) / 255.0f) * 2.0f - 1.0f;
        *reinterpret_cast<float4*>(out_f32 + o) = f;
      }
    }
  }
}

extern "C" int vunet_stickman_raster_thick(const float* kps, int32_t B, int32_t J, const int32_t* body, int32_t n_body,
                                           const int32_t* cmds, int32_t n_cmds, uint8_t* out_u8, float* out_f32, int32_t H,
                                           int32_t W, int32_t thickness, void* stream) {
  if (!kps || !cmds || (!out_u8 && !out_f32) || B < 1 || J < 1 || H < 1 || W < 4 || (W & 3)) return VUNET_ERR_ARG;
  if (n_cmds < 0 || n_cmds > R_MAXCMD || n_body < 0 || n_body > R_MAXV || (n_body > 0 && !body)) return VUNET_ERR_ARG;
  if (thickness < 1 || thickness > 2 * R_MAXRAD - 1) return VUNET_ERR_ARG;
  int gy = (H * (W >> 2) + 255) / 256;
  if (gy > 64) gy = 64;
  const size_t lds = thickness > 1 ? (size_t)n_cmds * sizeof(RThick) : 0;
  VUNET_LAUNCH(stickman_raster_kernel, dim3((unsigned)B, (unsigned)gy), dim3(256), lds, (hipStream_t)stream, kps, J, body,
               n_body, cmds, n_cmds, out_u8, out_f32, H, W, thickness);
  return vunet_check_launch();
}

extern "C" int vunet_stickman_raster(const float* kps, int32_t B, int32_t J, const int32_t* body, int32_t n_body,
                                     const int32_t* cmds, int32_t n_cmds, uint8_t* out_u8, float* out_f32, int32_t H,
                                     int32_t W, void* stream) {
  return vunet_stickman_raster_thick(kps, B, J, body, n_body, cmds, n_cmds, out_u8, out_f32, H, W, 1, stream);
}
